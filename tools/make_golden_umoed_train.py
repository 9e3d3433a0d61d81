#!/usr/bin/env python3
"""Golden values of UMoED's decoder head in TRAIN mode, produced by the UNMODIFIED reference TokenHash (models/UMoED/hash/hash_moe.py with
its SoftMoEDecoder) through oracle._ref_import, on the CPU in ``.train()`` mode, in float64 and float32:
python tools/make_golden_umoed_train.py [DIR] -> tests/golden/umoed_train.npz (or DIR/).  Needs the reference checkout and einops;
nothing at test time runs or imports this.

The one case is umoed_train_cases.GOLDEN_CASE (the reference's dim_feedforward is always 2048), in two settings: ``dropout=0.0``, and
p = 0.3 with the masks of the case's seed REPLAYED.  The replay patches torch, not the reference: ``torch.nn.functional.dropout`` hands out
the stored masks in the order they are asked for, and ``torch.nn.functional.scaled_dot_product_attention`` (where nn.MultiheadAttention
applies its dropout with need_weights=False) becomes the explicit softmax -> dropout -> P V in torch ops.  It is asserted that exactly
six masks per layer were consumed, with the documented shapes in the documented order (include/xmh.h).

Parameters, tokens, the upstream G and the masks are drawn from the seeds of tests/umoed_train_cases.py and never stored.  Recorded, per
setting and dtype, ``embeds`` and the gradient of sum(embeds * G) with respect to the tokens and every parameter -- whole up to 256
elements, otherwise 64 sampled values with the tensor's sum and sum of squares, all in one vector (umoed_train_cases.golden_vector):
  train__<setting>__{f64,f32},  train__seed
Before writing it asserts the case's ReLU guard and that the float64 restatement reproduces the reference to 1e-12."""
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import umoed_cases as UC  # noqa: E402
import umoed_train_cases as TC  # noqa: E402
from oracle import _ref_import  # noqa: E402
from oracle.fixtures import out_path  # noqa: E402

_ref_import.setup()
for ns in ("UMoED", "UMoED/hash"):                              # bare: the packages' __init__ pull the registry in
    _ref_import._ns("models." + ns.replace("/", "."), os.path.join(_ref_import.REF, "models", *ns.split("/")))
from models.UMoED.hash.hash_moe import HashLayer  # noqa: E402  (the reference's own module)


class Replay:
    """torch.nn.functional.dropout and scaled_dot_product_attention for the time of one forward: the stored masks, in order"""

    def __init__(self, masks, p):
        self.queue = [m for layer in masks for m in layer]
        self.p, self.used = p, []

    def dropout(self, input, p=0.5, training=True, inplace=False):
        assert training and abs(p - self.p) < 1e-12, (training, p)
        keep = self.queue[len(self.used)]
        assert keep.size == input.numel(), (len(self.used), keep.shape, tuple(input.shape))
        self.used.append(tuple(input.shape))
        return input * torch.tensor(keep).to(input.dtype).reshape(input.shape) * (1.0 / (1.0 - p))

    def sdpa(self, query, key, value, attn_mask=None, dropout_p=0.0, is_causal=False, scale=None, **kw):
        assert attn_mask is None and not is_causal and scale is None and query.dim() == 4
        P = torch.softmax((query / math.sqrt(query.shape[-1])) @ key.transpose(-1, -2), dim=-1)
        return (self.dropout(P, dropout_p, True) if dropout_p > 0 else P) @ value

    def __enter__(self):
        self.saved = (F.dropout, F.scaled_dot_product_attention)
        F.dropout, F.scaled_dot_product_attention = self.dropout, self.sdpa
        return self

    def __exit__(self, *exc):
        F.dropout, F.scaled_dot_product_attention = self.saved


def ref_run(c, which, dtype):
    masks, p = TC.setting(c, which)
    layer = HashLayer(visual_tokens=c["T"], txt_tokens=0, img_feature_size=c["E"], txt_feature_size=c["E"], outputDim=c["V"], setDim=c["M"],
                      dropout=p, decoder_heads=c["heads"], decoder_layers=c["layers"], num_experts=c["n"], slots_per_expert=c["p"], MoE=True,
                      fusion=True, hidden_dim=c["d"], hash_func_=c["hash_func"], merge_func_=UC.MERGE_OF[c["hash_func"]]).to(dtype).train()
    head = layer.hash_module
    assert list(head.state_dict()) == list(c["P"])
    head.load_state_dict({k: torch.tensor(v).to(dtype) for k, v in c["P"].items()}, strict=True)
    x = torch.tensor(c["x"]).to(dtype).requires_grad_(True)
    if masks is None:
        embeds, _ = head(x)
    else:
        with Replay(masks, p) as r:
            embeds, _ = head(x)
        B, M = c["B"], c["M"]
        want = [tuple(s) for _ in range(c["layers"]) for s in TC.keep_shapes(c)]
        assert len(r.used) == 6 * c["layers"], (len(r.used), r.used)
        assert [int(np.prod(s)) for s in r.used] == [int(np.prod(s)) for s in want], (r.used, want)
        assert r.used[0] == want[0] and r.used[2] == want[2] and r.used[4] == (B, M, c["F"]), r.used[:6]
    (embeds * torch.tensor(c["G"]).to(dtype)).sum().backward()
    out = {"embeds": embeds.detach().double().numpy(), "g_tokens": x.grad.double().numpy()}
    for k, v in head.named_parameters():
        out["g_" + k] = v.grad.double().numpy()
    return out


def main():
    c = TC.case("golden")
    gap = TC.case_gap(c)
    assert gap >= TC.RELU_GAP, gap
    out = {"train__seed": np.array(c["seed"])}
    for which in TC.SETTINGS:
        r64, r32 = ref_run(c, which, torch.float64), ref_run(c, which, torch.float32)
        mine = TC.reference("golden", which)
        assert set(mine) == set(r64), sorted(set(mine) ^ set(r64))
        worst = 0.0
        for key in r64:
            e = UC.rel_err(mine[key], r64[key])
            worst = max(worst, e)
            assert e <= 1e-12, (which, key, e)
        out["train__%s__f64" % which] = TC.golden_vector(r64)[0]
        out["train__%s__f32" % which] = TC.golden_vector(r32)[0].astype(np.float32)
        print(which, "ReLU gap %.2e" % gap, "restatement against the reference %.2e" % worst, "f32 - f64, worst tensor %.2e"
              % max(UC.rel_err(r32[k], r64[k]) for k in r64))
    path = out_path("umoed_train.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
