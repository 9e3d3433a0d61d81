#!/usr/bin/env python3
"""Golden outputs and gradients of the two CLIP towers trained through their token outputs, produced by the UNMODIFIED
reference VisionTransformer(return_patches=True) and CLIP.encode_text of a return_patches=True model (models/CLIP/model.py) through
oracle._ref_import, on the CPU in fp32: python tools/make_golden_tower_tokens.py [DIR] -> tests/golden/tower_tokens.npz (or DIR/).
Needs the reference checkout; nothing at test time runs or imports this.

Cases, seeds, the loss and the float64 restatement live in tests/tower_tokens_cases.py.  Per case <c>: `<c>__seed`, `<c>__checksum` of
the regenerated parameters / inputs / upstream gradients / mask, the reference's fp32 `<c>__y_cls`, `<c>__y_tok` and `<c>__g_<tensor>`
(thinned), per tensor `<c>__eref_<tensor>` = max|fp32 - fp64| / max|fp64| on the whole tensor, the fp64 side being the restatement,
and `<c>__bit_equal` = 1 when the restatement's own fp32 run equals the reference's to the bit in every tensor.  That is printed and
recorded, not required: the reference normalises and multiplies the text rows in [L, B] order and the restatement in [B, L] order.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tower_tokens_cases as TT  # noqa: E402
from oracle import _ref_import  # noqa: E402
from oracle.fixtures import out_path  # noqa: E402

_ref_import.setup()
from models.CLIP.model import CLIP, VisionTransformer  # noqa: E402  (the reference classes)


def _collect(tower, m, cls, tokens, layers, prefix):
    out = {"y_cls": cls.detach().numpy().copy(), "y_tok": tokens.detach().numpy().copy()}
    for name in TT.tensor_names(tower, layers)[2:]:
        out[name] = m.get_parameter(TT.tensor_key(tower, name)[len(prefix):]).grad.numpy().copy()
    return out


def run_reference(tower, sd, x, ups, kpm):
    """the reference's tower in fp32 -> the dict run_restatement returns"""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        layers = TT.count_layers(tower, sd)
        ups = [torch.tensor(u) for u in ups]
        if tower == "img":
            D, out_dim = sd["visual.proj"].shape
            patch = sd["visual.conv1.weight"].shape[-1]
            res = patch * round((sd["visual.positional_embedding"].shape[0] - 1) ** 0.5)
            m = VisionTransformer(res, patch, D, layers, D // 64, out_dim, return_patches=True)
            m.load_state_dict({k[len("visual."):]: torch.tensor(v) for k, v in sd.items()}, strict=True)
            cls, tokens, _ = m(torch.tensor(x))
            TT.loss_of(cls, tokens, ups).backward()
            return _collect(tower, m, cls, tokens, layers, "visual.")
        D, out_dim = sd["text_projection"].shape
        vocab, context = sd["token_embedding.weight"].shape[0], sd["positional_embedding"].shape[0]
        m = CLIP(out_dim, 4, 0, 64, 4, context, vocab, D, D // 64, layers, return_patches=True)
        missing, unexpected = m.load_state_dict({k: torch.tensor(v) for k, v in sd.items()}, strict=False)
        assert not unexpected and all(k.startswith("visual.") or k == "logit_scale" for k in missing), (missing, unexpected)
        cls, tokens, _, _ = m.encode_text(torch.tensor(x), key_padding_mask=None if kpm is None else torch.tensor(kpm))
        TT.loss_of(cls, tokens, ups).backward()
        return _collect(tower, m, cls, tokens, layers, "")
    finally:
        torch.set_num_threads(threads)


def main():
    out, pool = {}, {"img": {}, "txt": {}}
    for name in TT.CASES:
        tower = TT.tower_of(name)
        sd, x, ups, kpm = TT.case_inputs(name)
        ref = run_reference(tower, sd, x, ups, kpm)
        r32 = TT.run_restatement(tower, sd, x, ups, kpm, torch.float32)
        r64 = TT.run_restatement(tower, sd, x, ups, kpm, torch.float64)
        assert sorted(ref) == sorted(r32) == sorted(r64)
        differ = []
        for k in ref:
            assert np.isfinite(ref[k]).all(), (name, k)
            ref[k] = ref[k].reshape(r32[k].shape)
            if not np.array_equal(ref[k], r32[k]):
                differ.append("%s %.1e" % (k, TT.rel_err(ref[k], r32[k])))
        print("%-26s the restatement's fp32 run %s" % (name, "equals the reference's to the bit" if not differ else
                                                        "differs from the reference's in: " + ", ".join(differ)))
        per, pl = TT.erefs(ref, r64)                                 # the reference's own fp32 error
        out[name + "__seed"] = np.int64(TT.case_seed(name))
        out[name + "__checksum"] = np.float64(TT.inputs_checksum(sd, x, ups, kpm))
        out[name + "__bit_equal"] = np.int64(not differ)
        for k in ref:
            out["%s__%s" % (name, k)] = TT.thin(ref[k]).astype(np.float32)
            out["%s__eref_%s" % (name, k)] = np.float64(per[k])
        for k, e in pl.items():
            pool[tower][k] = max(pool[tower].get(k, 0.0), e)
        print("%-26s %s" % ("", " ".join("%s %.1e" % (k[2:], pl[k]) for k in TT.KINDS[tower])))
    for tower in pool:
        print("pooled e_ref (%s):" % tower, " ".join("%s %.2e" % (k, pool[tower][k]) for k in TT.KINDS[tower]))
    path = out_path("tower_tokens.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
