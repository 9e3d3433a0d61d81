#!/usr/bin/env python3
"""Golden values of DIMCH's training objective, produced by the UNMODIFIED reference (models/DIMCH: DIMCH.object_function on an
instance made without its constructor, SetwiseDistance, TripletLoss, plus torch's autograd) through oracle._ref_import, on the CPU in
float32 and in float64: python tools/make_golden_dimch.py [DIR] -> tests/golden/dimch.npz (or DIR/).  Needs the reference checkout
and einops (the reference's diversity term calls it); nothing at test time runs or imports this.

SetwiseDistance's constructor moves two scalars to the GPU (``.cuda()``); this process has none, so that one call is made a no-op
here, in this process only.  Cases: tests/dimch_cases.py:GOLDEN_CASES -- all four distance modes at (B, M, K) = (7, 5, 6), the
configuration's smooth_chamfer at (20, 8, 16) and at (9, 64, 32), and hash_func softmax once.  N = B M stays at or below 576: the
reference's diversity term builds an [N, N, N] tensor.  Per case and dtype: the loss, every entry of the loss dictionary and the four
gradients; the inputs and constants once; the largest float32-against-float64 deviation per tensor kind is printed and recorded.

The head (models/DIMCH/hash/hash.py): the state-dict keys and shapes of HashLayer(50, 32, 512, 16, setDim=8) under ``state__<key>``,
and under ``head__*`` one forward and backward of an image-side TokenHash at T = 5, E = 64, M = 3, K = 6 in eval mode (B = 4: the
reference's ``.squeeze()`` drops the batch axis at B = 1), in float32 and float64: parameters, tokens, the two upstream gradients,
both outputs and the gradients of sum(embeds g_embeds) + sum(hash g_hash)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dimch_cases as DC  # noqa: E402
from oracle import _ref_import  # noqa: E402
from oracle.fixtures import out_path  # noqa: E402

_ref_import.setup()
_ref_import._ns("models.DIMCH", os.path.join(_ref_import.REF, "models", "DIMCH"))      # bare: the package's __init__ pulls the registry in
_ref_import._ns("models.DIMCH.hash", os.path.join(_ref_import.REF, "models", "DIMCH", "hash"))
torch.Tensor.cuda = lambda self, *a, **k: self                                          # see the module text
from models.DIMCH import DIMCH as ref_dimch  # noqa: E402  (the reference's own module)
from models.DIMCH.distance import SetwiseDistance  # noqa: E402
from models.DIMCH.loss.triplet_loss import TripletLoss  # noqa: E402
from models.DIMCH.hash.hash import HashLayer  # noqa: E402


def instance(c):
    k = DC.consts(c)
    m = ref_dimch.DIMCH.__new__(ref_dimch.DIMCH)
    torch.nn.Module.__init__(m)
    m.hash_func = k["hash_func"]
    m.triplet_loss = TripletLoss(reduction="mean")
    m.distance = SetwiseDistance(img_set_size=c["M"], txt_set_size=c["M"], denominator=k["denominator"], temperature=k["temperature"],
                                 temperature_txt_scale=k["temperature_txt_scale"], mode=k["mode"])
    m.chamfer_parmeters = {"set_size": c["M"], "mmd_alpha": k["mmd_alpha"], "unif_alpha": k["unif_alpha"], "mmd_gamma": k["mmd_gamma"],
                           "token_triplet_margin": k["token_triplet_margin"]}
    m.hash_parameters = {"triplet_alpha": k["triplet_alpha"], "quan_alpha": k["quan_alpha"], "hash_triplet_alpha": k["hash_triplet_alpha"]}
    m.triplet_margin = k["triplet_margin"]
    return m


def run(c, dtype):
    m = instance(c)
    leaves = {k: torch.tensor(c[k]).to(dtype).requires_grad_(True) for k in DC.INPUTS}
    loss, d = m.object_function(leaves["e_img"], leaves["h_img"], leaves["e_txt"], leaves["h_txt"], labels=torch.tensor(c["labels"]).to(dtype))
    loss.backward()
    vals = [d["All loss"], d["Tokens"]["Similarity"]["i2t"], d["Tokens"]["Similarity"]["t2i"], d["Tokens"]["Maximum Mean Discrepancy"],
            d["Tokens"]["Diversity"], d["Hash"]["Triplet"]["i2t"], d["Hash"]["Triplet"]["t2i"], d["Hash"]["Quantization"]["image"],
            d["Hash"]["Quantization"]["text"]]
    assert float(loss.detach()) == float(d["All loss"])
    out = {k: np.asarray(float(v), np.float64).reshape(1) for k, v in zip(DC.TERMS, vals)}
    for g, k in zip(DC.GRADS, DC.INPUTS):
        out[g] = leaves[k].grad.double().numpy().copy()
    return out


def head_records():
    out = {"state__" + k: np.array(v.shape, np.int64) for k, v in HashLayer(50, 32, 512, 16, setDim=8).state_dict().items()}
    torch.manual_seed(6401)
    layer = HashLayer(visual_tokens=5, txt_tokens=5, feature_size=64, outputDim=6, setDim=3, hash_func_="tanh").eval()
    th = layer.img_token_hash
    with torch.no_grad():
        for p in th.parameters():
            if p.dim() == 1:
                p.copy_(torch.randn(p.shape) * 0.1)          # weights_init_kaiming zeroes the biases: give them a value to check
    names = dict(zip(DC.HEAD_PARAMS, ("token_layer.weight", "token_layer.bias", "hash_layer.0.weight", "hash_layer.0.bias",
                                      "hash_layer.3.weight", "hash_layer.3.bias")))
    x, ge, gh = torch.randn(4, 5, 64), torch.randn(4, 3, 6), torch.randn(4, 6)
    out.update({"head__" + k: th.get_parameter(n).detach().numpy().copy() for k, n in names.items()})
    out.update(head__x=x.numpy(), head__g_embeds=ge.numpy(), head__g_hash=gh.numpy())
    dev = 0.0
    for tag, dtype in (("f64", torch.float64), ("f32", torch.float32)):
        th.to(dtype)
        th.zero_grad()
        leaf = x.to(dtype).requires_grad_(True)
        embeds, code = layer.encode_img(leaf)
        ((embeds * ge.to(dtype)).sum() + (code * gh.to(dtype)).sum()).backward()
        rec = {"embeds": embeds, "hash": code, "g_x": leaf.grad}
        rec.update({"g_" + k: th.get_parameter(n).grad for k, n in names.items()})
        for k, v in rec.items():
            out["head__%s_%s" % (tag, k)] = v.detach().double().numpy().copy() if tag == "f64" else v.detach().numpy().copy()
    for k in rec:
        dev = max(dev, DC.rel_err(out["head__f32_" + k], out["head__f64_" + k]))
    out["deviation__head"] = np.array(dev)
    print("head: largest float32-against-float64 deviation", dev)
    return out


def main():
    out, dev = {}, {k: 0.0 for k in DC.KINDS}
    for name, spec in DC.GOLDEN_CASES.items():
        c = DC.draw(**spec)
        assert c["B"] * c["M"] <= 576
        k = DC.consts(c)
        rec = {key: c[key] for key in DC.INPUTS}
        rec.update(labels=c["labels"].astype(np.int8), seed=np.array(c["seed"]), mode=np.array(k["mode"]), hash_func=np.array(k["hash_func"]))
        rec.update({key: np.array(float(k[key])) for key in DC.CONST_KEYS if key not in ("mode", "hash_func")})
        r64, r32 = run(c, torch.float64), run(c, torch.float32)
        for key in r64:
            rec["f64_" + key], rec["f32_" + key] = r64[key], r32[key].astype(np.float32)
            dev[DC.kind_of(key)] = max(dev[DC.kind_of(key)], DC.rel_err(r32[key], r64[key]))
        for key, v in rec.items():
            out["%s__%s" % (name, key)] = v
        print(name, "loss", float(r64["loss"][0]), "f32 - f64:", " ".join("%s %.2e" % (key, DC.rel_err(r32[key], r64[key])) for key in r64))
    for kind, v in dev.items():
        out["deviation__" + kind] = np.array(v)
    out.update(head_records())
    print("largest float32-against-float64 deviation per tensor kind:", dev)
    path = out_path("dimch.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
