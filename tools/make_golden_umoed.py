#!/usr/bin/env python3
"""Golden values of UMoED, produced by the UNMODIFIED reference (models/UMoED: HashLayer with its SoftMoEDecoder or nn.TransformerDecoder,
UMoED.object_function on an instance made without its constructor, SetwiseDistance, DIMCH's TripletLoss, torch's autograd) through
oracle._ref_import, on the CPU in float32 and in float64: python tools/make_golden_umoed.py [DIR] -> tests/golden/umoed.npz (or DIR/).
Needs the reference checkout and einops (the Soft-MoE calls it); nothing at test time runs or imports this.

SetwiseDistance's constructor moves two scalars to the GPU (``.cuda()``); this process has none, so that one call is made a no-op here,
in this process only.

Parameters and inputs are drawn from the seeds of tests/umoed_cases.py and loaded into the reference's modules by name; the file stores
only what the reference made of them -- the weights are not stored (F = 2048 makes one layer half a megabyte):
  head__<case>__{f64,f32}_{embeds,code}, head__<case>__seed   for umoed_cases.GOLDEN_HEAD_CASES (MoE, the fusion call, the plain decoder)
  state__<config>__<key>                                      shapes of HashLayer's state dict for umoed_cases.STATE_CONFIGS, in order
  loss__<case>__{f64,f32}_<term or gradient>, loss__<case>__seed   for umoed_cases.GOLDEN_LOSS_CASES
  deviation__<kind>                                           the largest float32-against-float64 deviation per tensor kind
Before writing it asserts what the tests rely on: every row's top-2 logit gap (umoed_cases.HEAD_GAP), the objective's guards, a live
triplet term where the class count allows one, and that the float64 restatement reproduces the reference to 1e-12."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import umoed_cases as UC  # noqa: E402
from oracle import _ref_import  # noqa: E402
from oracle.fixtures import out_path  # noqa: E402

_ref_import.setup()
for ns in ("UMoED", "UMoED/hash", "DIMCH", "DIMCH/loss"):      # bare: the packages' __init__ pull the registry in
    _ref_import._ns("models." + ns.replace("/", "."), os.path.join(_ref_import.REF, "models", *ns.split("/")))
torch.Tensor.cuda = lambda self, *a, **k: self                  # see the module text
from models.UMoED import UMoED as ref_umoed  # noqa: E402  (the reference's own module)
from models.UMoED.distance import SetwiseDistance  # noqa: E402
from models.UMoED.hash.hash_moe import HashLayer  # noqa: E402
from models.DIMCH.loss.triplet_loss import TripletLoss  # noqa: E402


def ref_layer(c):
    return HashLayer(visual_tokens=c.get("T_img", c["T"]), txt_tokens=c["T"] - c.get("T_img", c["T"]), img_feature_size=c["E"],
                     txt_feature_size=c["E"], outputDim=c["V"], setDim=c["M"], decoder_heads=c["heads"], decoder_layers=c["layers"],
                     num_experts=max(c["n"], 1), slots_per_expert=max(c["p"], 1), MoE=c["moe"], fusion=True, hidden_dim=c["d"],
                     hash_func_=c["hash_func"], merge_func_=UC.MERGE_OF[c["hash_func"]]).eval()


def head_records():
    out, dev = {}, {"embeds": 0.0, "code": 0.0}
    for name in UC.GOLDEN_HEAD_CASES:
        c = UC.head_case(name)
        assert c["F"] == 2048
        if c["hash_func"] == "linear_subspace":
            assert c["gap"] >= UC.HEAD_GAP, (name, c["gap"])
        layer = ref_layer(c)
        assert list(layer.hash_module.state_dict()) == list(c["P"]), name
        rec = {}
        for tag, dtype in (("f64", torch.float64), ("f32", torch.float32)):
            layer.to(dtype)
            layer.hash_module.load_state_dict({k: torch.tensor(v).to(dtype) for k, v in c["P"].items()}, strict=True)
            x = torch.tensor(c["x"]).to(dtype)
            with torch.no_grad():
                if "T_img" in c:
                    embeds, code = layer.encode_imgAndtxt(x[:, :c["T_img"]], x[:, c["T_img"]:])
                else:
                    embeds, code = layer.encode_img(x)
            rec[tag] = {"embeds": embeds.double().numpy(), "code": code.reshape(x.shape[0], -1).double().numpy()}
        mine = UC.head_reference(name)
        for k in ("embeds", "code"):
            assert UC.rel_err(mine[k], rec["f64"][k]) <= 1e-12, (name, k, UC.rel_err(mine[k], rec["f64"][k]))
            out["head__%s__f64_%s" % (name, k)] = rec["f64"][k]
            out["head__%s__f32_%s" % (name, k)] = rec["f32"][k].astype(np.float32)
        if c["hash_func"] == "linear_subspace":
            assert np.array_equal(rec["f32"]["code"], rec["f64"]["code"]), name
        else:
            dev["code"] = max(dev["code"], UC.rel_err(rec["f32"]["code"], rec["f64"]["code"]))
        dev["embeds"] = max(dev["embeds"], UC.rel_err(rec["f32"]["embeds"], rec["f64"]["embeds"]))
        out["head__%s__seed" % name] = np.array(c["seed"])
        print("head", name, "seed", c["seed"], "gap %.2e" % c["gap"], "f32 - f64 embeds %.2e" % UC.rel_err(rec["f32"]["embeds"], rec["f64"]["embeds"]))
    for cfg, kw in UC.STATE_CONFIGS.items():
        for i, (k, v) in enumerate(HashLayer(**kw).state_dict().items()):
            out["state__%s__%03d__%s" % (cfg, i, k)] = np.array(v.shape, np.int64)
    for k, v in dev.items():
        out["deviation__" + k] = np.array(v)
    return out


def ref_objective(c, dtype):
    k = UC.consts(c)
    m = ref_umoed.UMoED.__new__(ref_umoed.UMoED)
    torch.nn.Module.__init__(m)
    m.triplet_loss = TripletLoss(reduction="mean")
    m.distance = SetwiseDistance(img_set_size=c["M"], txt_set_size=c["M"], mode="pairwise")
    m.chamfer_parmeters = {"set_size": c["M"], "unif_alpha": k["unif_alpha"], "token_triplet_margin": k["token_triplet_margin"]}
    m.hash_parameters = {"triplet_alpha": k["triplet_alpha"], "quan_alpha": 0.001}
    m.extreme, m.extreme_T, m.distance_mode = k["extreme"], k["extreme_T"], "cosine"
    leaves = {n: torch.tensor(c[n]).to(dtype).requires_grad_(True) for n in UC.INPUTS}
    loss, d = m.object_function(img_embeds=leaves["e_img"], img_hash=None, txt_embeds=leaves["e_txt"], txt_hash=None, fusion_embeds=None,
                                fusion_hash=None, labels=torch.tensor(c["labels"]).to(dtype))
    loss.backward()
    sim, div = d["Tokens"]["Similarity"], d["Tokens"]["Diversity"]
    assert sim["it2i"] == 0 and sim["it2t"] == 0 and div["it"] == 0
    vals = [d["All loss"], sim["i2t"], sim["t2i"], div["i"], div["t"]]
    out = {n: np.asarray(float(v), np.float64).reshape(1) for n, v in zip(UC.TERMS, vals)}
    for g, n in zip(UC.GRADS, UC.INPUTS):
        out[g] = leaves[n].grad.double().numpy().copy()
    return out


def loss_records():
    out, dev = {}, {k: 0.0 for k in UC.KINDS}
    for name, spec in UC.GOLDEN_LOSS_CASES.items():
        c = UC.draw_loss(**spec)
        assert UC.guarded(UC.guards(c)), name
        r64, r32 = ref_objective(c, torch.float64), ref_objective(c, torch.float32)
        if c["C"] > 1:
            assert r64["T_i2t"][0] > 0 and r64["T_t2i"][0] > 0, name
        mine = UC.objective(c, torch.float64, up=1.0)
        for key in r64:
            e = UC.rel_err(mine[key], r64[key])
            assert e <= 1e-12, (name, key, e)
            out["loss__%s__f64_%s" % (name, key)], out["loss__%s__f32_%s" % (name, key)] = r64[key], r32[key].astype(np.float32)
            dev[UC.kind_of(key)] = max(dev[UC.kind_of(key)], UC.rel_err(r32[key], r64[key]))
        out["loss__%s__seed" % name] = np.array(c["seed"])
        print("loss", name, "seed", c["seed"], float(r64["loss"][0]), " ".join("%s %.2e" % (key, UC.rel_err(r32[key], r64[key])) for key in r64))
    for k, v in dev.items():
        out["deviation__" + k] = np.array(v)
    return out


def main():
    out = head_records()
    out.update(loss_records())
    for name in UC.LOSS_CASES:                                   # the GPU pool's cases: guarded, and live where a class count allows it
        c = UC.loss_case(name)
        assert UC.guarded(UC.guards(c)), name
        if c["C"] > 1:
            assert UC.loss_reference(name)["T_i2t"][0] > 0, name
    print("largest float32-against-float64 deviation per tensor kind:", {k[11:]: float(v) for k, v in out.items() if k.startswith("deviation__")})
    path = out_path("umoed.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
