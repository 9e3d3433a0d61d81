#!/usr/bin/env python3
"""Golden values of TwDH's training objective, produced by the UNMODIFIED reference (models/TwDH/TwDH.py: hash_center_multilables,
hash_convert and TwDH.compute_loss on an instance made without its constructor, plus torch's autograd) through oracle._ref_import, on
the CPU in float32: python tools/make_golden_twdh_loss.py [DIR] -> tests/golden/twdh_loss.npz (or DIR/).  Needs the reference
checkout; nothing at test time runs or imports this.

Two cases (tests/twdh_cases.py:GOLDEN_CASES).  `small`: C = 12 classes, long 32, shorts 4 and 8, B = 9, seeded +-1 centres; row 0
has no label (the reference's NaN mean), row 1 every label, rows 2 and 3 two labels each (zero sums), and the probabilities
[0, 1, 1e-30, .3]-style saturated entries in row 4; every other probability comes from unit-scale logits.  `coco16`: the first 16 classes of the centres the reference ships for coco
(long 512, shorts 16 / 32 / 64), stored as int8, B = 6.  Per case: the inputs, the seed and the tie vectors the reference drew
(replayed from the seed by its own torch.randint_like calls, in its order), the targets it built, every scalar of loss_dict in
xmh_twdh_loss's layout, and the four input gradients (the short ones side by side)."""
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "clip-based-cross-modal-hash_amd"))
import twdh_cases as TC  # noqa: E402
from oracle import _ref_import  # noqa: E402
from oracle.fixtures import out_path  # noqa: E402

_ref_import.setup()
_ref_import._ns("models.TwDH", os.path.join(_ref_import.REF, "models", "TwDH"))
sys.modules.pop("models.DCMHT.hash", None)      # the bare namespace: TwDH imports HashLayer from the package itself
from models.TwDH.TwDH import TwDH, hash_center_multilables, hash_convert  # noqa: E402  (the reference's own)

COCO = os.path.join(_ref_import.REF, "data", "transformer", "TwDH", "coco")


def inputs(name):
    rng = np.random.default_rng({"small": 5101, "coco16": 5102}[name])
    if name == "small":
        B, C, lens = 9, 12, (32, 4, 8)
        centres = [(rng.integers(0, 2, (C, k)) * 2 - 1).astype(np.int8) for k in lens]
    else:
        B, C, lens = 6, 16, (512, 16, 32, 64)
        centres = [torch.load(os.path.join(COCO, "long", "512.pkl")).numpy()[:C].astype(np.int8)] + \
                  [torch.load(os.path.join(COCO, "short", "%d.pkl" % k)).numpy()[:C].astype(np.int8) for k in lens[1:]]
        assert all(np.isin(c, (-1, 1)).all() for c in centres)
    labels = (rng.random((B, C)) < 0.15).astype(np.int64)
    labels[np.arange(B), rng.integers(0, C, B)] = 1
    labels[1] = 1
    for r in (2, 3):
        labels[r] = 0
        labels[r, rng.choice(C, 2, replace=False)] = 1
    if name == "small":
        labels[0] = 0
    S = sum(lens[1:])
    # logits of unit scale, as in tests/twdh_cases.py:build: the quantisation part is then a visible share of every ordinary entry
    P = {k: TC._probs(rng, B, n, scale=1.0) for k, n in (("img_long", lens[0]), ("img_short", S), ("txt_long", lens[0]), ("txt_short", S))}
    for k in P:                                     # saturated and nearly saturated entries, valid probabilities all the same
        P[k][4, :8] = (0.0, 1.0, 1.0, 0.0, 1e-30, 1.0, 0.3, 0.7)
    return dict(B=B, C=C, lens=lens, centres=centres, labels=labels, quan_alpha=0.5, low_rate=0.3, seed=1814 + len(name), **P)


def run(name):
    c = inputs(name)
    lens, keys = c["lens"], [str(k) for k in c["lens"][1:]]
    m = TwDH.__new__(TwDH)
    torch.nn.Module.__init__(m)
    m.long_center = torch.tensor(c["centres"][0]).float()
    m.short_center = {k: torch.tensor(cen).float() for k, cen in zip(keys, c["centres"][1:])}
    m.quan_alpha, m.low_rate, m.criterion = c["quan_alpha"], c["low_rate"], torch.nn.BCELoss()
    labels = torch.tensor(c["labels"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.manual_seed(c["seed"])                # the tie vectors, by the reference's own call in its order
        ties = [torch.randint_like(cen[0], 2) * 2 - 1 for cen in [m.long_center] + list(m.short_center.values())]
        torch.manual_seed(c["seed"])                # the targets the reference builds from the same draws
        tg = [hash_convert(hash_center_multilables(labels, cen)) for cen in [m.long_center] + list(m.short_center.values())]
        bits = np.concatenate([t.reshape(t.shape[0], -1, 2)[:, :, 1].numpy() for t in tg], 1).astype(np.uint8)
        leaves = {k: torch.tensor(c[k]).requires_grad_(True) for k in ("img_long", "img_short", "txt_long", "txt_short")}
        split = lambda t: {k: v for k, v in zip(keys, TC._split(lens, None, t)[1:])}      # noqa: E731
        torch.manual_seed(c["seed"])
        loss, d = m.compute_loss(leaves["img_long"], leaves["txt_long"], split(leaves["img_short"]), split(leaves["txt_short"]), labels, None)
        loss.backward()
    n = len(lens)
    terms = np.full(1 + 6 * n, np.nan, np.float64)     # the per-modality short terms are not in loss_dict: NaN = not recorded
    terms[0] = float(d["All loss"])
    terms[1], terms[2] = float(d["Long"]["NCE"]["image"]), float(d["Long"]["Quan"]["image"])
    terms[1 + 2 * n], terms[2 + 2 * n] = float(d["Long"]["NCE"]["text"]), float(d["Long"]["Quan"]["text"])
    for i, k in enumerate(keys):
        terms[1 + 4 * n + 2 * (i + 1)], terms[2 + 4 * n + 2 * (i + 1)] = float(d["Short"][k]["NCE"].detach()), float(d["Short"][k]["Quan"].detach())
    rec = {"lens": np.array(lens), "labels": c["labels"].astype(np.int8), "seed": np.array(c["seed"]), "quan_alpha": np.array(c["quan_alpha"]),
           "low_rate": np.array(c["low_rate"]), "bits": bits, "terms": terms, "loss_f32": loss.detach().numpy()}
    for i, (cen, tie) in enumerate(zip(c["centres"], ties)):
        rec["centre_%d" % i], rec["tie_%d" % i] = cen, tie.numpy().astype(np.int8)
    for k, t in leaves.items():
        rec[k], rec["d_" + k] = c[k], t.grad.numpy()
    return rec


def main():
    out = {}
    for name in TC.GOLDEN_CASES:
        for k, v in run(name).items():
            out["%s__%s" % (name, k)] = v
    path = out_path("twdh_loss.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
