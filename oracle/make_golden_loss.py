#!/usr/bin/env python3
"""Golden vectors of the DCMHT loss and of its gradient with respect to the codes (loss.backward()), produced by the
UNMODIFIED reference (models/DCMHT/DCMHT.py our_loss) in this container: python oracle/make_golden_loss.py [DIR] -> tests/golden/loss_dcmht.npz (or DIR/).  Build-container only (/root/reference)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import _ref_models  # noqa: E402
from oracle.fixtures import labels_random, out_path  # noqa: E402

out = {}
cases = [("b40_k16_euclid", 40, 16, 24, "euclidean", True), ("b40_k64_cos", 40, 64, 24, "cosine", True),
         ("b96_k64_euclid", 96, 64, 80, "euclidean", True), ("b17_k32_euclid_nolabels", 17, 32, 0, "euclidean", False)]
for name, B, K, C, sim, has_labels in cases:
    g = torch.Generator().manual_seed(1814 + B + K)
    img = torch.softmax(torch.randn(B, K, 2, generator=g) * 2.0, dim=-1).reshape(B, 2 * K)     # what the softmax hash emits
    txt = torch.softmax(torch.randn(B, K, 2, generator=g) * 2.0, dim=-1).reshape(B, 2 * K)
    labels = None
    if has_labels:
        labels = labels_random(g, B, C, 0.1)
    m = _ref_models.dcmht(K, sim)
    img.requires_grad_(True)
    txt.requires_grad_(True)
    loss, d = m.object_function(img, txt, labels=labels)
    loss.backward()                                 # runners/DCMHT/runner.py:124
    out[name + "_gimg"], out[name + "_gtxt"] = img.grad.numpy().copy(), txt.grad.numpy().copy()
    img, txt = img.detach(), txt.detach()
    out[name + "_img"], out[name + "_txt"] = img.numpy(), txt.numpy()
    if has_labels:
        out[name + "_labels"] = labels.numpy()
    out[name + "_meta"] = np.array([K, 1.0 if sim == "cosine" else 0.0, 0.75, 0.1, 0.001])
    out[name + "_ref"] = np.array([float(loss), float(d["Intra"]["Positive"]), float(d["Intra"]["Negative"]), float(d["Inter"]["Positive"]["i2t"]),
                                   float(d["Inter"]["Negative"]["i2t"]), float(d["Inter"]["Positive"]["t2i"]), float(d["Inter"]["Negative"]["t2i"]),
                                   float(d["Quan"]["Image"]), float(d["Quan"]["Text"])], dtype=np.float64)
    print(name, out[name + "_ref"])
np.savez_compressed(out_path("loss_dcmht.npz"), **out)
