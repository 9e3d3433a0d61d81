#!/usr/bin/env python3
"""Golden vectors of DSPH's HyP loss and of its gradients (loss.backward() with respect to the image codes, the text codes and the
proxies), produced by the UNMODIFIED reference (models/DSPH/DSPH.py + models/DSPH/loss/HyP.py) through oracle._ref_import:
python tools/make_golden_hyp.py -> tests/golden/loss_dsph.npz.  Needs the reference checkout; nothing at test time runs this.

The HyP module is built by the reference's own DSPH.__init__ (backbone replaced by a stub), so its threshold is the codetable cell
the reference looks up for (K, numclass): K 16 / C 80 -> 0.25, K 128 / C 80 -> 0.0."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from oracle import _ref_import  # noqa: E402

_ref_import.setup()
from models.DSPH.DSPH import DSPH  # noqa: E402  (the reference class)

# this package's codetable reader, loaded on its own (no libxmh.so needed): it must find the cell the reference's lookup finds
_spec = importlib.util.spec_from_file_location("xmh_codetable", os.path.join(ROOT, "clip-based-cross-modal-hash_amd", "xmh", "models",
                                                                              "codetable.py"))
codetable = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(codetable)
CODETABLE = os.path.join(_ref_import.REF, "models", "DSPH", "loss", "codetable.xlsx")


class _NoBackbone(DSPH):
    def load_backbone(self, clipPath, return_patches=False):
        return 8, torch.nn.Identity()


def ref_model(K, C, alpha, hypseed=0):
    m = _NoBackbone(cfg=None, outputDim=K, numclass=C, hypseed=hypseed, alpha=alpha)
    assert m.hyp.threshold == codetable.hyp_threshold(CODETABLE, K, C), (K, C, m.hyp.threshold)
    return m


def labels_random(g, B, C, p=0.05):
    L = (torch.rand(B, C, generator=g) < p).float()
    L[torch.arange(B), torch.randint(0, C, (B,), generator=g)] = 1.0
    return L


def labels_single(g, B, C):
    L = torch.zeros(B, C)
    L[torch.arange(B), torch.randint(0, C, (B,), generator=g)] = 1.0
    return L


def labels_shared(g, B, C):
    """multi-label rows all carry class 0: no pair of them is disjoint (Z = 0, M > 0)"""
    L = labels_random(g, B, C, 0.08)
    multi = L.sum(1) > 1
    L[multi, 0] = 1.0
    return L


# name, B, K, C, alpha, labels, zero code row
CASES = [("b100_k16_c80", 100, 16, 80, 0.8, labels_random, False),
         ("b64_k128_c80", 64, 128, 80, 0.8, labels_random, False),
         ("b64_k16_c80_alpha0", 64, 16, 80, 0.0, labels_random, False),
         ("b48_k16_c80_single", 48, 16, 80, 0.8, labels_single, False),
         ("b48_k16_c80_shared", 48, 16, 80, 0.8, labels_shared, False),
         ("b40_k16_c80_zero_row", 40, 16, 80, 0.8, labels_random, True),
         ("b24_k16_c24_nolabels", 24, 16, 24, 0.8, None, False)]


def main():
    out = {}
    for name, B, K, C, alpha, make_labels, zero_row in CASES:
        g = torch.Generator().manual_seed(1814 + B + K + C)
        x = torch.tanh(torch.randn(B, K, generator=g) * 1.5)                   # what the DSPH head emits
        y = torch.tanh(torch.randn(B, K, generator=g) * 1.5)
        if zero_row:
            x[3] = 0.0
        labels = None if make_labels is None else make_labels(g, B, C)
        m = ref_model(K, C, alpha)
        proxies = m.hyp.proxies.detach().clone()
        x.requires_grad_(True)
        y.requires_grad_(True)
        loss, _ = m.object_function(x, y, labels=labels)
        loss.backward()                                                        # runners/DSPH/runner.py:123
        out[name + "_x"], out[name + "_y"], out[name + "_proxies"] = x.detach().numpy(), y.detach().numpy(), proxies.numpy()
        if labels is not None:
            out[name + "_labels"] = labels.numpy().astype(np.uint8)
        out[name + "_meta"] = np.array([K, C, alpha, m.hyp.threshold], dtype=np.float64)
        out[name + "_loss"] = np.array(float(loss.detach()), dtype=np.float64)
        out[name + "_gx"], out[name + "_gy"] = x.grad.numpy().copy(), y.grad.numpy().copy()
        out[name + "_gproxies"] = m.hyp.proxies.grad.numpy().copy()
        print(name, "threshold", m.hyp.threshold, "loss", float(loss))
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "loss_dsph.npz"), **out)


if __name__ == "__main__":
    main()
