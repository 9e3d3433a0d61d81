#!/usr/bin/env python3
"""Golden vectors of DSPH's HyP loss and of its gradients (loss.backward() with respect to the image codes, the text codes and the
proxies), produced by the UNMODIFIED reference (models/DSPH/DSPH.py + models/DSPH/loss/HyP.py) through oracle._ref_import:
python oracle/make_golden_hyp.py [DIR] -> tests/golden/loss_dsph.npz (or DIR/).  Needs the reference checkout; nothing at test time runs this.

The HyP module is built by the reference's own DSPH.__init__ (oracle/_ref_models.py: backbone replaced by a stub), so its threshold is the codetable cell
the reference looks up for (K, numclass): K 16 / C 80 -> 0.25, K 128 / C 80 -> 0.0."""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import _ref_import, _ref_models  # noqa: E402
from oracle.fixtures import labels_random, labels_shared, labels_single, out_path  # noqa: E402
from oracle.losses import HYP_CASES  # noqa: E402

# this package's codetable reader, loaded on its own (no libxmh.so needed): it must find the cell the reference's lookup finds
_spec = importlib.util.spec_from_file_location("xmh_codetable", os.path.join(ROOT, "clip-based-cross-modal-hash_amd", "xmh", "models",
                                                                              "codetable.py"))
codetable = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(codetable)
CODETABLE = os.path.join(_ref_import.REF, "models", "DSPH", "loss", "codetable.xlsx")


def ref_model(K, C, alpha):
    m = _ref_models.dsph(K, C, alpha)
    assert m.hyp.threshold == codetable.hyp_threshold(CODETABLE, K, C), (K, C, m.hyp.threshold)
    return m


# name, B, K, C, alpha, labels, zero code row
CASES = [("b100_k16_c80", 100, 16, 80, 0.8, labels_random, False),
         ("b64_k128_c80", 64, 128, 80, 0.8, labels_random, False),
         ("b64_k16_c80_alpha0", 64, 16, 80, 0.0, labels_random, False),
         ("b48_k16_c80_single", 48, 16, 80, 0.8, labels_single, False),
         ("b48_k16_c80_shared", 48, 16, 80, 0.8, labels_shared, False),
         ("b40_k16_c80_zero_row", 40, 16, 80, 0.8, labels_random, True),
         ("b24_k16_c24_nolabels", 24, 16, 24, 0.8, None, False)]


def main():
    assert [c[0] for c in CASES] == HYP_CASES
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
    np.savez_compressed(out_path("loss_dsph.npz"), **out)


if __name__ == "__main__":
    main()
