#!/usr/bin/env python3
"""Golden values of DNPH's training objective and head, produced by the UNMODIFIED reference (models/DNPH: Loss, gene_noise,
rand_unit_rect, HashLayer and DNPH.compute_loss on an instance made without its constructor, plus torch's autograd) through
oracle._ref_import, on the CPU in float32: python tools/make_golden_dnph.py [DIR] -> tests/golden/dnph.npz (or DIR/).  Needs the
reference checkout and scipy (the reference's gene_noise calls it); nothing at test time runs or imports this.

Two cases (tests/dnph_cases.py:GOLDEN_CASES: B = 7, K = 16, C = 5 and B = 37, K = 48, C = 33, the class logits 80 wide as the
reference builds them).  Per case: the inputs; Loss.forward's value and loss.backward()'s gradients of the four inputs and of the
proxies; the +-1 vectors the reference's rand_unit_rect drew (replayed from the seed by its own call), gene_noise's output for both
modalities' codes; DNPH.compute_loss's value and its two noise means with those draws (noise_alpha 0.1).  Once: the key names and
shapes of HashLayer(512, 16).state_dict()."""
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dnph_cases as DC  # noqa: E402
from oracle import _ref_import  # noqa: E402
from oracle.fixtures import out_path  # noqa: E402

_ref_import.setup()
_ref_import._ns("models.DNPH", os.path.join(_ref_import.REF, "models", "DNPH"))      # bare: the package's __init__ pulls the registry in
from models.DNPH import DNPH as ref_dnph  # noqa: E402  (the reference's own module; its sub-packages import for real)
from models.DNPH.hash.hash import HashLayer  # noqa: E402
from models.DNPH.loss.b_reg import gene_noise, rand_unit_rect  # noqa: E402
from models.DNPH.loss.loss import Loss  # noqa: E402

NOISE_ALPHA = 0.1


def run(name):
    c = DC.draw(**DC.GOLDEN_CASES[name])
    B, K, C = c["B"], c["K"], c["C"]
    loss_mod = Loss(num_classes=C, output_dim=K, mrg=1.0)
    with torch.no_grad():
        loss_mod.proxies.copy_(torch.tensor(c["P"]))
    labels = torch.tensor(c["labels"])
    leaves = {k: torch.tensor(c[k]).requires_grad_(True) for k in ("f_img", "f_txt", "p_img", "p_txt")}
    loss1 = loss_mod(leaves["f_img"], leaves["f_txt"], leaves["p_img"], leaves["p_txt"], labels, labels)
    loss1.backward()
    rec = {k: c[k] for k in ("f_img", "f_txt", "p_img", "p_txt", "P")}
    rec.update(labels=c["labels"].astype(np.int8), mrg=np.array(1.0), noise_alpha=np.array(NOISE_ALPHA), seed=np.array(c["seed"]),
               loss1=loss1.detach().numpy(), g_P=loss_mod.proxies.grad.numpy().copy())
    for k, t in leaves.items():
        rec["g_" + k] = t.grad.numpy().copy()
    # the draws of compute_loss, by the reference's own call from numpy's global generator
    np.random.seed(c["seed"])
    s_vector = rand_unit_rect(B, K)
    rec["s_vector"] = s_vector.astype(np.int8)
    rec["noise_img"] = gene_noise(c["f_img"], s_vector)
    rec["noise_txt"] = gene_noise(c["f_txt"], s_vector)
    m = ref_dnph.DNPH.__new__(ref_dnph.DNPH)
    torch.nn.Module.__init__(m)
    m.loss, m.noise_alpha = loss_mod, NOISE_ALPHA
    np.random.seed(c["seed"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        loss, d = m.compute_loss(torch.tensor(c["f_img"]), torch.tensor(c["f_txt"]), torch.tensor(c["p_img"]), torch.tensor(c["p_txt"]), labels, None)
    rec.update(loss=loss.detach().numpy(), noise_mean_img=d["Noise"]["image"].detach().numpy(), noise_mean_txt=d["Noise"]["text"].detach().numpy())
    assert float(d["All loss"]) == float(loss.detach())
    return rec


def main():
    out = {}
    for name in DC.GOLDEN_CASES:
        for k, v in run(name).items():
            out["%s__%s" % (name, k)] = v
    sd = HashLayer(inputDim=512, outputDim=16).state_dict()
    out["head_state_keys"] = np.array(list(sd))
    out["head_state_shapes"] = np.array([",".join(str(n) for n in v.shape) for v in sd.values()])
    path = out_path("dnph.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
