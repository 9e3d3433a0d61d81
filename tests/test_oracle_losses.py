"""CPU: the oracle's restatement of the DCMHT loss, and of its gradient with respect to the codes, against goldens produced by
the reference's own our_loss and loss.backward() (oracle/make_golden_loss.py)."""
import numpy as np
import torch

from oracle import losses as OL
from oracle.fixtures import grads_close
from oracle.losses import DCMHT_CASES as CASES, DCMHT_TERMS as ORDER, load_dcmht as load, load_dcmht_grads as load_grads


def test_oracle_loss_matches_the_reference():
    for name in CASES:
        img, txt, labels, K, sim, vartheta, threshold, alpha, ref = load(name)
        if labels is None:
            labels = torch.eye(img.shape[0])                   # reference object_function :152-154
        got = OL.our_loss(img, txt, labels, K, vartheta, threshold, alpha, sim)
        vec = np.array([float(got[k]) for k in ORDER])
        # fp32 reference (and its cdist may take the matmul route) against a float64 restatement
        assert np.allclose(vec, ref, rtol=2e-5, atol=1e-6), (name, vec, ref)


def test_oracle_gradient_matches_the_reference_backward():
    for name in CASES:
        img, txt, labels, K, sim, vartheta, threshold, alpha, _ = load(name)
        if labels is None:
            labels = torch.eye(img.shape[0])
        gi, gt = OL.our_loss_grad(img, txt, labels, K, vartheta=vartheta, threshold=threshold, quan_alpha=alpha, similarity_function=sim)
        ri, rt = load_grads(name)
        assert grads_close(gi.numpy(), ri) and grads_close(gt.numpy(), rt), (name, np.abs(gi.numpy() - ri).max(), np.abs(ri).max())
