"""The DCMHT loss suite without a GPU: the dtype-preserving restatement of tests/dcmht_loss_cases.py (which the GPU tests lean on)
equals oracle.losses in float64 and reproduces the reference's own numbers of tests/golden/loss_dcmht.npz; every case of the GPU module
meets the conditions on its inputs; the NaN patterns of the non-finite cases are what the GPU test expects."""
import numpy as np
import pytest
import torch

import dcmht_loss_cases as DC
from oracle import losses as OL
from oracle.fixtures import grads_close


@pytest.mark.parametrize("name", OL.DCMHT_CASES)
def test_float64_restatement_equals_the_oracle_and_reproduces_the_goldens(name):
    img, txt, labels, K, sim, vartheta, threshold, alpha, ref = OL.load_dcmht(name)
    own = DC.restate(img, txt, labels, K, sim, vartheta=vartheta, threshold=threshold, alpha=alpha)
    L = torch.eye(img.shape[0]) if labels is None else labels
    want = OL.our_loss(img, txt, L, K, vartheta, threshold, alpha, sim)
    gi, gt = OL.our_loss_grad(img, txt, L, K, vartheta=vartheta, threshold=threshold, quan_alpha=alpha, similarity_function=sim)
    # the same float64 ops; only the thread count of the reductions may differ
    assert DC.rel_err(own["terms"], np.array([float(want[k]) for k in DC.TERMS])) <= 1e-14
    assert DC.rel_err(own["g_img"], gi.numpy()) <= 1e-14 and DC.rel_err(own["g_txt"], gt.numpy()) <= 1e-14
    # the bounds of tests/test_oracle_losses.py against the reference's fp32 run
    assert np.allclose(own["terms"], ref, rtol=2e-5, atol=1e-6), (name, own["terms"], ref)
    ri, rt = OL.load_dcmht_grads(name)
    assert grads_close(own["g_img"], ri) and grads_close(own["g_txt"], rt), name


def test_float32_restatement_keeps_its_dtype_and_the_pool_is_an_fp32_error():
    img, txt, labels, K, sim, vartheta, threshold, alpha, _ = OL.load_dcmht(OL.DCMHT_CASES[0])
    t = DC.terms(img.float(), txt.float(), labels, K, sim, vartheta, threshold, alpha)
    assert all(v.dtype == torch.float32 for v in t)
    t = DC.terms(img.double(), txt.double(), labels, K, sim, vartheta, threshold, alpha)
    assert all(v.dtype == torch.float64 for v in t)
    pool = DC.golden_pool()
    print("golden pool", " ".join("%s %.2e" % kv for kv in pool.items()))
    for kind in DC.KINDS:                             # a few fp32 roundings: neither exact nor loose
        assert 2.0 ** -27 < pool[kind] < 2.0 ** -20, (kind, pool[kind])


def test_the_table_of_the_gpu_module_is_what_the_cases_hold():
    got = sorted((c["B"], c["K"], c["C"], c["sim"]) for c in DC.CASES.values() if c["C"] is not None)
    assert got == sorted([(257, 16, 21, "euclidean"), (300, 64, 33, "euclidean"), (257, 16, 21, "cosine"), (64, 64, 65, "cosine"),
                          (1, 16, 3, "euclidean"), (5, 1, 1, "euclidean"), (33, 128, 64, "euclidean")])
    assert [(c["B"], c["K"], c["sim"]) for c in DC.CASES.values() if c["C"] is None] == [(300, 16, "euclidean")]
    assert {c["C"] for c in DC.CASES.values()} >= {1, 33, 64, 65}
    assert max(c["B"] for c in DC.CASES.values()) > 256               # the second trip of the j loops, coef[] longer than the block


@pytest.mark.parametrize("name", list(DC.CASES))
def test_every_case_meets_the_conditions_on_its_inputs(name):
    c = DC.build(name)
    image, text = DC.codes(c)
    assert image.dtype == torch.float32 and image.shape == text.shape == (c["B"], 2 * c["K"])
    m = DC.check_conditions(name, image, text)
    print(name, DC.describe(m))
    again = DC.codes(DC.build(name))
    assert torch.equal(again[0], image) and torch.equal(again[1], text)                   # seeded: the same case at every call
    if c["inputs"] == "soft" and c["B"] > 1:          # what the older tests draw: the hinge is active for every pair
        assert all(v["beyond"] == 0 for v in m.values())
    if c["sim"] == "cosine":                          # the three regions of the clamp are all populated in every pair term
        assert all(v["below"] > 0.5 and v["above"] > 0 for v in m.values()), m
    if c.get("zero_label") is not None:               # the diagonal pair of that row is a negative pair at distance 0
        assert OL.label_sim(c["labels"])[c["zero_label"], c["zero_label"]] == 0


@pytest.mark.parametrize("name", list(DC.NONFINITE))
def test_nan_patterns_of_the_reference_expression(name):
    image, text, labels, K, sim, nan_terms = DC.build_nonfinite(name)
    assert image.shape == (6, 8) and torch.isfinite(text).all()
    assert int((~torch.isfinite(image)).sum()) == (0 if name == "zero_row_cos" else 1)
    for dtype in (torch.float64, torch.float32):
        r = DC.restate(image, text, labels, K, sim, dtype=dtype)
        assert {t for t, v in zip(DC.TERMS, r["terms"]) if np.isnan(v)} == set(nan_terms), (name, dtype, r["terms"])
        assert not np.isinf(r["terms"]).any()
        assert np.isnan(r["g_img"]).all() and np.isnan(r["g_txt"]).all(), (name, dtype)    # every entry of both gradients
    # the same batch without the poke is finite throughout: the NaNs above come from the poke alone
    clean = image.clone()
    clean[2] = text[2]
    clean[1, 3] = 0.5
    r = DC.restate(clean, text, labels, K, sim)
    assert np.isfinite(r["terms"]).all() and np.isfinite(r["g_img"]).all() and np.isfinite(r["g_txt"]).all()
