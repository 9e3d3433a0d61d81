"""The float64 HyP loss suite without a GPU: the restatement wrapper of tests/hyp_loss_cases.py (which the GPU tests lean on) reproduces
the reference's own numbers of tests/golden/loss_dsph.npz; every case of the GPU module meets the conditions on its inputs; the NaN
patterns recorded for the non-finite cases are what the reference's expression gives; building a case is deterministic."""
import numpy as np
import pytest
import torch

import hyp_loss_cases as HC
from oracle import losses as OL
from oracle.fixtures import grads_close_rows


@pytest.mark.parametrize("name", OL.HYP_CASES)
def test_restatement_wrapper_reproduces_the_goldens(name):
    x, y, P, labels, threshold, alpha, loss, grads = OL.load_hyp(name)
    labels = np.eye(x.shape[0]) if labels is None else labels
    own = HC.restate(x, y, P, labels, threshold, alpha)
    want = OL.hyp_oracle(x, y, P, labels, threshold, alpha)
    # the same float64 ops; only the thread count of the reductions may differ
    assert HC.rel_err(own["terms"], want[0]) <= 1e-14
    assert all(HC.rel_err(own[k], w) <= 1e-14 for k, w in zip(HC.KINDS[1:], want[1:]))
    # the bounds of tests/test_hyp_loss_cpu.py against the reference's fp32 run
    assert np.allclose(own["terms"][0], loss, rtol=2e-5, atol=1e-6), (name, own["terms"][0], loss)
    for k, ref in zip(HC.KINDS[1:], grads):
        assert grads_close_rows(own[k], ref), (name, k)


def test_float32_restatement_keeps_its_dtype_and_the_pool_is_an_fp32_error():
    x, y, P, labels, threshold, alpha, _, _ = OL.load_hyp(OL.HYP_CASES[0])
    for dtype in (torch.float32, torch.float64):
        t = OL.hyp_terms(torch.tensor(x).to(dtype), torch.tensor(y).to(dtype), torch.tensor(P).to(dtype), torch.tensor(labels), threshold, alpha)
        assert all(v.dtype == dtype for v in t.values())
    pool = HC.golden_pool()
    print("golden pool", " ".join("%s %.2e" % kv for kv in pool.items()))
    for kind in HC.KINDS:                             # a few fp32 roundings: neither exact nor loose
        assert 2.0 ** -27 < pool[kind] < 2.0 ** -20, (kind, pool[kind])


@pytest.mark.parametrize("name", list(HC.CASES))
def test_every_case_meets_the_conditions_on_its_inputs(name):
    c = HC.build(name)
    m = HC.check_conditions(name)
    print(name, "redrawn %d" % c["redrawn"], HC.describe(m))
    assert c["redrawn"] <= 40                         # the recipe leaves a handful of entries near the threshold, not a systematic cluster
    assert (c["floor"] is not None) == (c["K"] == 1)


@pytest.mark.parametrize("name", list(HC.CASES))
def test_building_a_case_is_deterministic(name):
    first = {k: HC.build(name)[k].clone() for k in ("x", "y", "P", "labels")}
    HC._built.pop(name)
    again = HC.build(name)
    assert all(torch.equal(first[k], again[k]) for k in first)


def test_k1_gradients_vanish_and_the_scale_bounds_their_parts():
    """at K = 1 the float64 gradients are rounding residue, far below the scale the errors are divided by (see HC.cancel_scale)"""
    for name in ("b40_k1_c3", "b40_k1_c4"):
        c = HC.build(name)
        ref = HC.restate(c["x"], c["y"], c["P"], c["labels"], c["thr"], HC.ALPHA)
        for k in HC.KINDS[1:]:
            assert c["floor"][k].shape == (ref[k].shape[0],) and (c["floor"][k] > 0).all(), (name, k)
            assert (np.abs(ref[k]).max(axis=1) <= 2.0 ** -40 * c["floor"][k]).all(), (name, k)


@pytest.mark.parametrize("name", list(HC.NONFINITE))
def test_nan_patterns_of_the_reference_expression(name):
    x, y, P, labels, thr, alpha = HC.build_nonfinite(name)
    spec = HC.NONFINITE[name]
    assert x.shape == y.shape == (6, 4) and P.shape == (7, 4) and labels.shape == (6, 7)
    assert [tuple(torch.nonzero(r).flatten().tolist()) for r in labels] == list(HC.NONFINITE_LABELS)
    M, pairs = HC.pairs_of(labels)
    assert torch.nonzero(M).flatten().tolist() == [0, 1, 3] and int(pairs.sum()) == 6 and not labels[:, 5].any()
    bad = [int((~torch.isfinite(t)).sum()) for t in (x, y, P)]
    assert bad == {"nan_unused_proxy": [0, 0, 1], "nan_code_in_M": [1, 0, 0], "inf_code_in_M": [4, 0, 0], "inf_used_proxy": [0, 0, 1],
                   "inf_both_codes": [4, 4, 0]}[name]
    if name == "inf_used_proxy":
        assert labels[:, 2].any()
    want = (spec["nan_terms"], {k: spec[k] for k in HC.KINDS[1:]})
    for dtype in (torch.float32, torch.float64):
        assert HC.nan_pattern(HC.restate(x, y, P, labels, thr, alpha, dtype=dtype)) == want, (name, dtype)
    # the finite mask entries keep the gap, so the finite rows can be held to the bound of the finite cases
    for k, (v, valid) in HC.families(x, y, P, labels).items():
        keep = valid & torch.isfinite(v)
        assert not keep.any() or float((v - thr).abs()[keep].min()) >= HC.GAP, (name, k)
    # the same batch without the poke is finite throughout: the NaNs above come from the poke alone
    clean = [torch.where(torch.isfinite(t), t, torch.full_like(t, 0.5)) for t in (x, y, P)]
    r = HC.restate(*clean, labels, thr, alpha)
    assert all(np.isfinite(r[k]).all() for k in HC.KINDS)
