"""The float64 MITH loss suite without a GPU: the restatement wrapper of tests/mith_loss_cases.py (which the GPU tests lean on)
reproduces the reference's own numbers of tests/golden/loss_mith.npz; the golden pool is computed and printed; the copy of the
kernel's likelihood grid gives the hand-computed triples; every case of the GPU module builds and meets the conditions on its inputs,
the redraw cap included; the NaN patterns recorded for the non-finite cases are what the reference's expression gives in float64 and
in float32; and the comparison the GPU tests apply has teeth: a float32 restatement that leaves out the last buffer row, and one whose
clamp mask is the open interval, each fail it.

The case at the N limit (N = 2^22) is not marked slow: building it and its float64 and float32 backward take a few seconds together."""
import numpy as np
import pytest
import torch

import mith_loss_cases as MC
from oracle import losses as OL
from oracle.fixtures import grads_close


@pytest.mark.parametrize("name", OL.MITH_CASES)
def test_restatement_wrapper_reproduces_the_goldens(name):
    _, _, _, _, w, _, steps = OL.load_mith(name)
    for st in steps:
        own = MC.restate(st["inputs"], st["buf"], st["label_sim"], w)
        terms, grads = OL.mith_oracle(st["inputs"], st["buf"], st["label_sim"], w)
        # the same float64 ops; only the thread count of the reductions may differ
        assert MC.rel_err(own["terms"], terms) <= 1e-13
        assert all(MC.rel_err(own["g_" + k], g) <= 1e-13 for k, g in zip(MC.INPUTS, grads))
        # the bounds of tests/test_mith_loss_cpu.py against the reference's fp32 run
        assert np.allclose(own["terms"], st["terms"], rtol=2e-5, atol=1e-6), (name, own["terms"], st["terms"])
        for k, ref in zip(MC.INPUTS, st["grads"]):
            assert grads_close(own["g_" + k], ref), (name, k)


def test_float32_restatement_keeps_its_dtype_and_the_pool_is_an_fp32_error():
    _, _, _, _, w, _, steps = OL.load_mith("odd")
    st = steps[0]
    for dtype in (torch.float32, torch.float64):
        t = OL.mith_terms([torch.tensor(x).to(dtype) for x in st["inputs"]], torch.tensor(st["buf"]).to(dtype),
                          torch.tensor(st["label_sim"]).to(dtype), w)
        assert all(v.dtype == dtype for v in t)
    assert OL.load_mith("weights")[4] == MC.WSETS["golden"] and MC.WSETS["golden"]["hyper_alpha"] == 0.0
    pool = MC.golden_pool()
    print("golden pool", "  ".join("%s %.2e" % kv for kv in pool.items()))
    for kind in MC.KINDS:                             # a few fp32 roundings: neither exact nor loose
        assert 2.0 ** -28 < pool[kind] < 2.0 ** -19, (kind, pool[kind])


def test_likelihood_grid_copy_gives_the_hand_computed_triples():
    """(ctiles, P, rows) by hand from the kernel's formula: 64-wide tiles of 4B columns; P = min(ceil(1024 / ctiles), row tiles), then
    per = ceil(tiles / P) row tiles per chunk and P = ceil(tiles / per)"""
    assert MC.lik_grid(130, 17) == (2, 3, 64)                 # 68 columns, 3 row tiles, one per chunk
    assert MC.lik_grid(2100, 1024) == (64, 11, 192)           # 33 tiles, target 16 -> 3 per chunk -> 11 chunks
    assert MC.lik_grid(4200, 256) == (16, 33, 128)            # 66 tiles, target 64 -> 2 per chunk -> 33 chunks, below the target
    assert MC.lik_grid(1 << 22, 2) == (1, 1024, 4096)         # 65536 tiles, 64 per chunk
    assert MC.lik_grid(10000, 100) == (7, 79, 128)            # 157 tiles, target 147 -> 2 per chunk -> 79 chunks
    assert MC.lik_grid(1, 1) == (1, 1, 64) and MC.lik_grid(64, 1024) == (64, 1, 64) and MC.lik_grid(65, 1024) == (64, 2, 64)
    assert MC.edge_rows(130, 17) == [0, 63, 64, 127, 128, 129]
    assert MC.edge_rows(2100, 1024)[-3:] == [1919, 1920, 2099] and len(MC.edge_rows(2100, 1024)) == 22
    assert MC.edge_rows(70, 3) == [0, 63, 64, 69]


@pytest.mark.parametrize("name", list(MC.CASES))
def test_every_case_builds_and_meets_the_conditions_on_its_inputs(name):
    c = MC.build(name)
    m = MC.check_conditions(name)
    print(name, MC.describe(m))
    assert c["redrawn"] <= 0.02 * c["N"]              # the cap: a handful of rows near the clamp, not a systematic cluster
    ref, r32 = MC.reference(name), MC.reference(name, dtype=torch.float32)
    zero = {k for k in MC.KINDS[1:] if not ref[k].any()}
    assert zero == set(c.get("zero", ())), (name, zero)
    for k in zero:                                    # where float64 vanishes identically the float32 restatement does too
        assert not r32[k].any(), (name, k)
    assert all(np.isfinite(ref[k]).all() and np.isfinite(r32[k]).all() for k in MC.KINDS)
    e_ref = MC.errors(r32, ref)
    print(name, "e_ref", "  ".join("%s %.2e" % kv for kv in e_ref.items()))


@pytest.mark.parametrize("name", [n for n in MC.CASES if MC.CASES[n]["N"] <= 5000])
def test_building_a_case_is_deterministic(name):
    first = MC.build(name)
    keep = {k: first[k].clone() for k in ("Y", "S")}
    xs = [t.clone() for t in first["xs"]]
    MC._built.pop(name)
    try:
        again = MC.build(name)
        assert all(torch.equal(keep[k], again[k]) for k in keep) and all(torch.equal(a, b) for a, b in zip(xs, again["xs"]))
    finally:
        MC._built[name] = first                       # the shared references belong to the first build


def test_row_effect_is_what_leaving_the_row_out_changes():
    """the closed form behind the edge-row condition against the restatement with that row left out, in float64"""
    name, w = "n130_b17_k65_d17", MC.WSETS["lik_only"]
    c = MC.build(name)
    ref = MC.reference(name, "lik_only")
    for n in (0, 64, 129):
        out = MC.restate_broken(c["xs"], c["Y"], c["S"], w, drop_row=n, dtype=torch.float64)
        dt, dg = MC.row_effect(c, n, w)
        for i, t, g in zip(MC.CODES, dt, dg):
            k, q = "g_" + MC.INPUTS[i], MC.LIK_OF[i]
            assert abs(abs(out["terms"][q] - ref["terms"][q]) - t) <= 1e-12 * abs(ref["terms"][q])
            assert abs(np.abs(out[k] - ref[k]).max() - g) <= 1e-12 * np.abs(ref[k]).max()
    same = MC.restate_broken(c["xs"], c["Y"], c["S"], w, dtype=torch.float64)          # no defect: the restatement itself
    assert all(MC.rel_err(same[k], ref[k]) <= 1e-13 for k in MC.KINDS)


@pytest.mark.parametrize("wname", ["default", "lik_only"])
def test_comparison_fails_a_restatement_that_loses_the_last_buffer_row(wname):
    name, w = "n130_b17_k65_d17", MC.WSETS[wname]
    c = MC.build(name)
    ref, r32 = MC.reference(name, wname), MC.reference(name, wname, torch.float32)
    MC.compare(name + " float32 restatement", r32, ref, r32)                              # passes its own yardstick
    broken = MC.restate_broken(c["xs"], c["Y"], c["S"], w, drop_row=c["N"] - 1)
    with pytest.raises(AssertionError):
        MC.compare(name + " last row lost", broken, ref, r32, kinds=("terms",))
    for i in MC.CODES:
        with pytest.raises(AssertionError):
            MC.compare(name + " last row lost", broken, ref, r32, kinds=("g_" + MC.INPUTS[i],))


@pytest.mark.parametrize("name", ["n130_b4_k256_d32_pm1", "n130_b4_k192_d32_pm1"])
def test_comparison_fails_a_restatement_with_the_open_interval_mask(name):
    c = MC.build(name)
    w = MC.WSETS["default"]
    ref, r32 = MC.reference(name), MC.reference(name, dtype=torch.float32)
    broken = MC.restate_broken(c["xs"], c["Y"], c["S"], w, open_mask=True)
    assert MC.rel_err(broken["terms"], ref["terms"]) <= MC.TOL_FACTOR * MC.golden_pool()["terms"]      # the forward is the same
    for i in MC.CODES:
        with pytest.raises(AssertionError):
            MC.compare(name + " open mask", broken, ref, r32, kinds=("g_" + MC.INPUTS[i],))
    # and through the differenced runs of the GPU module's clamp-edge test
    lo, hi = MC.with_edge_S(c, 0.0), MC.with_edge_S(c, 1.0)
    diff = lambda f, **kw: {k: f(c["xs"], c["Y"], hi, w, **kw)[k] - f(c["xs"], c["Y"], lo, w, **kw)[k] for k in MC.KINDS}  # noqa: E731
    dref, d32 = diff(MC.restate), diff(MC.restate, dtype=torch.float32)
    kinds = tuple("g_" + MC.INPUTS[i] for i in MC.CODES)
    MC.compare(name + " edge rows, float32 restatement", d32, dref, d32, kinds=kinds)
    dbroken = diff(MC.restate_broken, open_mask=True)
    for k in kinds:
        with pytest.raises(AssertionError):
            MC.compare(name + " edge rows, open mask", dbroken, dref, d32, kinds=(k,))


@pytest.mark.parametrize("name", list(MC.NONFINITE))
def test_nan_patterns_of_the_reference_expression(name):
    xs, Y, S, idx = MC.build_nonfinite(name)
    assert Y.shape == (MC.NF_N, MC.NF_K) and S.shape == (MC.NF_N, MC.NF_B) and xs[0].shape == (MC.NF_B, MC.NF_D)
    assert MC.lik_grid(MC.NF_N, MC.NF_B) == (1, 2, 64) and MC.NF_ROW >= 64         # the poisoned row lies in the second chunk
    bad = [int((~torch.isfinite(t)).sum()) for t in xs + [Y]]
    assert bad == {"nan_buffer_entry": [0] * 8 + [1], "nan_code_entry": [0, 0, 1, 0, 0, 0, 0, 0, 0],
                   "nan_feature_entry": [1] + [0] * 8, "inf_buffer_row": [0] * 8 + [MC.NF_K]}[name]
    if name == "inf_buffer_row":                      # every code row has entries of both signs: inf - inf in every product
        assert all(bool(((xs[i] > 0).any(1) & (xs[i] < 0).any(1)).all()) for i in MC.CODES)
    for dtype in (torch.float64, torch.float32):
        r = MC.restate(xs, Y, S, MC.DEFAULT, dtype)
        got, want = MC.nan_pattern(r), MC.recorded_pattern(name, r)
        assert got[0] == want[0], (name, dtype, got[0])
        for k in MC.KINDS[1:]:
            assert np.array_equal(got[1][k], want[1][k]), (name, dtype, k, got[1][k])
    # the same batch without the poke is finite throughout: the NaNs above come from the poke alone
    clean = [torch.where(torch.isfinite(t), t, torch.full_like(t, 0.5)) for t in xs + [Y]]
    r = MC.restate(clean[:8], clean[8], S, MC.DEFAULT)
    assert all(np.isfinite(r[k]).all() for k in MC.KINDS)
