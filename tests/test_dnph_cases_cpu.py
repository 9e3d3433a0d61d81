"""CPU: the conditions that the edge cases of tests/dnph_cases.py (EDGE_CASES, NONFINITE) promise of their inputs, so that the bounds of
tests/test_gpu_dnph_loss_f64.py mean what they say.  Nothing here runs the port: these are statements about the inputs and about the
float64 / float32 restatements, and every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

import dnph_cases as DC

KEYS = ("labels", "f_img", "f_txt", "p_img", "p_txt", "P", "noise_img", "noise_txt")


def _classes_of(row):
    return tuple(int(i) for i in np.nonzero(row)[0])


def _lowest(labels):
    """per row with a label: its lowest class"""
    return np.array([int(np.argmax(r)) for r in labels if r.any()])


@pytest.mark.parametrize("name", list(DC.EDGE_CASES))
def test_shapes_ranges_and_named_label_rows(name):
    spec, c = DC.EDGE_CASES[name], DC.build_edge(name)
    B, K, C, Cp = spec["B"], spec["K"], spec["C"], spec["Cp"]
    assert c["labels"].shape == (B, C) and c["f_img"].shape == c["f_txt"].shape == c["noise_img"].shape == c["noise_txt"].shape == (B, K)
    assert c["p_img"].shape == c["p_txt"].shape == (B, Cp) and c["P"].shape == (C, K)
    assert all(c[k].dtype == np.float32 and np.isfinite(c[k]).all() for k in KEYS[1:]) and set(np.unique(c["labels"])) <= {0, 1}
    assert set(np.unique(c["noise_img"])) == set(np.unique(c["noise_txt"])) == {-1.0, 1.0}
    ranges = {k: {v[k] for v in DC.CASES.values()} for k in ("mrg", "alpha", "up")}
    assert all(min(ranges[k]) <= spec[k] <= max(ranges[k]) for k in ranges), (name, ranges)
    for row, classes in spec.get("set_labels", {}).items():
        want = tuple(range(C)) if classes == "all" else tuple(sorted(classes))
        assert _classes_of(c["labels"][row]) == want, (name, row)
    if B >= 3 and not spec.get("eye") and 0 not in spec.get("set_labels", {}):
        assert not c["labels"][0].any()
    if B >= 3 and not spec.get("eye"):
        assert c["labels"][1].all()


def test_the_table_has_the_upstreams_and_weights_asked_for():
    assert sum(v["up"] != 1.0 for v in DC.EDGE_CASES.values()) >= 2 and any(v["alpha"] == 1.0 for v in DC.EDGE_CASES.values())
    assert not set(DC.EDGE_CASES) & set(DC.CASES)                                    # pool() is over CASES alone


def test_label_words():
    lab = {n: DC.build_edge(n)["labels"] for n in ("b5_k257_c33", "b9_k100_c1024", "b129_k65_c65", "b97_k16_c97_eye")}
    rows = sorted(_classes_of(r) for r in lab["b5_k257_c33"])
    assert rows == sorted([(), tuple(range(33)), (32,), (31,), (31, 32)])            # class 32 alone in word 1, bit 31, both, none, all
    low = _lowest(lab["b9_k100_c1024"])
    print("b9_k100_c1024 lowest labels", low.tolist(), "words", (low // 32).tolist())
    assert 15 in low // 32 and 31 in low // 32 and 31 in low % 32 and 16 in low // 32 and 0 in low // 32
    assert lab["b9_k100_c1024"][:, 992:].any() and (lab["b9_k100_c1024"].sum(1) == 0).sum() == 1
    b129 = [_classes_of(r) for r in lab["b129_k65_c65"]]
    assert (64,) in b129 and (31, 64) in b129 and b129[128] == (64,)                  # word 2 alone; the last row of either modality
    eye = lab["b97_k16_c97_eye"]
    assert np.array_equal(eye, np.eye(97, dtype=eye.dtype)) and np.array_equal(np.argmax(eye, 1), np.arange(97))
    assert np.array_equal(eye, torch.ones([97], dtype=torch.int).diag().numpy())     # DNPH.object_function's construction


def test_norms_keep_clear_of_the_eps_branch():
    """the clamped case's zero and tiny rows lie at most at 0.5e-12, every other row of every case at 1e-3 or more"""
    for name in DC.EDGE_CASES:
        c, n = DC.build_edge(name), DC.row_norms(DC.build_edge(name))
        spec = DC.EDGE_CASES[name]
        low = {"g_f_img": [spec["zero_img"]] if "zero_img" in spec else [], "g_f_txt": [spec["tiny_txt"][0]] if "tiny_txt" in spec else [],
               "g_P": [spec[k] if k == "zero_P" else spec[k][0] for k in ("tiny_P", "zero_P") if k in spec]}
        for g, rows in low.items():
            rest = np.delete(n[g], rows)
            print("%-22s %-8s smallest other norm %.3e  clamped rows %s norms %s" % (name, g, rest.min(), rows, n[g][rows].tolist()))
            assert rest.min() >= 1e-3 and (n[g][rows] <= 0.5e-12).all(), (name, g)
            assert np.array_equal(np.nonzero(DC.clamped_rows(c)[g])[0], np.sort(np.array(rows, dtype=np.int64)))
    c = DC.build_edge("b33_k64_c24_clamped")
    assert not c["f_img"][5].any() and not c["P"][2].any()
    for k, row in (("f_txt", 9), ("P", 7)):                                           # non-zero and clamped, in float32 as well
        n32 = float(torch.tensor(c[k][row]).norm())
        print("%s[%d] float32 norm %.3e  float64 norm %.3e" % (k, row, n32, np.linalg.norm(c[k][row].astype(np.float64))))
        assert 0.0 < n32 < 0.5e-12 and (c[k][row] != 0).all()
    assert c["labels"][5].any() and c["labels"][9].any() and c["labels"][:, 7].any() and c["labels"][:, 2].any()   # the rows take part


def test_k1_gradients_are_residue_of_parts_that_cancel():
    c = DC.build_edge("b40_k1_c3")
    r64, _, floor, _ = DC.edge_reference("b40_k1_c3")
    part = DC.normalize_part(c, r64)
    assert len(set(np.sign(c["P"].ravel()))) == 2 and c["labels"].any(1).all()
    for g in DC.CODE_OF:
        ratio = np.abs(part[g]).max(1) / floor[g]
        print("b40_k1_c3 %-8s smallest floor %.3e  largest |normalise part| %.3e  largest part / floor %.3e (2^-40 = %.3e)" %
              (g, floor[g].min(), np.abs(part[g]).max(), ratio.max(), 2.0 ** -40))
        assert (floor[g] > 0).all() and (ratio <= 2.0 ** -40).all(), g


def test_large_logits_overflow_expf_without_the_maximum():
    c = DC.build_edge("b37_k48_c24_logits")
    r64 = DC.edge_reference("b37_k48_c24_logits")[0]
    for m in ("img", "txt"):
        big = float(c["p_" + m].max())
        with np.errstate(over="ignore"):
            overflow = np.exp(np.float32(big))
        print("b37_k48_c24_logits p_%s max p %.2f  float32 exp -> %s  float64 d_loss %.6f" %
              (m, big, overflow, r64["d_loss_" + m][0]))
        assert big > 89 and np.isinf(overflow) and np.isfinite(r64["d_loss_" + m]).all()


@pytest.mark.parametrize("name", list(DC.EDGE_CASES))
def test_yardstick_is_a_real_float32_error(name):
    """per tensor kind the largest e_ref of the case lies in (2^-30, 2^-16): neither an exact agreement that would leave the bound to
    the pool alone, nor a float32 restatement that has lost the result"""
    r64, r32, _, e_ref = DC.edge_reference(name)
    assert all(np.isfinite(v).all() for v in r64.values()) and all(np.isfinite(v).all() for v in r32.values())
    kinds = {}
    for key, e in e_ref.items():
        print("%-22s %-16s e_ref %.3e" % (name, key, e))
        kinds[DC.kind_of(key)] = max(kinds.get(DC.kind_of(key), 0.0), e)
    print(name, {k: "%.3e" % v for k, v in kinds.items()})
    assert set(kinds) == {"term", "g_f", "g_p", "g_P"}
    assert all(2.0 ** -30 < v < 2.0 ** -16 for v in kinds.values()), (name, kinds)


def test_building_is_deterministic():
    for name in DC.EDGE_CASES:
        a = DC.build_edge(name)
        DC.build_edge.cache_clear()
        b = DC.build_edge(name)
        assert a is not b and all(np.array_equal(a[k], b[k]) for k in KEYS), name
    for name in DC.NONFINITE:
        a = DC.build_nonfinite(name)
        DC.build_nonfinite.cache_clear()
        b = DC.build_nonfinite(name)
        assert a is not b and all(np.array_equal(a[k], b[k], equal_nan=True) for k in KEYS), name


@pytest.mark.parametrize("name", list(DC.NONFINITE))
def test_nonfinite_patterns_are_the_recorded_ones(name):
    c, clean = DC.build_nonfinite(name), DC.build_nonfinite(name, poke=False)
    poked = [k for k in KEYS if not np.array_equal(c[k], clean[k])]
    assert len(poked) == 1 and int((~np.isfinite(c[poked[0]])).sum()) == 1            # one poke: a single entry of a single input
    t, o = DC.nonfinite_target(clean, 2)
    assert clean["labels"][2, t] == 1 and not clean["labels"][2, :t].any() and o != t
    c64, c32 = DC.classes(DC.objective(c, torch.float64)), DC.classes(DC.objective(c, torch.float32))
    want = DC.recorded_classes(name)
    for k in want:
        print("%-24s %-10s not finite: float64 %d  float32 %d  recorded %d of %d" %
              (name, k, (c64[k] != 0).sum(), (c32[k] != 0).sum(), (want[k] != 0).sum(), want[k].size))
    assert set(c64) == set(c32) == set(want)
    assert all(np.array_equal(c64[k], want[k]) and np.array_equal(c32[k], want[k]) for k in want), name
    for dtype in (torch.float64, torch.float32):                                      # the same batch without the poke is finite throughout
        assert all(np.isfinite(v).all() for v in DC.objective(clean, dtype).values())
    if name == "neginf_logit_off_target":                                             # that entry's gradient is exactly 0
        assert DC.objective(c, torch.float64)["g_p_img"][2, o] == 0 and DC.objective(c, torch.float32)["g_p_img"][2, o] == 0
