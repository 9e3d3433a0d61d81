"""GPU: xmh_umoed_loss / xmh_umoed_loss_grad (csrc/xmh_umoed.hip) against the float64 restatement of UMoED's pairwise objective
(tests/umoed_cases.py), called through the C ABI, and once through the Python layer (xmh.models.umoed.UMoEDObjective).

Rule (tests/test_gpu_dimch_loss.py's): per tensor e = max|got - f64| / max|f64| <= TOL_FACTOR = 4 times the float32 restatement's e on the
same inputs (or the largest such e of that tensor kind over LOSS_CASES, whichever is larger).  Every ratio is printed before the first
assertion.  The five terms and both gradients of every case of umoed_cases.LOSS_CASES: (B, M, V, C) = (7, 5, 2, 4) with the softmax on
and off, (20, 8, 16, 6), (9, 64, 2, 5), (6, 1, 2, 3) where U = 0, a sample whose text set is its image set with two equal token rows,
(258, 3, 2, 1).  Further: accumulate, a NULL gradient, two calls to the bit, a row without a label (NaN), the golden cases against the
reference's recorded numbers.

Measured on an MI355X, worst e / yardstick over the tensors of a case (the bound is 4): 2.11 (U_txt of b20_m8_v16), 1.41 (g_e_txt of
b7_m5_v2_extreme), 0.92 (b258_m3_v2_c1), 0.78 (same_set), 0.65 (b9_m64_v2), 0.52 (b7_m5_v2_plain), 0.45 (b6_m1_v2).  Against the
reference's recorded float64 numbers: 0.83 at most (T_t2i of g_m64)."""
import ctypes

import numpy as np
import pytest
import torch

import umoed_cases as UC

pytestmark = pytest.mark.gpu


def _consts(c, **over):
    from xmh._lib import UmoedConsts
    k = dict(UC.consts(c), **over)
    return UmoedConsts(int(k["extreme"]), k["extreme_T"], k["token_triplet_margin"], k["triplet_alpha"], k["unif_alpha"])


def _dev(c):
    from xmh import retrieval as R
    d = {k: torch.tensor(np.asarray(c[k], np.float32)).cuda().contiguous() for k in UC.INPUTS}
    d["lab"] = R.pack_labels(torch.tensor((np.asarray(c["labels"]) == 1).astype(np.uint8)).cuda())
    return d


def _call(c, d, up=None, accumulate=0, into=None, skip=()):
    """one xmh_umoed_loss and one xmh_umoed_loss_grad -> (out8 float64 numpy, {gradient name: device tensor or None})"""
    from xmh._lib import check, current_stream, lib, ptr
    B, M, V, C = c["B"], c["M"], c["V"], c["C"]
    up = c.get("up", 1.0) if up is None else up
    cst = _consts(c)
    nbytes = lib.xmh_umoed_loss_ws_bytes(B, M, V, C)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    out = torch.full((8,), 7.0, dtype=torch.float64, device="cuda")
    args = [ptr(d["e_img"]), ptr(d["e_txt"]), B, M, V, C, ptr(d["lab"]), ctypes.byref(cst)]
    check(lib.xmh_umoed_loss(*args, ptr(ws), nbytes, ptr(out), current_stream()), "xmh_umoed_loss")
    upt = None if up == 1.0 else torch.tensor([up], dtype=torch.float32, device="cuda")
    grads = {}
    for g, k in zip(UC.GRADS, UC.INPUTS):
        grads[g] = None if g in skip else (into[g] if into is not None else torch.full_like(d[k], 3.0))
    check(lib.xmh_umoed_loss_grad(*args, ptr(upt), *[ptr(grads[g]) for g in UC.GRADS], accumulate, ptr(ws), nbytes, current_stream()),
          "xmh_umoed_loss_grad")
    torch.cuda.synchronize()
    return out.cpu().numpy(), grads


def _port(c, d=None, **kw):
    d = _dev(c) if d is None else d
    out, grads = _call(c, d, **kw)
    assert (out[5:] == 0).all()
    vals = {k: out[i:i + 1] for i, k in enumerate(UC.TERMS)}
    vals.update({g: t.cpu().double().numpy() for g, t in grads.items() if t is not None})
    return vals


@pytest.mark.parametrize("name", list(UC.LOSS_CASES))
def test_terms_and_gradients_against_float64(name):
    c = UC.loss_case(name)
    got = _port(c)
    assert all(np.isfinite(v).all() for v in got.values())
    r64 = UC.loss_reference(name)
    if c["M"] == 1:
        assert got["U_img"][0] == 0 and got["U_txt"][0] == 0
    if c["C"] == 1:
        assert got["T_i2t"][0] == 0 and got["T_t2i"][0] == 0                         # no negatives: no triplet
    else:
        assert r64["T_i2t"][0] > 0 and got["T_i2t"][0] > 0                           # the triplet terms are live
    worst = UC.compare(name, got, r64, UC.loss_e_ref(name), UC.loss_pool())
    print(name, "worst ratio %.2f" % worst)


def test_accumulate_null_gradients_and_bit_identity():
    c = UC.loss_case("b20_m8_v16")
    d = _dev(c)
    out_a, ga = _call(c, d)
    out_b, gb = _call(c, d)
    assert np.array_equal(out_a, out_b) and all(torch.equal(ga[g], gb[g]) for g in UC.GRADS)      # two calls agree to the bit
    assert all(bool((ga[g] != 3.0).all()) for g in UC.GRADS)                         # every entry was written
    _, twice = _call(c, d, accumulate=1, into={g: t.clone() for g, t in ga.items()})
    assert all(torch.equal(twice[g], 2 * ga[g]) for g in UC.GRADS)                   # x + x is exact: the same gradient was added
    for g in UC.GRADS:                                                               # one gradient not asked for: the other unchanged
        _, part = _call(c, d, skip=(g,))
        assert part[g] is None and all(torch.equal(part[o], ga[o]) for o in UC.GRADS if o != g), g
    _call(c, d, skip=UC.GRADS)                                                       # neither: nothing to do, no error


def test_a_row_without_a_label_gives_nan():
    c = dict(UC.loss_case("b7_m5_v2_extreme"))
    c["labels"] = c["labels"].copy()
    c["labels"][0] = 0
    r32 = UC.objective(c, torch.float32)
    got = _port(c)
    for k in ("loss", "T_i2t", "T_t2i"):
        assert np.isnan(r32[k][0]) and np.isnan(got[k][0]), k
    for k in ("U_img", "U_txt"):
        assert np.isfinite(got[k][0]) and abs(got[k][0] - r32[k][0]) <= 1e-5 * abs(r32[k][0]), k


@pytest.mark.parametrize("name", list(UC.GOLDEN_LOSS_CASES))
def test_golden_cases_against_the_reference(name):
    """the reference's own recorded float64 numbers: the same rule, the yardstick being the reference's own float32-against-float64
    deviation of that tensor (or the largest recorded of its kind)"""
    G = np.load(UC.GOLDEN)
    c = dict(UC.draw_loss(**UC.GOLDEN_LOSS_CASES[name]), up=1.0)
    assert int(G["loss__%s__seed" % name]) == c["seed"]
    got = _port(c)
    g64 = {k: G["loss__%s__f64_%s" % (name, k)] for k in UC.TERMS + UC.GRADS}
    own = {k: UC.rel_err(G["loss__%s__f32_%s" % (name, k)], g64[k]) for k in g64}
    UC.compare(name + " (reference)", got, g64, own, {kind: float(G["deviation__" + kind]) for kind in UC.KINDS})


def test_python_layer_matches_the_c_call():
    from xmh.models.umoed import UMoEDObjective
    c = UC.loss_case("b20_m8_v16")
    mod = UMoEDObjective(mode="pairwise", **UC.consts(c))
    leaves = {n: torch.tensor(c[n]).cuda().requires_grad_(True) for n in UC.INPUTS}
    loss, d = mod(leaves["e_img"], leaves["e_txt"], torch.tensor(c["labels"]))
    loss.backward()
    out, grads = _call(c, _dev(c), up=1.0)
    assert float(loss) == float(np.float32(out[0])) and float(d["All loss"]) == float(loss)
    sim, div = d["Tokens"]["Similarity"], d["Tokens"]["Diversity"]
    assert float(sim["t2i"]) == float(np.float32(out[2])) and float(div["i"]) == float(np.float32(out[3]))
    assert sim["it2i"] == 0 and sim["it2t"] == 0 and div["it"] == 0
    for g, n in zip(UC.GRADS, UC.INPUTS):
        assert torch.equal(leaves[n].grad, grads[g]), g
