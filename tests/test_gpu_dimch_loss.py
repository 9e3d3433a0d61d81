"""GPU: xmh_dimch_loss / xmh_dimch_loss_grad (csrc/xmh_dimch.hip) against the float64 restatement of DIMCH's objective
(tests/dimch_cases.py), called through the C ABI, and once through the Python layer (xmh.models.dimch.DIMCHObjective).

Rule (tests/test_gpu_dnph_loss.py's): per tensor e = max|got - f64| / max|f64| <= TOL_FACTOR = 4 times the float32 restatement's e on
the same inputs (or the largest such e of that tensor kind over CASES, whichever is larger).  Every ratio is printed before the first
assertion.  The nine terms and the four gradients of every case of dimch_cases.CASES: (B, M, K) = (3, 1, 16), (7, 5, 6) in all four
distance modes, (20, 8, 16), (9, 64, 32), (33, 8, 64), (65, 3, 130), (5, 4, 100), (258, 2, 8); C = 1, 24, 80, 127; the softmax quantiser; sigma != 1; upstreams
other than 1; one sample whose text tokens are its image tokens (clamp(1 - s, 0) active).  Further: accumulate, single NULL gradients,
two calls to the bit, a row without a label (NaN), a NaN input, and the golden cases against the reference's recorded numbers.

Measured on an MI355X, worst e / yardstick over the tensors of a case (the bound is 4): 1.12 (g_h_txt of b7_m5_k6_clamp), 0.69
(b5_m4_k100), 0.65 (b20_m8_k16_softmax), 0.57 (b3_m1_k16), 0.56 (b65_m3_k130, b20_m8_k16_sigma), 0.55 (b7_m5_k6_chamfer), 0.54
(b7_m5_k6_max), 0.49 (b7_m5_k6_avg), 0.43 (b33_m8_k64), 0.38 (b9_m64_k32), 0.35 (b20_m8_k16), 0.33 (b7_m5_k6_smooth), 0.22
(b7_m5_k6_c1), 0.19 (b258_m2_k8_c1), 0.63 (upstream -3).  Against the reference's recorded float64 numbers: 0.88 at most (g_h_txt of
g_softmax and of g_max)."""
import numpy as np
import pytest
import torch

import dimch_cases as DC

pytestmark = pytest.mark.gpu


def _consts(c, **over):
    from xmh.models.dimch import DimchConsts, HASH_FUNCS, mode_index
    k = dict(DC.consts(c), **over)
    return DimchConsts(mode_index(k["mode"]), HASH_FUNCS.index(k["hash_func"]), *[k[f] for f in DC.CONST_KEYS if f not in ("mode", "hash_func")])


def _dev(c):
    from xmh import retrieval as R
    d = {k: torch.tensor(np.asarray(c[k], np.float32)).cuda().contiguous() for k in DC.INPUTS}
    d["lab"] = R.pack_labels(torch.tensor((np.asarray(c["labels"]) == 1).astype(np.uint8)).cuda())
    return d


def _call(c, d, up=None, accumulate=0, into=None, skip=(), **over):
    """one xmh_dimch_loss and one xmh_dimch_loss_grad -> (out12 float64 numpy, {gradient name: device tensor or None})"""
    import ctypes
    from xmh._lib import check, current_stream, lib, ptr
    B, M, K, C = c["B"], c["M"], c["K"], c["C"]
    up = c.get("up", 1.0) if up is None else up
    cst = _consts(c, **over)
    nbytes = lib.xmh_dimch_loss_ws_bytes(B, M, K, C)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    out = torch.full((12,), 7.0, dtype=torch.float64, device="cuda")
    args = [ptr(d[k]) for k in DC.INPUTS] + [B, M, K, d["h_img"].shape[1], C, ptr(d["lab"]), ctypes.byref(cst)]
    check(lib.xmh_dimch_loss(*args, ptr(ws), nbytes, ptr(out), current_stream()), "xmh_dimch_loss")
    upt = None if up == 1.0 else torch.tensor([up], dtype=torch.float32, device="cuda")
    grads = {}
    for g, k in zip(DC.GRADS, DC.INPUTS):
        grads[g] = None if g in skip else (into[g] if into is not None else torch.full_like(d[k], 3.0))
    check(lib.xmh_dimch_loss_grad(*args, ptr(upt), *[ptr(grads[g]) for g in DC.GRADS], accumulate, ptr(ws), nbytes, current_stream()),
          "xmh_dimch_loss_grad")
    torch.cuda.synchronize()
    return out.cpu().numpy(), grads


def _port(c, d=None, **kw):
    d = _dev(c) if d is None else d
    out, grads = _call(c, d, **kw)
    assert (out[9:] == 0).all()
    vals = {k: out[i:i + 1] for i, k in enumerate(DC.TERMS)}
    vals.update({g: t.cpu().double().numpy() for g, t in grads.items() if t is not None})
    return vals


@pytest.mark.parametrize("name", list(DC.CASES))
def test_terms_and_gradients_against_float64(name):
    c = DC.build(name)
    got = _port(c)
    assert all(np.isfinite(v).all() for v in got.values())
    if c["M"] == 1:
        assert got["unif"][0] == 0
    if c["C"] == 1:
        assert got["T_i2t"][0] == 0 and got["Th_t2i"][0] == 0                        # no negatives: no triplet
    if c.get("clamp"):
        # the designed sample: 1 - s < 0 there in float64, so both its distances are clamped to 0
        r = DC.CLAMP_ROW
        x = torch.tensor(c["e_img"], dtype=torch.float64)
        u = torch.nn.functional.normalize(x.reshape(-1, c["K"]), dim=-1)
        s = DC.set_similarity(u, u, c["M"], DC.consts(c))
        assert float(s[r, r]) > 1 + 1e-5
    worst = DC.compare(name, got, DC.reference(name), DC.e_ref(name))
    print(name, "worst ratio %.2f" % worst)


def test_upstream_against_float64():
    c = DC.build("b20_m8_k16")
    r64, r32 = DC.objective(c, torch.float64, up=-3.0), DC.objective(c, torch.float32, up=-3.0)
    DC.compare("up_-3", _port(c, up=-3.0), r64, {k: DC.rel_err(r32[k], r64[k]) for k in r64})


def test_accumulate_null_gradients_and_bit_identity():
    c = DC.build("b65_m3_k130")
    d = _dev(c)
    out_a, ga = _call(c, d)
    out_b, gb = _call(c, d)
    assert np.array_equal(out_a, out_b) and all(torch.equal(ga[g], gb[g]) for g in DC.GRADS)      # two calls agree to the bit
    assert all(bool((ga[g] != 3.0).all()) for g in DC.GRADS)                         # every entry was written
    _, twice = _call(c, d, accumulate=1, into={g: t.clone() for g, t in ga.items()})
    assert all(torch.equal(twice[g], 2 * ga[g]) for g in DC.GRADS)                   # x + x is exact: the same gradient was added
    for g in DC.GRADS:                                                               # one gradient not asked for: the others unchanged
        _, part = _call(c, d, skip=(g,))
        assert part[g] is None and all(torch.equal(part[o], ga[o]) for o in DC.GRADS if o != g), g
    _, pair = _call(c, d, skip=("g_e_img", "g_h_img"))                               # a whole modality
    assert torch.equal(pair["g_e_txt"], ga["g_e_txt"]) and torch.equal(pair["g_h_txt"], ga["g_h_txt"])


def test_a_row_without_a_label_gives_nan():
    c = dict(DC.build("b7_m5_k6_smooth"))
    c["labels"] = c["labels"].copy()
    c["labels"][0] = 0
    r32 = DC.objective(c, torch.float32)
    got = _port(c)
    for k in ("loss", "T_i2t", "T_t2i", "Th_i2t", "Th_t2i"):
        assert np.isnan(r32[k][0]) and np.isnan(got[k][0]), k
    for k in ("mmd", "unif", "Q_img", "Q_txt"):
        assert np.isfinite(got[k][0]), k


def test_a_nan_input_passes_through():
    c = dict(DC.build("b7_m5_k6_smooth"))
    c["e_txt"] = c["e_txt"].copy()
    c["e_txt"][3, 1, 2] = np.nan
    r32 = DC.objective(c, torch.float32)
    got = _port(c)
    for k in ("loss", "T_i2t", "T_t2i", "mmd", "unif"):
        assert np.isnan(r32[k][0]) and np.isnan(got[k][0]), k
    for k in ("Th_i2t", "Th_t2i", "Q_img", "Q_txt"):
        assert np.isfinite(got[k][0]), k
    assert np.isnan(got["g_e_txt"][3, 1]).all() and np.isfinite(got["g_h_img"]).all() and np.isfinite(got["g_h_txt"]).all()


def _golden(name):
    G = np.load(DC.GOLDEN)
    g = {k.split("__", 1)[1]: G[k] for k in G.files if k.startswith(name + "__")}
    c = dict(DC.GOLDEN_CASES[name], **{k: g[k] for k in DC.INPUTS}, labels=g["labels"].astype(np.int64), up=1.0)
    return g, c, {kind: float(G["deviation__" + kind]) for kind in DC.KINDS}


@pytest.mark.parametrize("name", list(DC.GOLDEN_CASES))
def test_golden_cases_against_the_reference(name):
    """the reference's own recorded float64 numbers: the same rule, the yardstick being the reference's own float32-against-float64
    deviation of that tensor (or the largest recorded of its kind)"""
    g, c, dev = _golden(name)
    got = _port(c)
    rows = []
    for k in DC.TERMS + DC.GRADS:
        yard = max(dev[DC.kind_of(k)], DC.rel_err(g["f32_" + k], g["f64_" + k]))
        rows.append((k, DC.rel_err(got[k], g["f64_" + k]), yard))
        print("%-10s %-8s e %.3e  yardstick %.3e  ratio %.2f" % (name, k, rows[-1][1], yard, rows[-1][1] / yard))
    for k, e, yard in rows:
        assert e <= DC.TOL_FACTOR * yard, (name, k, e, yard)


def test_python_layer_matches_the_c_call():
    from xmh.models.dimch import DIMCHObjective
    c = DC.build("b20_m8_k16")
    k = DC.consts(c)
    mod = DIMCHObjective(**k)
    leaves = {n: torch.tensor(c[n]).cuda().requires_grad_(True) for n in DC.INPUTS}
    loss, d = mod(leaves["e_img"], leaves["h_img"], leaves["e_txt"], leaves["h_txt"], torch.tensor(c["labels"]))
    loss.backward()
    out, grads = _call(c, _dev(c), up=1.0)
    assert float(loss) == float(np.float32(out[0])) and float(d["All loss"]) == float(loss)
    assert float(d["Tokens"]["Maximum Mean Discrepancy"]) == float(np.float32(out[3]))
    assert float(d["Hash"]["Quantization"]["text"]) == float(np.float32(out[8]))
    for g, n in zip(DC.GRADS, DC.INPUTS):
        assert torch.equal(leaves[n].grad, grads[g]), g
