"""GPU: xmh_dnph_loss / xmh_dnph_loss_grad (csrc/xmh_dnph.hip) against the float64 restatement of DNPH's objective
(tests/dnph_cases.py), called through the C ABI.

Rule (tests/test_gpu_tower_grad.py's): per tensor e = max|got - f64| / max|f64| <= TOL_FACTOR = 4 times the float32 restatement's e on
the same inputs (or the largest such e of that tensor kind over CASES, whichever is larger).  Every ratio is printed before the first
assertion.  The six terms and the five gradients of every case of dnph_cases.CASES: B = 1 .. 257, K = 16 .. 130, C = 1 .. 80 with
Cp = C and Cp = 80 > C, a row without a label, a row with every label, an all-zero code row (F.normalize's eps branch; compared whole
and with that row zeroed on both sides), mrg = 50, upstreams other than 1.  Further: no noise term (NULL), accumulate, single NULL
gradients, two calls to the bit, a NaN in a code row and in a proxy, and the golden cases against the reference's recorded numbers.

Measured on an MI355X, worst e / yardstick over the tensors of a case (the bound is 4): 2.50 (g_f_txt of b37_k48_c24_mrg50), 2.01
(g_p_img of b257_k48_c80), 0.92 (b65_k130_c32), 0.84 (b65_k16_c33_zero: nz_f_img; g_f_img whole 0.08), 0.78 (b37_k48_c24, and with no
or one noise), 0.77 (b37_k16_c33), 0.65 (upstream -3), 0.02 (b1_k16_c1).  Against the reference's recorded numbers: 8.1e-7 at most
(g_f_txt of `mid`) where the bound is 6.2e-6."""
import numpy as np
import pytest
import torch

import dnph_cases as DC

pytestmark = pytest.mark.gpu

INPUTS = ("f_img", "f_txt", "p_img", "p_txt", "P")
EPS32 = float(np.finfo(np.float32).eps)


def _dev(c):
    from xmh import retrieval as R
    d = {k: torch.tensor(np.asarray(c[k], np.float32)).cuda().contiguous() for k in INPUTS + ("noise_img", "noise_txt")}
    d["lab"] = R.pack_labels(torch.tensor((np.asarray(c["labels"]) == 1).astype(np.uint8)).cuda())
    return d


def _call(c, d, mrg=None, alpha=None, up=None, noise=True, accumulate=0, into=None, skip=()):
    """one xmh_dnph_loss and one xmh_dnph_loss_grad -> (out8 float64 numpy, {gradient name: device tensor or None})"""
    from xmh._lib import check, current_stream, lib, ptr
    B, K, C, Cp = c["B"], c["K"], c["C"], c["Cp"]
    mrg, alpha, up = (c["mrg"] if mrg is None else mrg), (c["alpha"] if alpha is None else alpha), (c["up"] if up is None else up)
    nbytes = lib.xmh_dnph_loss_ws_bytes(B, K, C, Cp)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    out = torch.full((8,), 7.0, dtype=torch.float64, device="cuda")
    ns = [ptr(d[k]) if noise else None for k in ("noise_img", "noise_txt")]
    args = [ptr(d[k]) for k in INPUTS] + [B, K, C, Cp, ptr(d["lab"]), mrg, alpha] + ns
    check(lib.xmh_dnph_loss(*args, ptr(ws), nbytes, ptr(out), current_stream()), "xmh_dnph_loss")
    upt = None if up is None or up == 1.0 else torch.tensor([up], dtype=torch.float32, device="cuda")
    grads = {}
    for g, k in zip(DC.GRADS, INPUTS):
        grads[g] = None if g in skip else (into[g] if into is not None else torch.full_like(d[k], 3.0))
    check(lib.xmh_dnph_loss_grad(*args, ptr(upt), *[ptr(grads[g]) for g in DC.GRADS], accumulate, ptr(ws), nbytes, current_stream()),
          "xmh_dnph_loss_grad")
    torch.cuda.synchronize()
    return out.cpu().numpy(), grads


def _port(c, d=None, **kw):
    d = _dev(c) if d is None else d
    out, grads = _call(c, d, **kw)
    assert out[6] == 0 and out[7] == 0
    vals = {k: out[i:i + 1] for i, k in enumerate(DC.TERMS)}
    vals.update({g: None if t is None else t.cpu().double().numpy() for g, t in grads.items()})
    return DC.expand(c, vals)


@pytest.mark.parametrize("name", list(DC.CASES))
def test_terms_and_gradients_against_float64(name):
    c = DC.build(name)
    got = _port(c)
    assert all(np.isfinite(v).all() for v in got.values())                           # mrg = 50 among them: the softmax stays finite
    worst = DC.compare(name, got, DC.reference(name), DC.e_ref(name))
    print(name, "worst ratio %.2f" % worst)


@pytest.mark.parametrize("variant", ["no_noise", "up_3", "one_noise"])
def test_variants_against_float64(variant):
    c = DC.build("b37_k48_c24")
    kw = {"no_noise": dict(noise=False), "up_3": dict(up=-3.0), "one_noise": dict(alpha=0.7)}[variant]
    d = _dev(c)
    if variant == "one_noise":                                                       # the text noise alone: the image one is NULL
        d = dict(d, noise_img=None)
        c = dict(c, noise_img=np.zeros_like(c["noise_img"]))
    r64, r32 = DC.objective(c, torch.float64, **kw), DC.objective(c, torch.float32, **kw)
    got = _port(c, d, **kw)
    if variant == "no_noise":
        assert got["noise_img"][0] == 0 and got["noise_txt"][0] == 0
        assert got["loss"][0] == got["p_loss"][0] + (got["d_loss_img"][0] + got["d_loss_txt"][0])
    DC.compare(variant, got, r64, {k: DC.rel_err(r32[k], r64[k]) for k in r64})


def test_accumulate_null_gradients_and_bit_identity():
    c = DC.build("b65_k130_c32")
    d = _dev(c)
    out_a, ga = _call(c, d)
    out_b, gb = _call(c, d)
    assert np.array_equal(out_a, out_b) and all(torch.equal(ga[g], gb[g]) for g in DC.GRADS)      # two calls agree to the bit
    assert all(bool((ga[g] != 3.0).any()) for g in DC.GRADS)
    _, twice = _call(c, d, accumulate=1, into={g: t.clone() for g, t in ga.items()})
    assert all(torch.equal(twice[g], 2 * ga[g]) for g in DC.GRADS)                   # x + x is exact: the same gradient was added
    for g in DC.GRADS:                                                               # one gradient not asked for: the others unchanged
        _, part = _call(c, d, skip=(g,))
        assert part[g] is None and all(torch.equal(part[o], ga[o]) for o in DC.GRADS if o != g), g
    _, pair = _call(c, d, skip=("g_f_img", "g_p_img", "g_P"))                        # a whole modality and the proxies
    assert torch.equal(pair["g_f_txt"], ga["g_f_txt"]) and torch.equal(pair["g_p_txt"], ga["g_p_txt"])


@pytest.mark.parametrize("where", ["code", "proxy"])
def test_nan_appears_where_the_float32_restatement_puts_it(where):
    c = dict(DC.build("b37_k16_c33"))
    key, at = ("f_txt", (3, 5)) if where == "code" else ("P", (2, 7))
    c[key] = c[key].copy()
    c[key][at] = np.nan
    r32 = DC.objective(c, torch.float32)
    got = _port(c)
    for k in r32:
        assert np.array_equal(np.isnan(got[k]), np.isnan(r32[k])), (where, k, int(np.isnan(got[k]).sum()), int(np.isnan(r32[k]).sum()))
    assert np.isnan(got["loss"][0]) and np.isnan(got["p_loss"][0]) and np.isfinite(got["d_loss_img"][0]) and np.isnan(got["g_P"]).all()
    assert np.isfinite(got["g_p_img"]).all() and np.isfinite(got["g_p_txt"]).all()
    if where == "code":
        assert np.isfinite(got["g_f_img"]).all() and np.isnan(got["g_f_txt"][3]).all() and np.isfinite(np.delete(got["g_f_txt"], 3, 0)).all()
    else:
        assert np.isnan(got["g_f_img"]).all() and np.isnan(got["g_f_txt"]).all()


@pytest.mark.parametrize("name", list(DC.GOLDEN_CASES))
def test_golden_cases_against_the_reference(name):
    """the reference's own float32 numbers: the port is within TOL_FACTOR e_ref of float64 and the golden within 24 eps32 of it
    (tests/test_dnph_cpu.py: 4 times the 5.9 eps32 measured there), so the two are within the sum of each other"""
    G = np.load(DC.GOLDEN)
    g = {k.split("__", 1)[1]: G[k] for k in G.files if k.startswith(name + "__")}
    c = dict(g, **DC.GOLDEN_CASES[name], labels=g["labels"].astype(np.int64), mrg=float(g["mrg"]), alpha=float(g["noise_alpha"]), up=1.0,
             noise_img=g["noise_img"].astype(np.float32), noise_txt=g["noise_txt"].astype(np.float32))
    r64, r32 = DC.objective(c, torch.float64, noise=False), DC.objective(c, torch.float32, noise=False)
    got = _port(c, noise=False)
    rows = [("loss", DC.rel_err(got["loss"], g["loss1"]), "loss")] + [(k, DC.rel_err(got[k], g[k]), k) for k in DC.GRADS]
    full = _port(c)
    rows += [("loss+noise", DC.rel_err(full["loss"], g["loss"]), "loss"), ("noise_img", DC.rel_err(full["noise_img"], g["noise_mean_img"]), "noise_img"),
             ("noise_txt", DC.rel_err(full["noise_txt"], g["noise_mean_txt"]), "noise_txt")]
    bounds = {k: 24 * EPS32 + DC.TOL_FACTOR * max(DC.pool()[DC.kind_of(k)], DC.rel_err(r32[k], r64[k])) for k in r64}
    for what, e, k in rows:
        print("%-6s %-11s e %.3e  bound %.3e" % (name, what, e, bounds[k]))
    for what, e, k in rows:
        assert e <= bounds[k], (name, what, e, bounds[k])
