"""GPU: DSPH's HyP loss and its gradient kernels (xmh_hyp.hip behind HyPProxies.forward / DSPH.object_function) against the float64
restatement of tests/hyp_loss_cases.py (validated against the reference's own numbers by tests/test_hyp_loss_cases_cpu.py), where the
older tests/test_gpu_hyp_loss.py does not look: code widths that are no multiple of the 64 lanes or the 256 threads (K = 1, 63, 65, 100,
257, and the limit 4096), batches that end one row, 44 rows and one row into a 256-row partner chunk, label words with bit 31 set and
with a class alone in its word, rows without a label, rows and a proxy clamped by F.normalize's eps, a threshold at which no hinge is
active, non-finite inputs, reproducibility and the accumulate flag at those edges.

Tolerances.  Per kind (the eight terms as one vector, d loss / d x, d loss / d y, d loss / d P), e = max|got - fp64| / max|fp64|, rows
clamped by eps measured as a group of their own.  The port must stay within TOL_FACTOR * max(pool, e_ref): pool = the reference's own fp32
error over the seven golden cases, e_ref = the float32 restatement against the float64 one at the case's own inputs (both computed here,
neither hard-coded).  Factor 4 as in tests/test_gpu_head_grad.py and tests/test_gpu_dcmht_loss.py: a different but equally long
summation order may lose about twice the reference's bits at each of two chained reductions (here the sum over the code width inside a
cosine, then the sum over proxies or partners).  Every mask entry of every case keeps HC.GAP from the threshold, so there is no
allowance for a flipped relu' anywhere.  Each figure is printed before the first assertion; the conditions on the inputs are asserted
again here before anything is compared."""
import numpy as np
import pytest
import torch

import hyp_loss_cases as HC

pytestmark = pytest.mark.gpu

TOL_FACTOR = 4.0
UPSTREAM = 3.0                       # the loss is scaled after the Function: the upstream gradient goes through the kernel


def _model(K, C, threshold, alpha, proxies):
    from xmh.models.dsph import DSPH, HyPProxies
    m = DSPH.__new__(DSPH)                                     # the loss reads the hyp module only; no backbone needed here
    torch.nn.Module.__init__(m)
    m.hyp = HyPProxies(numclass=C, output_dim=K, alpha=alpha, threshold=threshold)
    with torch.no_grad():
        m.hyp.proxies.copy_(torch.as_tensor(proxies))
    return m.cuda()


def _raw(x, y, P, labels, threshold, alpha, upstream=None, grads=None, accumulate=0):
    """out8 (float64 [8]) and (gx, gy, gP) straight from the C ABI"""
    from xmh import retrieval as R
    from xmh._lib import check, current_stream, lib, ptr
    B, K = x.shape
    C = P.shape[0]
    lab = R.pack_labels(labels)
    ws = torch.empty(lib.xmh_hyp_loss_ws_bytes(B, K, C), dtype=torch.uint8, device="cuda")
    out = torch.empty(8, dtype=torch.float64, device="cuda")
    args = (ptr(x), ptr(y), ptr(P), B, K, C, ptr(lab), float(threshold), float(alpha))
    check(lib.xmh_hyp_loss(*args, ptr(ws), ws.numel(), ptr(out), current_stream()), "xmh_hyp_loss")
    g = grads if grads is not None else (torch.empty_like(x), torch.empty_like(y), torch.empty_like(P))
    check(lib.xmh_hyp_loss_grad(*args, ptr(upstream), *(ptr(t) for t in g), accumulate, ptr(ws), ws.numel(), current_stream()),
          "xmh_hyp_loss_grad")
    return out, g


def _step(x, y, P, labels, thr, alpha):
    """object_function + backward of UPSTREAM * loss, and out8 of xmh_hyp_loss on the same tensors -> dict(terms, g_x, g_y, g_P) as
    float64 numpy, gradients per unit of upstream"""
    B, K = x.shape
    m = _model(K, P.shape[0], thr, alpha, P)
    dx, dy, dl = x.cuda().requires_grad_(True), y.cuda().requires_grad_(True), labels.cuda()
    loss, d = m.object_function(dx, dy, labels=dl)
    assert loss.is_cuda and loss.dim() == 0 and loss.requires_grad
    (UPSTREAM * loss).backward()
    out8, _ = _raw(dx.detach(), dy.detach(), m.hyp.proxies.detach(), dl, thr, alpha)
    terms = out8.cpu().numpy()
    assert np.array_equal(np.float32(terms[0]), loss.detach().cpu().numpy(), equal_nan=True)     # the Function returns out8[0] as fp32
    grads = (dx.grad, dy.grad, m.hyp.proxies.grad)
    assert all(g.dtype == torch.float32 and g.shape == t.shape for g, t in zip(grads, (x, y, P)))
    return dict({k: g.cpu().double().numpy() / UPSTREAM for k, g in zip(HC.KINDS[1:], grads)}, terms=terms)


def _compare(what, got, ref, r32, clamped, floor=None):
    """prints e_ref, the yardstick, the port's error, their ratio and the bound per kind, then asserts e_port <= TOL_FACTOR * yardstick"""
    e_ref = HC.errors(r32, ref, clamped, floor)
    yard, e = HC.yardstick(e_ref), HC.errors(got, ref, clamped, floor)
    for k in HC.KINDS:
        print("%s %-5s e_ref %.2e  yardstick %.2e  e_port %.2e  e_port/e_ref %.2f  bound %.2e" %
              (what, k, e_ref[k], yard[k], e[k], e[k] / e_ref[k] if e_ref[k] else float("inf"), TOL_FACTOR * yard[k]))
    for k in HC.KINDS:
        assert np.isfinite(got[k]).all(), (what, k)
        assert e[k] <= TOL_FACTOR * yard[k], (what, k, e[k], yard[k])


# 1 the cases against float64 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(HC.CASES))
def test_cases_against_float64(name):
    c = HC.build(name)
    print(name, "redrawn %d" % c["redrawn"], HC.describe(HC.check_conditions(name)))          # before anything is compared
    x, y, P, L, thr = c["x"], c["y"], c["P"], c["labels"], c["thr"]
    got = _step(x, y, P, L, thr, HC.ALPHA)
    ref = HC.restate(x, y, P, L, thr, HC.ALPHA)
    r32 = HC.restate(x, y, P, L, thr, HC.ALPHA, dtype=torch.float32)
    _compare(name, got, ref, r32, HC.clamped_rows(x, y, P), c["floor"])
    if c["share"] == "none":                              # nothing passes the hinge: exact zeros, not small numbers
        t = got["terms"]
        print(name, "terms", t)
        assert t[2] == t[4] == t[5] == t[6] == t[7] == 0.0 and t[1] > 0 and t[3] > 0
        unused = ~(L != 0).any(0).numpy()
        assert unused.any() and (got["g_P"][unused] == 0.0).all() and np.abs(got["g_P"][~unused]).max() > 0


# 3 non-finite parity -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(HC.NONFINITE))
def test_nonfinite_inputs_pass_through(name):
    """fixed 6 x 4 tensors with one NaN or one row of inf: ordinary data to these kernels"""
    x, y, P, L, thr, alpha = HC.build_nonfinite(name)
    spec = HC.NONFINITE[name]
    got = _step(x, y, P, L, thr, alpha)
    ref = HC.restate(x, y, P, L, thr, alpha)
    r32 = HC.restate(x, y, P, L, thr, alpha, dtype=torch.float32)
    want_terms, want_rows = tuple(spec["nan_terms"]), {k: tuple(spec[k]) for k in HC.KINDS[1:]}
    assert HC.nan_pattern(ref) == HC.nan_pattern(r32) == (want_terms, want_rows)
    print("%s NaN terms: port %s  recorded %s" % (name, [t for t, v in zip(HC.TERMS, got["terms"]) if np.isnan(v)], list(want_terms)))
    for k in HC.KINDS[1:]:
        print("%s %s NaN entries per row: port %s  recorded rows %s" % (name, k, np.isnan(got[k]).sum(1).tolist(), list(want_rows[k])))
    fin = {"terms": ~np.isnan(ref["terms"])}
    fin.update({k: ~np.isnan(ref[k]).all(1) for k in HC.KINDS[1:]})
    keep = lambda r: {k: np.asarray(r[k])[fin[k]] for k in HC.KINDS}                         # noqa: E731
    e_ref = {k: HC.rel_err(keep(r32)[k], keep(ref)[k]) if fin[k].any() else 0.0 for k in HC.KINDS}
    e = {k: HC.rel_err(np.nan_to_num(keep(got)[k], nan=np.inf), keep(ref)[k]) if fin[k].any() else 0.0 for k in HC.KINDS}
    yard = HC.yardstick(e_ref)
    for k in HC.KINDS:
        print("%s %-5s finite part (%d of %d): e_ref %.2e  yardstick %.2e  e_port %.2e  bound %.2e" %
              (name, k, fin[k].sum(), fin[k].size, e_ref[k], yard[k], e[k], TOL_FACTOR * yard[k]))
    got_terms, got_rows = HC.nan_pattern(got)             # also: no inf, and a gradient row is NaN throughout or not at all
    assert got_terms == want_terms, (name, got_terms, want_terms)
    for k in HC.KINDS[1:]:
        assert got_rows[k] == want_rows[k], (name, k, got_rows[k], want_rows[k])
    for k in HC.KINDS:
        assert e[k] <= TOL_FACTOR * yard[k], (name, k, e[k], yard[k])


# 4 reproducibility at chunk edges ----------------------------------------------------------------------------------------------
def test_two_calls_bit_identical_at_chunk_edges():
    c = HC.build("b300_k65_c33")
    x, y, P, L = (c[k].cuda() for k in ("x", "y", "P", "labels"))
    o1, g1 = _raw(x, y, P, L, c["thr"], HC.ALPHA)
    o2, g2 = _raw(x, y, P, L, c["thr"], HC.ALPHA)
    assert bool(torch.isfinite(o1).all()) and all(bool(g.abs().max() > 0) for g in g1)
    assert torch.equal(o1, o2) and all(torch.equal(a, b) for a, b in zip(g1, g2))


# 5 the accumulate flag at a ragged width ---------------------------------------------------------------------------------------
def test_accumulate_at_ragged_k():
    g = torch.Generator().manual_seed(HC.SEED + 5)
    B, K, C = 257, 65, 21
    base = torch.randn(K, generator=g)
    x, y, P = HC._code_rows(g, B, base).cuda(), HC._code_rows(g, B, base).cuda(), HC._proxies(g, C, base).cuda()
    labels = HC._labels(g, B, C, 0.08, {256: (3, 17)}).cuda()
    _, g1 = _raw(x, y, P, labels, 0.0, HC.ALPHA)
    filled = tuple(torch.full_like(t, 3.0) for t in g1)
    up = torch.tensor([0.5], device="cuda")
    _, g2 = _raw(x, y, P, labels, 0.0, HC.ALPHA, upstream=up, grads=tuple(t.clone() for t in filled), accumulate=1)
    for a, b, f in zip(g2, g1, filled):
        assert bool(b.abs().max() > 0) and torch.allclose(a, f + 0.5 * b, rtol=1e-6, atol=1e-6)
