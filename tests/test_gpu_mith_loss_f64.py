"""GPU: MITH's training objective (xmh_mith_loss.hip behind MITH.object_function) against the float64 restatement of
tests/mith_loss_cases.py (validated against the reference's own numbers by tests/test_mith_loss_cases_cpu.py), where the older
tests/test_gpu_mith_loss.py does not look: likelihood chunks of one, two, three and 64 row tiles with short last chunks and tiles, a
chunk count the rounding leaves below its target, code widths 1, 3, 15, 65, 100, 129, 192 and 256 (k_mith_lik<true, 3> and <true, 4>, and
a last 64-column slice with a single live column), feature widths 1, 17, 33, 63, 65 and 2048, the limits B = 1024, K = 256, D = 2048 and
N = 2^22, trained-like codes with a fifth to a third of the dot products beyond the clamp, exact +-1 codes that land on +-64, +-62 and
+-66 in the first and last row of every chunk, unnormalised features, three weight vectors, non-finite inputs, a stale workspace,
gradient subsets, the accumulate flag and reproducibility at ragged K and D.

Tolerances.  Per kind (the ten terms as one vector, then each of the eight gradients), e = max|got - fp64| / max|fp64|.  The port must
stay within TOL_FACTOR * max(pool, e_ref): pool = the reference's own fp32 error over the six golden cases, e_ref = the float32
restatement against the float64 one at the case's own inputs (both computed here, neither hard-coded).  Factor 4 as in
tests/test_gpu_head_grad.py, tests/test_gpu_dcmht_loss.py and tests/test_gpu_hyp_loss_f64.py: a different but equally long summation
order may lose about twice the reference's bits at each of two chained reductions (the dot over K then the sum over N; the dot over D
then the softmax sum).  A gradient that vanishes identically in float64 must come back as exact zeros.  Every dot product of the
soft, trained and raw cases keeps MC.GAP from the clamp, so there is no allowance for a flipped mask anywhere.  Each figure is printed
before the first assertion; the conditions on the inputs are asserted again here before anything is compared."""
import ctypes

import numpy as np
import pytest
import torch

import mith_loss_cases as MC

pytestmark = pytest.mark.gpu

UPSTREAM = 3.0                       # the loss is scaled after the Function: the upstream gradient goes through the kernel


def _model(buf0, weights):
    """a MITH whose loss state is set by hand: the objective reads the weights and the buffer only, no backbone is needed"""
    from xmh.models.mith import MITH
    m = MITH.__new__(MITH)
    torch.nn.Module.__init__(m)
    for k in MC.WEIGHTS:
        setattr(m, k, float(weights[k]))
    m._bind_buffer(torch.as_tensor(buf0, dtype=torch.float32).clone())
    return m


class _Call:
    """the C ABI on one set of device tensors and one workspace"""

    def __init__(self, xs, Y, S, w):
        from xmh import _lib
        self.xs, self.Y, self.S = [t.cuda().contiguous() for t in xs], Y.cuda().contiguous(), S.cuda().contiguous()
        B, K = self.xs[2].shape
        self.a = _lib.MithLossArgs(Y.shape[0], B, K, self.xs[0].shape[1], *(t.data_ptr() for t in self.xs), self.Y.data_ptr(),
                                   self.S.data_ptr(), *(w[k] for k in MC.WEIGHTS), 0.07)
        self.ws = torch.empty(_lib.lib.xmh_mith_loss_ws_bytes(Y.shape[0], B, K, self.xs[0].shape[1]), dtype=torch.uint8, device="cuda")

    def forward(self):
        from xmh._lib import check, current_stream, lib, ptr
        out = torch.empty(10, dtype=torch.float64, device="cuda")
        check(lib.xmh_mith_loss(ctypes.byref(self.a), ptr(self.ws), self.ws.numel(), ptr(out), current_stream()), "xmh_mith_loss")
        return out

    def grad(self, which=range(8), upstream=None, into=None, accumulate=0, fill=None):
        """-> the eight gradient buffers; those not in `which` are not handed to the call"""
        from xmh._lib import check, current_stream, lib, ptr
        g = into if into is not None else [torch.empty_like(t) if fill is None else torch.full_like(t, fill) for t in self.xs]
        gp = (ctypes.c_void_p * 8)(*(g[i].data_ptr() if i in which else None for i in range(8)))
        check(lib.xmh_mith_loss_grad(ctypes.byref(self.a), ptr(upstream), gp, accumulate, ptr(self.ws), self.ws.numel(), current_stream()),
              "xmh_mith_loss_grad")
        return g


def _step(xs, Y, S, idx, w):
    """object_function on a buffer that the step's row write leaves equal to Y, backward of UPSTREAM * loss, and out10 of xmh_mith_loss
    on the same tensors -> dict(terms, g_<input>) as float64 numpy, gradients per unit of upstream"""
    m = _model(Y, w)
    dx = [t.cuda().requires_grad_(True) for t in xs]
    loss, _ = m.object_function(**dict(zip(MC.INPUTS, dx)), labels=None, indexs=idx, label_sim=S.cuda())
    assert loss.is_cuda and loss.dim() == 0 and loss.dtype == torch.float32 and loss.requires_grad
    assert np.array_equal(m.img_buffer_cls.cpu().numpy(), Y.numpy(), equal_nan=True)          # the write left the case's buffer
    (UPSTREAM * loss).backward()
    terms = _Call([t.detach() for t in dx], m.img_buffer_cls, S, w).forward().cpu().numpy()
    assert np.array_equal(np.float32(terms[0]), loss.detach().cpu().numpy(), equal_nan=True)   # the Function returns out10[0] as fp32
    assert all(x.grad.dtype == torch.float32 and x.grad.shape == t.shape for x, t in zip(dx, xs))
    return dict({"g_" + k: x.grad.cpu().double().numpy() / UPSTREAM for k, x in zip(MC.INPUTS, dx)}, terms=terms)


_steps = {}


def _case_step(name, wname="default"):
    if (name, wname) not in _steps:
        c = MC.build(name)
        _steps[name, wname] = _step(c["xs"], c["Y"], c["S"], c["idx"], MC.WSETS[wname])
    return _steps[name, wname]


# 1 the cases against float64 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,wname", MC.RUNS)
def test_cases_against_float64(name, wname):
    print(name, MC.describe(MC.check_conditions(name)))                                       # before anything is compared
    got = _case_step(name, wname)
    ref, r32 = MC.reference(name, wname), MC.reference(name, wname, torch.float32)
    MC.compare("%s %s" % (name, wname), got, ref, r32)


# 2 exact clamp edges -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in MC.CASES if MC.CASES[n]["family"] == "pm1"])
def test_exact_clamp_edges(name):
    """the code gradients restricted to the rows that sit at exactly +-64, +-62, +-66, 0 and +-K: the difference of a run with S = 1
    and one with S = 0 on those rows is -(0.5 / NB) sum over them of [|Y x| <= 64] Y[n], whatever sigma is, and the float64 mask is
    exact.  The same rule as everywhere: the differenced port against the differenced float64 within TOL_FACTOR * max(pool, e_ref),
    e_ref the differenced float32 restatement's error."""
    MC.check_conditions(name)
    c, w = MC.build(name), MC.DEFAULT
    runs = {}
    for v in (0.0, 1.0):
        S = MC.with_edge_S(c, v)
        runs[v] = (_step(c["xs"], c["Y"], S, c["idx"], w), MC.restate(c["xs"], c["Y"], S, w),
                   MC.restate(c["xs"], c["Y"], S, w, torch.float32))
    kinds = tuple("g_" + MC.INPUTS[i] for i in MC.CODES)
    got, ref, r32 = ({k: runs[1.0][j][k] - runs[0.0][j][k] for k in MC.KINDS} for j in range(3))
    for v in (0.0, 1.0):
        MC.compare("%s S[edge rows] = %g" % (name, v), *runs[v])
    for k in kinds:
        assert np.abs(ref[k]).max() > 0
    MC.compare("%s edge rows alone" % name, got, ref, r32, kinds=kinds)


# 3 non-finite parity -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MC.NONFINITE))
def test_nonfinite_inputs_pass_through(name):
    """fixed small tensors with one NaN, or one buffer row of inf: ordinary data to these kernels.  The buffer keeps such a row for the
    rest of the epoch, and the reference reports a NaN loss on every step that reads it."""
    xs, Y, S, idx = MC.build_nonfinite(name)
    got = _step(xs, Y, S, idx, MC.DEFAULT)
    ref, r32 = MC.restate(xs, Y, S, MC.DEFAULT), MC.restate(xs, Y, S, MC.DEFAULT, torch.float32)
    want = MC.recorded_pattern(name, ref)
    assert MC.same_pattern(MC.nan_pattern(ref), want) and MC.same_pattern(MC.nan_pattern(r32), want)
    print("%s (%s) NaN terms: port %s  recorded %s" % (name, MC.NONFINITE[name]["poke"],
                                                       [t for t, v in zip(MC.TERMS, got["terms"]) if np.isnan(v)], list(want[0])))
    for k in MC.KINDS[1:]:
        print("%s %-16s NaN entries: port %d  recorded %d of %d  inf entries: port %d" %
              (name, k, np.isnan(got[k]).sum(), want[1][k].sum(), want[1][k].size, np.isinf(got[k]).sum()))
    fin = dict({k: ~want[1][k] for k in MC.KINDS[1:]}, terms=np.array([t not in want[0] for t in MC.TERMS]))
    keep = lambda r: {k: np.asarray(r[k])[fin[k]] for k in MC.KINDS}                           # noqa: E731
    e_ref = {k: MC.rel_err(keep(r32)[k], keep(ref)[k]) if fin[k].any() else 0.0 for k in MC.KINDS}
    e = {k: MC.rel_err(np.nan_to_num(keep(got)[k], nan=np.inf), keep(ref)[k]) if fin[k].any() else 0.0 for k in MC.KINDS}
    yard = MC.yardstick(e_ref)
    for k in MC.KINDS:
        print("%s %-16s finite part (%d of %d): e_ref %.2e  yardstick %.2e  e_port %.2e  bound %.2e" %
              (name, k, fin[k].sum(), fin[k].size, e_ref[k], yard[k], e[k], MC.TOL_FACTOR * yard[k]))
    pattern = MC.nan_pattern(got)                         # also: no inf anywhere
    assert pattern[0] == want[0], (name, pattern[0], want[0])
    for k in MC.KINDS[1:]:
        assert np.array_equal(pattern[1][k], want[1][k]), (name, k, pattern[1][k])
    for k in MC.KINDS:
        assert e[k] <= MC.TOL_FACTOR * yard[k], (name, k, e[k], yard[k])


# 4 a stale workspace -----------------------------------------------------------------------------------------------------------
def test_gradient_and_forward_do_not_read_a_stale_workspace():
    """the gradient call alone, on a workspace full of 0xFF bytes (NaN as float and as double) and on a zeroed one, gives the bits it
    gives after a forward on the same workspace; likewise the forward"""
    c = MC.build("n130_b17_k65_d17")
    call = _Call(c["xs"], c["Y"], c["S"], MC.DEFAULT)
    call.ws.fill_(0xFF)
    g_ff = call.grad()
    call.ws.zero_()
    g_zero = call.grad()
    out_after_grad = call.forward()
    g_after_forward = call.grad()
    call.ws.fill_(0xFF)
    out_ff = call.forward()
    call.ws.zero_()
    out_zero = call.forward()
    assert all(bool(torch.isfinite(g).all()) and bool(g.abs().max() > 0) for g in g_ff) and bool(torch.isfinite(out_ff).all())
    for a, b, d in zip(g_ff, g_zero, g_after_forward):
        assert torch.equal(a, b) and torch.equal(a, d)
    assert torch.equal(out_ff, out_zero) and torch.equal(out_ff, out_after_grad)
    got = _case_step("n130_b17_k65_d17")
    assert np.array_equal(out_ff.cpu().numpy(), got["terms"])


# 5 gradient subsets ------------------------------------------------------------------------------------------------------------
def test_gradient_subsets_equal_the_full_call():
    c = MC.build("n130_b17_k65_d17")
    call = _Call(c["xs"], c["Y"], c["S"], MC.DEFAULT)
    full = call.grad()
    fill = 7.0
    for which in [(i,) for i in range(8)] + [MC.CODES, (0, 1, 6, 7)]:
        g = call.grad(which=which, fill=fill)
        for i in range(8):
            if i in which:
                assert torch.equal(g[i], full[i]), (which, i)
            else:
                assert bool((g[i] == fill).all()), (which, i)


# 6 accumulate and reproducibility at ragged K and D ----------------------------------------------------------------------------
def test_accumulate_and_two_calls_bit_identical_at_ragged_k_and_d():
    c = MC.build("n300_b20_k129_d65")
    call = _Call(c["xs"], c["Y"], c["S"], MC.DEFAULT)
    o1, g1 = call.forward(), call.grad()
    o2, g2 = call.forward(), call.grad()
    assert bool(torch.isfinite(o1).all()) and all(bool(g.abs().max() > 0) for g in g1)
    assert torch.equal(o1, o2) and all(torch.equal(a, b) for a, b in zip(g1, g2))
    up = torch.tensor([0.5], device="cuda")
    acc = call.grad(upstream=up, into=[torch.full_like(t, 3.0) for t in g1], accumulate=1)
    for a, b in zip(acc, g1):
        assert torch.allclose(a, 3.0 + 0.5 * b, rtol=1e-6, atol=1e-6)
