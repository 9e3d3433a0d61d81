"""GPU, one process: the split entries of the DCMHT head's cross-rank BatchNorm (xmh_head_dcmht_train_forward_stats / _apply,
xmh_head_dcmht_backward_stats / _apply), called through ctypes with the statistics table stacked by hand.

One rank (the table is the rank's own row): bit-equal to the fused xmh_head_dcmht_train_forward / xmh_head_dcmht_backward -- the
probabilities, every section of the saved buffer, the running mean and variance, all nine gradients -- at B in {2, 3, 33},
E in {8, 40, 512}, N in {2, 32}.

Emulated ranks, W = 2 with shards of (1, 4) rows and W = 3 with (5, 1, 3): the statistics halves run per shard, the rows are stacked in
rank order, the apply halves run per shard, each with its own copy of the running statistics.  Against the float64 restatement
oracle.heads_train.dcmht_f64 of the CONCATENATED batch with the concatenated upstream gradient (BatchNorm over all rows; the scalar is
sum_r <d_probs_r, probs_r>): the probabilities, d_x, the parameter gradients added over the shards (in float64), under the rule of
tests/test_gpu_head_grad.py (`_tol`: TOL_FACTOR times the reference's own fp32 error of that tensor kind, the pool chosen by the
global batch size; relu near-ties evaluated with the forward's own mask); the running statistics, towards the global mean and the
unbiased variance over n_total, under that module's rtol 1e-5 / atol 1e-6.  rstd and the running statistics are bit-equal across the
shards.  A global batch of one row is XMH_EINVAL; one local row beside another rank's is legal (the first shard of W = 2).

Measured on an MI355X, error / tolerance: shards (1, 4) probs 2.7e-07 / 3.1e-06, g_x 4.3e-07 / 4.1e-06, g_w2 1.1e-06 / 3.8e-06 (the
closest), g_out_b (identically zero) 1.8e-07 / 4.0e-04; shards (5, 1, 3) all below 0.15 of their tolerance; running mean within
2.5e-08 and variance within 1.7e-07.  On the commit before this feature the module fails at the first call: the library has no
xmh_head_dcmht_stats_len."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import heads_train as T
from test_gpu_head_grad import DCMHT_KINDS, _tol

pytestmark = pytest.mark.gpu

EPS, MOMENTUM = 1e-5, 0.1
GRADS = ("d_wv", "d_bv", "d_wo", "d_bo", "d_norm_w", "d_norm_b", "d_w2", "d_b2", "d_x")


def _L():
    from xmh import _lib
    return _lib


def _a256(v):
    return (v + 255) & ~255


def _sections(saved, B, E, N):
    """the six sections of the saved buffer (include/xmh.h): v, nhat, n [B, E], rstd [E], f, p [B, N]"""
    be, bn = _a256(B * E * 4), _a256(B * N * 4)
    at = {"v": (0, B * E), "nhat": (be, B * E), "n": (2 * be, B * E), "rstd": (3 * be, E),
          "f": (3 * be + _a256(max(B, E) * 4), B * N), "p": (3 * be + _a256(max(B, E) * 4) + bn, B * N)}
    return {k: saved[o:o + 4 * n].view(torch.int32).clone() for k, (o, n) in at.items()}


def _device_params(P, E):
    """T.draw_dcmht's arrays as the ten device tensors of xmh_dcmht_train (the v third of in_proj)"""
    d = {"wv": P["in_w"][2 * E:], "bv": P["in_b"][2 * E:], "wo": P["out_w"], "bo": P["out_b"], "norm_w": P["norm_w"], "norm_b": P["norm_b"],
         "running_mean": P["running_mean"], "running_var": P["running_var"], "w2": P["w2"], "b2": P["b2"]}
    return {k: torch.tensor(np.ascontiguousarray(v)).cuda() for k, v in d.items()}


def _struct(D):
    L = _L()
    order = ("wv", "bv", "wo", "bo", "norm_w", "norm_b", "running_mean", "running_var", "w2", "b2")
    return L.DcmhtTrain(*[D[k].data_ptr() for k in order], 1, EPS, MOMENTUM)


class _Rank:
    """one (emulated) rank: its rows, its copy of the running statistics, its buffers"""

    def __init__(self, D, x, up):
        L = _L()
        self.D = dict(D, running_mean=D["running_mean"].clone(), running_var=D["running_var"].clone())
        self.h = _struct(self.D)
        self.x, self.up = torch.tensor(x).cuda().contiguous(), torch.tensor(up).cuda().contiguous()
        self.B, self.E = self.x.shape
        self.N = self.up.shape[1]
        nws = ctypes.c_size_t(0)
        self.nsaved = L.lib.xmh_head_dcmht_train_bytes(self.B, self.E, self.N, ctypes.byref(nws))
        self.nws = nws.value
        self.saved = torch.zeros(self.nsaved, dtype=torch.uint8, device="cuda")
        self.ws = torch.zeros(self.nws, dtype=torch.uint8, device="cuda")
        self.probs = torch.empty(self.B, self.N, device="cuda")
        self.row = torch.zeros(L.lib.xmh_head_dcmht_stats_len(self.E), dtype=torch.float64, device="cuda")
        shapes = dict(d_wv=(self.E, self.E), d_bv=(self.E,), d_wo=(self.E, self.E), d_bo=(self.E,), d_norm_w=(self.E,), d_norm_b=(self.E,),
                      d_w2=(self.N, self.E), d_b2=(self.N,), d_x=(self.B, self.E))
        self.g = {k: torch.full(shapes[k], 7.0, device="cuda") for k in GRADS}
        self.grads = L.DcmhtGrads(*[self.g[k].data_ptr() for k in GRADS])

    def _args(self):
        L = _L()
        return ctypes.byref(self.h), L.ptr(self.x)

    def fused(self):
        L = _L()
        h, x = self._args()
        L.check(L.lib.xmh_head_dcmht_train_forward(h, x, self.B, self.E, self.N, L.ptr(self.probs), L.ptr(self.saved), self.nsaved,
                                                   L.ptr(self.ws), self.nws, L.current_stream()), "forward")
        L.check(L.lib.xmh_head_dcmht_backward(h, x, L.ptr(self.up), self.B, self.E, self.N, L.ptr(self.saved), self.nsaved,
                                              ctypes.byref(self.grads), 0, L.ptr(self.ws), self.nws, L.current_stream()), "backward")

    def forward_stats(self):
        L = _L()
        h, x = self._args()
        L.check(L.lib.xmh_head_dcmht_train_forward_stats(h, x, self.B, self.E, self.N, L.ptr(self.saved), self.nsaved, L.ptr(self.ws), self.nws,
                                                         L.ptr(self.row), L.current_stream()), "forward_stats")
        return self.row.clone()

    def forward_apply(self, table):
        L = _L()
        h, x = self._args()
        return L.lib.xmh_head_dcmht_train_forward_apply(h, x, self.B, self.E, self.N, L.ptr(table), table.shape[0], L.ptr(self.probs),
                                                        L.ptr(self.saved), self.nsaved, L.ptr(self.ws), self.nws, L.current_stream())

    def backward_stats(self):
        L = _L()
        h, x = self._args()
        L.check(L.lib.xmh_head_dcmht_backward_stats(h, x, L.ptr(self.up), self.B, self.E, self.N, L.ptr(self.saved), self.nsaved,
                                                    ctypes.byref(self.grads), 0, L.ptr(self.ws), self.nws, L.ptr(self.row),
                                                    L.current_stream()), "backward_stats")
        return self.row.clone()

    def backward_apply(self, table, rank):
        L = _L()
        h, x = self._args()
        return L.lib.xmh_head_dcmht_backward_apply(h, x, self.B, self.E, self.N, L.ptr(table), table.shape[0], rank, L.ptr(self.saved),
                                                   self.nsaved, ctypes.byref(self.grads), 0, L.ptr(self.ws), self.nws, L.current_stream())


def _split_step(ranks):
    """stats per shard, the rows stacked in rank order, apply per shard: forward, then backward"""
    table = torch.stack([r.forward_stats() for r in ranks]).contiguous()
    for r in ranks:
        assert r.forward_apply(table) == 0, _L().lib.xmh_last_error()
    table = torch.stack([r.backward_stats() for r in ranks]).contiguous()
    for i, r in enumerate(ranks):
        assert r.backward_apply(table, i) == 0, _L().lib.xmh_last_error()
    torch.cuda.synchronize()


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("N", [2, 32])
@pytest.mark.parametrize("E", [8, 40, 512])
@pytest.mark.parametrize("B", [2, 3, 33])
def test_one_rank_is_the_fused_call_to_the_bit(B, E, N):
    P = T.draw_dcmht(900 + B + E + N, N // 2, True, e=E)
    x, up = T.draw_batch(901 + B + E + N, B, N, e=E)
    D = _device_params(P, E)
    a, b = _Rank(D, x, up), _Rank(D, x, up)
    a.fused()
    torch.cuda.synchronize()
    _split_step([b])
    assert float(b.row[2 * E]) == B and float(b.row[2 * E + 1]) == 0.0
    assert torch.equal(_bits(a.probs), _bits(b.probs))
    sa, sb = _sections(a.saved, B, E, N), _sections(b.saved, B, E, N)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), ("saved", k)
    for k in ("running_mean", "running_var"):
        assert torch.equal(_bits(a.D[k]), _bits(b.D[k])), k
        assert not torch.equal(a.D[k], D[k])                                             # they did move
    for k in GRADS:
        assert torch.equal(_bits(a.g[k]), _bits(b.g[k])), k
        assert not bool((a.g[k] == 7.0).all()), k                                        # and every gradient was written


@pytest.mark.parametrize("shards", [(1, 4), (5, 1, 3)])
def test_emulated_ranks_follow_float64_batchnorm_over_the_concatenated_batch(shards):
    G = T.golden()
    E, K = T.E, 16
    N, total = 2 * K, sum(shards)
    P = T.draw_dcmht(950 + total, K, True)
    x, up = T.draw_batch(951 + total, total, N)
    D = _device_params(P, E)
    cuts = np.cumsum((0,) + shards)
    ranks = [_Rank(D, x[lo:hi], up[lo:hi]) for lo, hi in zip(cuts[:-1], cuts[1:])]
    _split_step(ranks)
    secs = [_sections(r.saved, r.B, E, N) for r in ranks]
    for r, s in zip(ranks[1:], secs[1:]):                                                # one set of statistics on every rank
        assert torch.equal(s["rstd"], secs[0]["rstd"])
        assert torch.equal(_bits(r.D["running_mean"]), _bits(ranks[0].D["running_mean"]))
        assert torch.equal(_bits(r.D["running_var"]), _bits(ranks[0].D["running_var"]))
    # float64 over the whole batch, the relu near-ties with the forward's own mask (tests/test_gpu_head_grad.py::_oracle)
    R = T.dcmht_f64(x, P, True, up, eps=EPS)
    port = torch.cat([s["f"].view(torch.float32).reshape(r.B, N) for r, s in zip(ranks, secs)]).cpu().numpy() > 0
    differ = port != R["mask"]
    assert (np.abs(R["z"]) <= R["tie"])[differ].all() and differ.sum() <= T.TIE_CAP * differ.size
    if differ.any():
        R = T.dcmht_f64(x, P, True, up, eps=EPS, mask=np.where(differ, port, R["mask"]))
    add = lambda k: sum(r.g[k].double() for r in ranks).cpu().numpy()                    # noqa: E731
    got = {"probs": torch.cat([r.probs for r in ranks]).cpu().numpy(), "g_x": torch.cat([r.g["d_x"] for r in ranks]).cpu().numpy(),
           "g_in_w": np.concatenate([np.zeros((2 * E, E)), add("d_wv")]), "g_in_b": np.concatenate([np.zeros(2 * E), add("d_bv")]),
           "g_out_w": add("d_wo"), "g_out_b": add("d_bo"), "g_norm_w": add("d_norm_w"), "g_norm_b": add("d_norm_b"),
           "g_w2": add("d_w2"), "g_b2": add("d_b2")}
    report = [(kind, T.rel_err(got[kind], R[kind]), _tol(G, "dcmht", kind, mod="img", B=total)) for kind in DCMHT_KINDS]
    print("shards %s: " % (shards,) + " ".join("%s %.2e/%.2e" % r for r in report))        # every figure before any assertion
    want_mean = (1 - MOMENTUM) * P["running_mean"].astype(np.float64) + MOMENTUM * R["mean"]
    want_var = (1 - MOMENTUM) * P["running_var"].astype(np.float64) + MOMENTUM * R["var_unbiased"]
    got_mean, got_var = ranks[0].D["running_mean"].cpu().numpy(), ranks[0].D["running_var"].cpu().numpy()
    print("running mean err %.2e var err %.2e" % (np.abs(got_mean - want_mean).max(), np.abs(got_var - want_var).max()))
    for kind, e, tol in report:
        assert got[kind].shape == R[kind].shape and e <= tol, (shards, kind, e, tol)
    assert np.allclose(got_mean, want_mean, rtol=1e-5, atol=1e-6) and np.allclose(got_var, want_var, rtol=1e-5, atol=1e-6)
    # d_norm_w / d_norm_b are each rank's OWN sums (the reducer adds them like every other gradient): were they the global ones,
    # the sums over the shards above would be W times the float64 value
    assert not torch.equal(ranks[0].g["d_norm_b"], ranks[1].g["d_norm_b"])


def test_a_global_batch_of_one_row_is_refused_and_arguments_are_checked():
    L = _L()
    E, N = 8, 2
    P = T.draw_dcmht(990, 1, True, e=E)
    x, up = T.draw_batch(991, 1, N, e=E)
    r = _Rank(_device_params(P, E), x, up)
    table = r.forward_stats().reshape(1, -1).contiguous()
    torch.cuda.synchronize()
    assert r.forward_apply(table) == -22 and b"more than 1 row" in L.lib.xmh_last_error()
    assert r.backward_apply(table, 0) == -22
    two = torch.cat([table, table]).contiguous()
    assert r.backward_apply(two, 2) == -22                                               # rank outside the world
    assert L.lib.xmh_head_dcmht_stats_len(E) == 2 * E + 2 and L.lib.xmh_head_dcmht_stats_len(0) == 0
    r.h.norm_is_batchnorm = 0
    assert r.forward_apply(two) == -22 and b"LayerNorm" in L.lib.xmh_last_error()
