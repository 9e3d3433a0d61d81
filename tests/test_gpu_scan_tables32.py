"""The packed chunk-offset table between the two passes of the ranking scan (csrc/xmh_scan_kernels.h, k_scan_below): one
32-bit word per (chunk, bucket, query), all << 16 | relevant, where the pass 2 is k_scan_ap_c alone, and the path a shard takes when
one bucket of one query holds 65 536 items or more (the gate word: every block of pass 2 then sums its start values from pass 1's
counters).

Every case compares the per-query AP sums and divisors of RankingScan.histograms(False) + map_all(k) with oracle.retrieval in
float64, to the tolerance tests/test_gpu_retrieval.py uses for that comparison (rtol 2e-6, atol 1e-9; divisors bit for bit)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from test_gpu_retrieval import MAP_TOL, _u32

GATE_WIDE = 4                          # kGateWide: word of the control block


@pytest.fixture(scope="module")
def xr():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from xmh import retrieval
    return retrieval


def _describe(Q, R, K, C):
    from xmh import _lib
    buf = ctypes.create_string_buffer(512)
    assert _lib.lib.xmh_scan_describe(Q, R, K, C, 0, buf, 512) == 0
    return buf.value.decode()


def _host_packed(Q, R, K, C, mode=0):
    from xmh import _lib
    return int(_lib.lib.xmh_scan_tables_packed(Q, R, K, C, 0, mode))


def _gate_wide(scan):
    """the device's word after pass 1: 1 = a bucket total did not fit the packed table"""
    from xmh import _lib
    off = int(_lib.lib.xmh_scan_gate_offset(scan.q.n, scan.r.n, scan.q.K, 0))
    return int(scan.ws[off + 4 * GATE_WIDE: off + 4 * GATE_WIDE + 4].view(torch.int32).item())


def _check(xr, scan, k, want_ap, nrel):
    scan.histograms(False)
    m, ap, cap = scan.map_all(k)
    got = ap.cpu().numpy()
    want_cap = nrel if k is None else np.minimum(nrel, k)
    err = float((np.abs(got - want_ap) / np.maximum(np.abs(want_ap), 1e-30)).max())
    print("k=%s max rel err %.3g" % (k, err))
    assert np.array_equal(cap.cpu().numpy(), want_cap)
    assert np.allclose(got, want_ap, rtol=2e-6, atol=1e-9), err
    assert abs(float(m) - float(np.mean(want_ap / want_cap))) < MAP_TOL
    return m, ap, cap


# ---- 1. the packed path: several chunks, ragged ends ----------------------------------------------------------------------------------
SHAPE = (70, 5000)                     # a ragged query tile (70 = 64 + 6), a ragged last batch (5000 = 78 * 64 + 8)


@functools.lru_cache(maxsize=None)
def _random_case(K, C):
    from oracle import retrieval as orc
    from xmh import retrieval as xr
    Q, R = SHAPE
    gen = torch.Generator().manual_seed(7100 + K + C)
    qL = torch.rand(Q, C, generator=gen) < 0.05
    rL = torch.rand(R, C, generator=gen) < 0.05
    qL[:, 0] = True
    rL[::3, 0] = True
    qB = torch.randn(Q, K, generator=gen).sign()
    rB = torch.randn(R, K, generator=gen).sign()
    rB[R // 2:R // 2 + 300] = rB[:300]                                              # ties inside and across chunks
    q, r = xr.pack_sign(qB.cuda()), xr.pack_sign(rB.cuda())
    ql, rl = xr.pack_labels(qL.long().cuda()), xr.pack_labels(rL.long().cuda())
    dist = orc.hamming_packed(_u32(q.bits), _u32(r.bits))
    rel = orc.relevance_packed(_u32(ql), _u32(rl))
    want = {k: orc.ap_from_ranking(dist, rel, k=k) for k in (None, 50)}
    return q, ql, r, rl, want, rel.sum(-1)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [None, 50])
@pytest.mark.parametrize("K, C, packed", [(64, 80, 1), (16, 24, 1), (128, 80, 0)])
def test_packed_table_chunks_and_ragged_ends(xr, K, C, packed, k):
    """K = 128 runs k_scan_ap_c<., 8, true> with its stand-in behind it -- not k_scan_ap_c alone -- and so keeps the 64-bit table."""
    Q, R = SHAPE
    q, ql, r, rl, want, nrel = _random_case(K, C)
    assert "pass2=k_scan_ap_c<" in _describe(Q, R, K, C) and "|" not in _describe(Q, R, K, C)
    assert _host_packed(Q, R, K, C) == packed
    scan = xr.RankingScan(q, ql, r, rl, C)
    assert scan.plan.nchunk > 1 and R % scan.plan.chunk != 0
    _check(xr, scan, k, want[k], nrel)
    assert _gate_wide(scan) == 0


# ---- 2. the edge of 16 bits -----------------------------------------------------------------------------------------------------------
def _one_code_case(xr, Q, R, K, every):
    """R copies of one code; item i is relevant when i % every == 0.  Every pair of a query has one distance, so a bucket total is R."""
    gen = torch.Generator().manual_seed(65535)
    qB = torch.randn(Q, K, generator=gen).sign()
    rB = torch.randn(1, K, generator=gen).sign().repeat(R, 1)
    qL = torch.zeros(Q, 8, dtype=torch.long)
    qL[:, 0] = 1
    rL = torch.zeros(R, 8, dtype=torch.long)
    rL[:, 1] = 1                                                                    # a class no query has
    rL[::every, 0] = 1
    return qB, rB, qL, rL


@pytest.mark.gpu
@pytest.mark.parametrize("every", [1, 100])
@pytest.mark.parametrize("R, fallback", [(65535, 0), (65536, 1), (70000, 1)])
def test_edge_of_16_bits(xr, R, fallback, every):
    from oracle import retrieval as orc
    Q, K, C = 16, 64, 8
    qB, rB, qL, rL = _one_code_case(xr, Q, R, K, every)
    q, r = xr.pack_sign(qB.cuda()), xr.pack_sign(rB.cuda())
    ql, rl = xr.pack_labels(qL.cuda()), xr.pack_labels(rL.cuda())
    assert _describe(Q, R, K, C).endswith("pass2=k_scan_ap_c<false, 8, false>") and _host_packed(Q, R, K, C) == 1
    dist = orc.hamming_packed(_u32(q.bits), _u32(r.bits))
    rel = orc.relevance_packed(_u32(ql), _u32(rl))
    want = orc.ap_from_ranking(dist, rel)
    # closed form: the ranking is the gallery order, item i has rank i + 1 and, if relevant, ordinal i / every + 1
    j = np.arange((R + every - 1) // every, dtype=np.float64)
    closed = float(((j + 1) / (every * j + 1)).sum())
    assert every != 1 or closed == R
    assert np.allclose(want, closed, rtol=1e-12)
    scan = xr.RankingScan(q, ql, r, rl, C)
    assert scan.plan.nchunk > 1
    _check(xr, scan, None, want, rel.sum(-1))
    assert _gate_wide(scan) == fallback, (R, _gate_wide(scan))


# ---- 3. one query only is too wide ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_fallback_for_one_query_only(xr):
    from oracle import retrieval as orc
    Q, R, K, C = 32, 70000, 16, 24
    gen = torch.Generator().manual_seed(316)
    rB = torch.randn(1, K, generator=gen).sign().repeat(R, 1)
    qB = torch.randn(Q, K, generator=gen).sign()
    qB[0] = rB[0]                                                                   # 70 000 items at distance 0 for query 0
    qL = torch.rand(Q, C, generator=gen) < 0.1
    rL = torch.rand(R, C, generator=gen) < 0.05
    qL[:, 0] = True
    rL[::7, 0] = True
    q, r = xr.pack_sign(qB.cuda()), xr.pack_sign(rB.cuda())
    ql, rl = xr.pack_labels(qL.long().cuda()), xr.pack_labels(rL.long().cuda())
    assert _describe(Q, R, K, C).endswith("pass2=k_scan_ap_c<false, 8, false>") and _host_packed(Q, R, K, C) == 1
    dist = orc.hamming_packed(_u32(q.bits), _u32(r.bits))
    rel = orc.relevance_packed(_u32(ql), _u32(rl))
    assert (dist[0] == 0).all()
    scan = xr.RankingScan(q, ql, r, rl, C)
    for k in (None, 50):
        _check(xr, scan, k, orc.ap_from_ranking(dist, rel, k=k), rel.sum(-1))
    assert _gate_wide(scan) == 1


# ---- 4. the sharded entry points keep the 64-bit table --------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("told", [True, False])
@pytest.mark.parametrize("k", [None, 50])
def test_sharded_entry_points_unchanged(xr, k, told):
    """a one-shard "world".  told: pass 1 knows that a sharded pass 2 follows (what sharded.HipShardOps does) and leaves the 64-bit table.
    Not told, it leaves the packed one and the sharded pass 2 writes the 64-bit table again first.  Either way the same arithmetic on
    the same table as before: the sums of map_all, to the bit."""
    K, C = 64, 80
    Q, R = SHAPE
    q, ql, r, rl, want, nrel = _random_case(K, C)
    assert _host_packed(Q, R, K, C, 0) == 1 and [_host_packed(Q, R, K, C, m) for m in (1, 2, 3)] == [0, 0, 0]
    scan = xr.RankingScan(q, ql, r, rl, C)
    m0, ap0, cap0 = _check(xr, scan, k, want[k], nrel)
    hint = {"sharded": True} if told else {}
    scan.histograms(False, **hint)
    t = scan.totals().clone()                                                       # [nb, qpad, 2]
    m1, ap1, cap1 = scan.map_sharded(k, t.unsqueeze(0).contiguous(), 0)
    assert torch.equal(ap1, ap0) and torch.equal(cap1, cap0) and torch.equal(m1, m0)
    scan.histograms(False, **hint)
    nb, qpad = t.shape[0], t.shape[1]
    offs = xr.slice_offsets(t.view(nb, 1, qpad, 2).permute(1, 0, 2, 3).contiguous())
    m2, ap2, cap2 = scan.map_sharded_offsets(k, offs)
    assert torch.equal(ap2, ap0) and torch.equal(cap2, cap0) and torch.equal(m2, m0)
    # the workspace holds the 64-bit table now: an unsharded pass 2 without a fresh pass 1 reads that form
    m3, ap3, cap3 = scan.map_all(k)
    assert torch.equal(ap3, ap0) and torch.equal(cap3, cap0) and torch.equal(m3, m0)
    _check(xr, scan, k, want[k], nrel)
