"""Round 11 of the ranking scan: on the packed-table route k_scan_below runs without its tail, and every block of
k_scan_ap_c prefixes the totals of its query tile over the buckets in registers, takes the cap from the row sum, and the blocks of chunk 0
store the relevant counts for the reduce launch.

The same inputs go two ways through the same library: the new route, histograms(False) -> map_all(k), and a route that still runs the
table kernels in full, histograms(False, sharded=True) -> map_all(k) (64-bit table, dpre and the relevant counts by k_scan_below).
Everything is compared BIT FOR BIT -- ap_sum and map as float64 bit patterns, cap as integers: the start value of every counter is an
integer sum, so a difference of rounding order is a failure here, not a tolerance.  One comparison per shape also goes to the oracle
(oracle.retrieval.map_k; the per-query sums to ap_from_ranking), at the tolerance of tests/test_gpu_scan_tables32.py.  map_k keeps
the reference's IndexError for Q == 1 and squeezes R == 1 away: those shapes are checked through ap_from_ranking only."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from test_gpu_retrieval import MAP_TOL, _u32

GATE_WIDE = 4


@pytest.fixture(scope="module")
def xr():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from xmh import retrieval
    return retrieval


def _lib():
    from xmh import _lib
    return _lib.lib


def _describe(Q, R, K, C):
    buf = ctypes.create_string_buffer(512)
    assert _lib().xmh_scan_describe(Q, R, K, C, 0, buf, 512) == 0
    return buf.value.decode()


def _packed_route(Q, R, K, C):
    """the unsharded step of this shape is k_scan_ap_c<., 8, false> alone on the packed table: the route this file is about"""
    return _describe(Q, R, K, C).endswith("pass2=k_scan_ap_c<false, 8, false>") and int(_lib().xmh_scan_tables_packed(Q, R, K, C, 0, 0)) == 1


def _gate_words(scan, first, n):
    off = int(_lib().xmh_scan_gate_offset(scan.q.n, scan.r.n, scan.q.K, 0))
    return scan.ws[off + 4 * first: off + 4 * (first + n)].view(torch.int32).cpu().numpy()


def _bits(t):
    return t.contiguous().view(torch.int64).cpu().numpy()


def _same(a, b):
    """(map, ap_sum, cap) of two evaluations, bit for bit"""
    return np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1])) and torch.equal(a[2], b[2])


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(Q, R, K, C, empty):
    """random codes with ties inside and across chunks, multi-hot labels; `empty`: query 1 has no relevant item.  Packed operands on
    the device, the float codes and labels for the oracle."""
    from xmh import retrieval as xr
    gen = torch.Generator().manual_seed(1100 + 7 * Q + R + 31 * K + C)
    qL = torch.rand(Q, C, generator=gen) < 0.05
    rL = torch.rand(R, C, generator=gen) < 0.05
    qL[:, 0] = True
    rL[::3, 0] = True
    rL[:, C - 1] = False
    if empty:
        qL[1] = False
        qL[1, C - 1] = True                                                         # a class no item has
    qB = torch.randn(Q, K, generator=gen).sign()
    rB = torch.randn(R, K, generator=gen).sign()
    if R >= 600:
        rB[R // 2:R // 2 + 300] = rB[:300]
    q, r = xr.pack_sign(qB.cuda()), xr.pack_sign(rB.cuda())
    ql, rl = xr.pack_labels(qL.long().cuda()), xr.pack_labels(rL.long().cuda())
    return q, ql, r, rl, (qB, rB, qL.long(), rL.long())


def _new_route(xr, ops, C, k):
    scan = xr.RankingScan(*ops, C)
    scan.histograms(False)
    return scan.map_all(k), scan


def _full_tables(xr, ops, C, k):
    scan = xr.RankingScan(*ops, C)
    scan.histograms(False, sharded=True)
    return scan.map_all(k), scan


def _oracle_check(got, ops, host, k):
    from oracle import retrieval as orc
    q, ql, r, rl = ops
    qB, rB, qL, rL = host
    m, ap, cap = got
    dist = orc.hamming_packed(_u32(q.bits), _u32(r.bits))
    rel = orc.relevance_packed(_u32(ql), _u32(rl))
    want_ap = orc.ap_from_ranking(dist, rel, k=k)
    nrel = rel.sum(-1)
    want_cap = nrel if k is None else np.minimum(nrel, k)
    a = ap.cpu().numpy()
    err = float((np.abs(a - want_ap) / np.maximum(np.abs(want_ap), 1e-30)).max())
    print("k=%s max rel err of ap_sum %.3g" % (k, err))
    assert np.array_equal(cap.cpu().numpy(), want_cap)
    assert np.allclose(a, want_ap, rtol=2e-6, atol=1e-9), err
    if qB.shape[0] > 1 and rB.shape[0] > 1:
        want = float(orc.map_k(qB, rB, qL, rL, k, stable=True))
        print("map %.9g oracle %.9g" % (float(m), want))
        assert (np.isnan(want) and np.isnan(float(m))) or abs(float(m) - want) < MAP_TOL
    return nrel


# ---- 1. shapes: bucket rows, label tiles, query tiles, ragged batches, chunks ----------------------------------------------------------
# (Q, R, K, C, empty query).  K 16 / 33 / 64: 17 rows (fewer than four parts of eight), 34, 65.  C 24 / 80: the i8 and the FP4 label tile.
# Q: one query, a partly filled 16-query tile (15, 17), a whole one, a partly filled 64-query tile (70), two pass-1 blocks (257).
# R: one item, a ragged / whole / one-past batch (63, 64, 65), one chunk of 256 nearly full, 12 chunks, 20 chunks (k_scan_below's second
# group of 16) with a ragged last one.
SHAPES = [
    (1, 1, 64, 80, False), (15, 63, 16, 24, True), (16, 64, 33, 80, False), (17, 65, 64, 24, False), (70, 200, 64, 80, True),
    (257, 3000, 64, 80, False), (70, 3000, 16, 24, False), (17, 5000, 33, 24, False), (70, 5000, 64, 80, True), (257, 5000, 16, 80, False),
    (1, 5000, 64, 24, False), (16, 1, 16, 80, True),
]


@pytest.mark.gpu
@pytest.mark.parametrize("Q, R, K, C, empty", SHAPES)
def test_new_route_equals_full_tables(xr, Q, R, K, C, empty):
    """k None (k_scan_ap_c<false, ...>) and a k below many queries' relevant counts (the CAPPED instance: capf from the in-block sum)"""
    assert _packed_route(Q, R, K, C)
    q, ql, r, rl, host = _case(Q, R, K, C, empty)
    ops = (q, ql, r, rl)
    for k in (None, 3):
        got, scan = _new_route(xr, ops, C, k)
        ref, _ = _full_tables(xr, ops, C, k)
        assert _same(got, ref), (k, float(got[0]), float(ref[0]))
        assert int(_gate_words(scan, GATE_WIDE, 1)[0]) == 0
        if k is None:
            nrel = _oracle_check(got, ops, host, None)
            assert not empty or (nrel[1] == 0 and int(got[2][1]) == 0 and _bits(got[1])[1] == 0)      # divisor 0, ap_sum +0
        else:
            assert R < 20 or int((got[2] == 3).sum()) > 0
    if R >= 3000:
        _oracle_check(got, ops, host, 3)


@pytest.mark.gpu
def test_new_route_runs_no_tail(xr):
    """k_scan_below of the new route draws no ticket; the full form draws one per block of a 64-query tile (17 bucket rows: 5 blocks)"""
    Q, R, K, C = 70, 3000, 16, 24
    ops = _case(Q, R, K, C, True)[:4]
    _, scan = _new_route(xr, ops, C, None)
    nqt = scan.plan.nqtile
    assert nqt * 4 <= 256
    assert not _gate_words(scan, -64, nqt).any()                                    # the ticket words end where the gate words start
    _, scan = _full_tables(xr, ops, C, None)
    assert (_gate_words(scan, -64, nqt) == 5).all()


# ---- 2. the kGateWide fallback with the in-block prefix -------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("R", [65536, 70000])
def test_wide_fallback_for_one_query(xr, R):
    """one query of 32 has R items at distance 0 (tests/test_gpu_scan_tables32.py): the packed table does not hold, every block sums its
    start values from pass 1's counters and adds the in-block prefix"""
    from oracle import retrieval as orc
    Q, K, C = 32, 16, 24
    gen = torch.Generator().manual_seed(316)
    rB = torch.randn(1, K, generator=gen).sign().repeat(R, 1)
    qB = torch.randn(Q, K, generator=gen).sign()
    qB[0] = rB[0]
    qL = torch.rand(Q, C, generator=gen) < 0.1
    rL = torch.rand(R, C, generator=gen) < 0.05
    qL[:, 0] = True
    rL[::7, 0] = True
    ops = (xr.pack_sign(qB.cuda()), xr.pack_labels(qL.long().cuda()), xr.pack_sign(rB.cuda()), xr.pack_labels(rL.long().cuda()))
    assert _packed_route(Q, R, K, C)
    dist = orc.hamming_packed(_u32(ops[0].bits), _u32(ops[2].bits))
    rel = orc.relevance_packed(_u32(ops[1]), _u32(ops[3]))
    for k in (None, 50):
        got, scan = _new_route(xr, ops, C, k)
        assert int(_gate_words(scan, GATE_WIDE, 1)[0]) == 1
        ref, _ = _full_tables(xr, ops, C, k)
        assert _same(got, ref)
        want = orc.ap_from_ranking(dist, rel, k=k)
        nrel = rel.sum(-1)
        assert np.array_equal(got[2].cpu().numpy(), nrel if k is None else np.minimum(nrel, k))
        assert np.allclose(got[1].cpu().numpy(), want, rtol=2e-6, atol=1e-9)


# ---- 3. sequences on one workspace ----------------------------------------------------------------------------------------------------
SEQ = (70, 5000, 64, 80)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [None, 3])
def test_pass_2_again_on_one_workspace(xr, k):
    Q, R, K, C = SEQ
    ops = _case(Q, R, K, C, True)[:4]
    ref, _ = _full_tables(xr, ops, C, k)
    ref_all, _ = _full_tables(xr, ops, C, None)
    scan = xr.RankingScan(*ops, C)
    scan.histograms(False)
    assert _same(scan.map_all(k), ref)
    assert _same(scan.map_all(k), ref)
    scan.histograms(False)
    ap, cap = scan.ap_sums(k)
    assert np.array_equal(_bits(ap), _bits(ref[1])) and torch.equal(cap, ref[2])
    assert _same(scan.map_all(None), ref_all)
    assert _same(scan.map_all(k), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [None, 3])
def test_other_pass_2_behind_a_pass_1_that_left_no_tail(xr, k):
    """ap_sums with the caller's offsets, map_sharded and map_sharded_offsets behind histograms(False): the host runs the table kernels in
    full first.  Compared with the same calls on a fresh workspace whose pass 1 was told (a one-shard world)."""
    Q, R, K, C = SEQ
    ops = _case(Q, R, K, C, True)[:4]
    told = xr.RankingScan(*ops, C)
    pair = torch.stack(told.histograms(True)).unsqueeze(0).contiguous()             # [1, 2, Q, nb]
    offs = xr.shard_offsets(pair, 0)
    ref_ap = told.ap_sums(k, *offs)
    told.histograms(False, sharded=True)
    t = told.totals().clone()
    ref_sh = told.map_sharded(k, t.unsqueeze(0).contiguous(), 0)
    told.histograms(False, sharded=True)
    nb, qpad = t.shape[0], t.shape[1]
    so = xr.slice_offsets(t.view(nb, 1, qpad, 2).permute(1, 0, 2, 3).contiguous())
    ref_so = told.map_sharded_offsets(k, so)
    ref_all, _ = _full_tables(xr, ops, C, k)

    scan = xr.RankingScan(*ops, C)
    scan.histograms(False)
    ap, cap = scan.ap_sums(k, *offs)
    assert np.array_equal(_bits(ap), _bits(ref_ap[0])) and torch.equal(cap, ref_ap[1])
    assert _same(scan.map_all(k), ref_all)                                         # the workspace holds the 64-bit table and its tail now
    scan.histograms(False)
    assert torch.equal(scan.totals(), t)
    assert _same(scan.map_sharded(k, t.unsqueeze(0).contiguous(), 0), ref_sh)
    scan.histograms(False)
    assert _same(scan.map_sharded_offsets(k, so), ref_so)
    scan.histograms(False)
    assert _same(scan.map_all(k), ref_all)


@pytest.mark.gpu
def test_histogram_export_on_the_packed_route_keeps_the_tail(xr):
    Q, R, K, C = SEQ
    ops = _case(Q, R, K, C, True)[:4]
    a = xr.RankingScan(*ops, C)
    ha, hr = a.histograms(True, sharded=False)
    b = xr.RankingScan(*ops, C)
    hb, hs = b.histograms(True, sharded=True)
    assert torch.equal(ha, hb) and torch.equal(hr, hs)
    assert int(ha.sum()) == Q * R
    assert (_gate_words(a, -64, a.plan.nqtile) == (K + 1 + 3) // 4).all()            # the tail ran: one ticket per block of a tile
    for k in (None, 3):
        assert _same(a.map_all(k), b.map_all(k))


@pytest.mark.gpu
@pytest.mark.parametrize("first", [64, 128])
def test_128_and_64_bit_calls_alternate_on_one_workspace(xr, first):
    """the table form the host remembers goes with the workspace, and what one call leaves in the control words (the 128-bit one raises
    kGateWrapped here, an item at distance 128) must not reach the next"""
    Q, R, C = 32, 3000, 80
    ops, fresh, plans = {}, {}, {}
    for K in (64, 128):
        q, ql, r, rl, host = _case(Q, R, K, C, False)
        if K == 128:
            flipped = xr.pack_sign((-host[0][:1]).cuda())
            r.bits[5] = flipped.bits[0]
        ops[K] = (q, ql, r, rl)
        fresh[K] = {k: _new_route(xr, ops[K], C, k)[0] for k in (None, 3)}
        plans[K] = xr.scan_plan(Q, R, K, False)
    buf = torch.empty(max(int(p.ws_bytes) for p in plans.values()), dtype=torch.uint8, device="cuda")
    order = [first, 192 - first, first, 192 - first]
    wrapped = []
    for K in order:
        scan = xr.RankingScan(*ops[K], C, workspace=(plans[K], buf))
        for k in (None, 3):
            scan.histograms(False)
            assert _same(scan.map_all(k), fresh[K][k]), (K, k)
        wrapped.append(int(_gate_words(scan, 3, 1)[0]))
    assert wrapped == [int(K == 128) for K in order]
