"""GPU: the block map and the launch geometry of the scan (csrc/xmh_scan_map.h, launch_geom) at the shapes where they take another path.

A plan's last chunk count is ceil(R / chunk), so a launch has up to seven chunks outside the whole groups of 8 that are pinned to one XCD
each: the block map deals their blocks over the XCDs.  And pass 2 launches only the query tiles that hold a query, while every layout
keeps the padded count.  Checked here: every (chunk, tile) is scanned exactly once (histogram row sums), both histograms equal the VALU route's bit for
bit, and the per-query AP sums and the mAP match the oracle (oracle.retrieval.map_k(stable=True) for the mean; for the sums its loop
restated for all queries at once, _ap_sums) -- divisors equal, sums within 4e-6 relative + 1e-9, the tolerance the library's own re-derivation
(xmh_scan_verify) holds two chunkings to.  The routes at 16 and 128 bits are pinned to the chunk count the library gave before this
file existed.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

AP_RTOL, AP_ATOL = 4e-6, 1e-9
MAP_TOL = 1e-6                       # the mean against map_k (float32 arithmetic in the oracle): the bar of tests/test_gpu_retrieval.py
Q0, R0 = 700, 45000                  # 3 query blocks of 256; on 256 CUs 141 chunks of 320 (17 whole groups + 5), the last one ragged


@pytest.fixture(scope="module")
def xr():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from xmh import retrieval
    return retrieval


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _synth(Q, R, K, C, seed, p=0.08):
    """label-correlated codes (as the small cases of tests/test_gpu_retrieval.py); every query has a relevant item"""
    gen = torch.Generator().manual_seed(seed)
    qL = (torch.rand(Q, C, generator=gen) < p)
    rL = (torch.rand(R, C, generator=gen) < p)
    qL[torch.arange(Q), torch.randint(0, C, (Q,), generator=gen)] = True
    rL[torch.arange(R), torch.randint(0, C, (R,), generator=gen)] = True
    qL[:, 0] = True
    rL[::3, 0] = True
    Wm = torch.randn(C, K, generator=gen)
    qB = (qL.float() @ Wm + 0.8 * torch.randn(Q, K, generator=gen)).sign()
    rB = (rL.float() @ Wm + 0.8 * torch.randn(R, K, generator=gen)).sign()
    qB[qB == 0] = 1
    rB[rB == 0] = 1
    return qB, rB, qL.to(torch.int64), rL.to(torch.int64)


def _ap_sums(dist, rel, ks):
    """per query: sum over the first min(n_rel, k) relevant items of ordinal / rank under the stable order (distance, then gallery index)
    -- the loop of oracle.retrieval.map_k(stable=True) for all queries at once, in float64 and before the division by the cap.  (The
    oracle's own per-query form, ap_from_ranking, takes 2.5 s per k at 700 x 45 000; the mean of these sums is held to map_k below.)"""
    order = torch.sort(torch.from_numpy(dist.astype(np.int16)), dim=-1, stable=True).indices
    hits = torch.from_numpy(rel).gather(1, order)
    ordinal = torch.cumsum(hits, 1, dtype=torch.int32)
    credit = ordinal.double() / torch.arange(1, dist.shape[1] + 1, dtype=torch.float64)
    nrel = rel.sum(-1)
    out = {}
    for k in ks:
        cap = nrel if k is None else np.minimum(nrel, k)
        take = hits & (ordinal <= torch.from_numpy(cap.astype(np.int32))[:, None])
        out[k] = ((credit * take).sum(1).numpy(), cap)
    return out


@functools.lru_cache(maxsize=None)
def _case(Q, R, K, C, with_mean=False):
    """inputs and reference results of one shape, computed once and shared: per-query AP sums and divisors for k = None and 50, the
    histograms, and (with_mean) oracle.retrieval.map_k(stable=True) itself, which the mean of the per-query sums has to meet"""
    from oracle import retrieval as orc
    qB, rB, qL, rL = _synth(Q, R, K, C, seed=Q + R + K + C)
    dist = orc.hamming_dist(qB, rB).numpy().astype(np.uint16)
    rel = orc.relevance_packed(orc.pack_labels(qL.numpy()), orc.pack_labels(rL.numpy()))
    assert (rel.sum(-1) > 0).all()
    want = _ap_sums(dist, rel, (None, 50))
    hist = orc.bucket_histograms(dist, rel, K + 1)
    mean = None
    if with_mean:
        mean = {k: float(orc.map_k(qB, rB, qL.float(), rL.float(), k, stable=True)) for k in (None, 50)}
        for k, (ap, cap) in want.items():
            assert abs(float(np.mean(ap / cap)) - mean[k]) < MAP_TOL, k
    return (qB, rB, qL, rL), want, hist, mean


def _scan(xr, data, C):
    qB, rB, qL, rL = data
    return xr.RankingScan(xr.pack_sign(qB.cuda()), xr.pack_labels(qL.cuda()), xr.pack_sign(rB.cuda()), xr.pack_labels(rL.cuda()), C)


def _check_against_oracle(scan, want, mean=None):
    for k, (ap_want, cap_want) in want.items():
        m, ap, cap = scan.map_all(k)
        assert np.array_equal(cap.cpu().numpy(), cap_want), k
        ap = ap.cpu().numpy()
        err = np.abs(ap - ap_want) - (AP_RTOL * np.abs(ap_want) + AP_ATOL)
        assert (err <= 0).all(), (k, int(np.argmax(err)), float(err.max()))
        assert abs(float(m.item()) - float(np.mean(ap_want / cap_want))) < 1e-7, k     # the mean of those sums, in float64 on both sides
        if mean is not None:
            assert abs(float(m.item()) - mean[k]) < MAP_TOL, (k, float(m.item()), mean[k])


@pytest.mark.parametrize("K,C", [(64, 80), (40, 24)])      # (40, 24): a partial second code word, one i8 label tile (k_scan_hist_r2<1, ...>)
def test_leftover_chunks_and_padded_query_tiles(xr, monkeypatch, K, C):
    data, want, (hist_all, hist_rel), mean = _case(Q0, R0, K, C, with_mean=K == 64)
    scan = _scan(xr, data, C)
    pl = scan.plan
    plan = dict(chunk=pl.chunk, nchunk=pl.nchunk, nqtile=pl.nqtile, qpad=pl.qpad)
    if not (pl.nchunk % 8 != 0 and pl.qpad // 16 > -(-Q0 // 16) and Q0 % 16 != 0 and R0 % pl.chunk != 0):
        pytest.skip("this device's plan has no leftover chunk or no padded tile: %r" % plan)
    ha, hr = scan.histograms(True)
    assert (ha.to(torch.int64).sum(1) == R0).all()           # every (chunk, tile) scanned exactly once
    assert np.array_equal(_u32(ha), hist_all) and np.array_equal(_u32(hr), hist_rel)
    _check_against_oracle(scan, want, mean)
    monkeypatch.setenv("XMH_SCAN_MFMA", "0")                 # the VALU kernels, in the same process
    valu = _scan(xr, data, C)
    va, vr = valu.histograms(True)
    assert torch.equal(va, ha) and torch.equal(vr, hr)
    _check_against_oracle(valu, want)


# nchunk as xmh_scan_plan_make gave it at the commit before the block map took leftover chunks (its library, 256 CUs, Q 700 x R 45 000):
# K = 16 -> 141 chunks of 320, K = 128 -> 141 chunks of 320.  These plans keep their rounding; their grids go through the new map.
@pytest.mark.parametrize("K,C,nchunk_before", [(16, 80, 141), (128, 80, 141)])
def test_routes_whose_plan_did_not_change(xr, K, C, nchunk_before):
    data, want, (hist_all, hist_rel), _ = _case(Q0, R0, K, C)
    scan = _scan(xr, data, C)
    if torch.cuda.get_device_properties(0).multi_processor_count == 256:
        assert scan.plan.nchunk == nchunk_before and scan.plan.chunk == 320
    ha, hr = scan.histograms(True)
    assert np.array_equal(_u32(ha), hist_all) and np.array_equal(_u32(hr), hist_rel)
    _check_against_oracle(scan, want)


@pytest.mark.parametrize("Q,R", [(16, 300), (17, 20000)])   # one 16-query tile exactly full; one query spilling into a second tile
def test_full_tile_and_one_query_more(xr, Q, R):
    K, C = 64, 80
    data, want, (hist_all, hist_rel), mean = _case(Q, R, K, C, with_mean=True)
    scan = _scan(xr, data, C)
    ha, hr = scan.histograms(True)
    assert np.array_equal(_u32(ha), hist_all) and np.array_equal(_u32(hr), hist_rel)
    _check_against_oracle(scan, want, mean)


def test_sharded_forms_equal_the_unsharded_scan(xr):
    """world 2 on one device, as the four-offset-sources test of tests/test_gpu_retrieval.py sets it up: the gathered totals tables
    (xmh_hamming_map_sharded) and the explicit offset slices (xmh_hamming_map_sharded_offsets)"""
    from xmh import sharded
    K, C, world = 64, 80, 2
    data, want, _, _ = _case(Q0, R0, K, C, with_mean=True)
    whole = _scan(xr, data, C)
    whole.histograms(False)
    qB, rB, qL, rL = data
    q, ql = xr.pack_sign(qB.cuda()), xr.pack_labels(qL.cuda())
    r, rl = xr.pack_sign(rB.cuda()), xr.pack_labels(rL.cuda())
    b = sharded.shard_bounds(R0, world)
    shards = [sharded.HipShardOps(q, ql, r.rows(b[i], b[i + 1]), rl[b[i]:b[i + 1]].contiguous(), C) for i in range(world)]
    tables = [o.totals().clone() for o in shards]                                     # [nb, qpad, 2] each
    nb, qpad = tables[0].shape[0], tables[0].shape[1]
    assert qpad % world == 0 and qpad // 16 > -(-Q0 // 16)
    sends = [t.view(nb, world, qpad // world, 2).permute(1, 0, 2, 3).contiguous() for t in tables]
    offs = [xr.slice_offsets(torch.stack([sends[w][j] for w in range(world)]).contiguous()) for j in range(world)]
    tg = torch.stack(tables).contiguous()
    for k in (None, 50):
        got_whole = float(whole.map_all(k)[0].item())
        assert abs(got_whole - float(np.mean(want[k][0] / want[k][1]))) < 1e-7
        got = got_gather = 0.0
        for w, o in enumerate(shards):
            got += float(o.map_partial_offsets(k, torch.stack([offs[j][w] for j in range(world)]).contiguous()).item())
            got_gather += float(o.map_partial(k, tg, w).item())
        # fp32 credits summed per chunk, and the shards chunk the gallery differently: the bar of the existing sharded tests
        assert abs(got - got_whole) < 1e-7 and abs(got - got_gather) < 1e-12, k
