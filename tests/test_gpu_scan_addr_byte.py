"""Pass 1 of the ranking scan takes the distance half of the pair-cache byte from the counter address (csrc/xmh_scan_mfma.h,
scan_hist_r2_body: counter rows of 512 bytes, byte 1 of the address is 2 * distance) instead of from a chain of its own.

Codes are made for that byte and for the counter layout behind it:
  * queries whose popcounts run through 0, 1, ..., K (the chain starts at 512 * popcount): the all-zero and the all-one code among them;
  * gallery rows equal to a query (distance 0: the lowest counter row), equal to its complement (distance K: the highest row; at
    K = 128 the byte wraps and pass 2 takes its stand-in) and one bit off the complement (K - 1) -- in the first batch, in the ragged
    last batch and on either side of a chunk boundary, each once sharing the query's classes and once without a label;
  * Q = 273: a whole block with all 16 (wave, query group) positions -- query 255 has the highest counter address -- and a ragged one.
Histograms and divisors must equal those of the VALU kernels (XMH_SCAN_MFMA=0) bit for bit, every query's AP sum the float64 oracle's
to the tolerance of tests/test_gpu_retrieval.py (a distance byte that is off moves an item to another bucket: at R = 70 that is a
change of percents), mAP@all the stable-order oracle's."""
import ctypes

import numpy as np
import pytest
import torch

from test_gpu_retrieval import MAP_TOL, _u32

H = (5000, 117218)
SHAPES = [(Q, R) for Q in (17, 273) for R in (70, 192, 1500, 10000)]
KINDS = [(d, shared) for d in ("same", "complement", "one_off") for shared in (True, False)]


def _case(xr, Q, R, K, C, seed):
    gen = torch.Generator().manual_seed(seed)
    qL = torch.rand(Q, C, generator=gen) < 0.05
    rL = torch.rand(R, C, generator=gen) < 0.05
    qL[torch.arange(Q), torch.randint(0, C, (Q,), generator=gen)] = True          # every query has a class
    rL[5::37] = True                                                                # ... and a relevant item
    qB = -torch.ones(Q, K)
    for i in range(Q):                                                              # popcounts 0 .. K: all of them where Q allows, else spread with both ends
        p = i % (K + 1) if Q > K else round(i * K / (Q - 1))
        qB[i, torch.randperm(K, generator=gen)[:p]] = 1.0
    rB = torch.randn(R, K, generator=gen).sign()
    rB[rB == 0] = 1
    chunk = int(xr.scan_plan(Q, R, K, False).chunk)
    places = [8, R - len(KINDS)]                                                    # the first batch; the last one (ragged where R % 64 != 0)
    if chunk + len(KINDS) <= R - len(KINDS):
        places += [chunk - len(KINDS), chunk]                                       # the last rows of chunk 0, the first of chunk 1
    queries = sorted({0, 1, K % Q, (K // 2) % Q, min(240, Q - 1), min(255, Q - 1), Q - 1})
    n = 0
    for base in places:
        for v, (d, shared) in enumerate(KINDS):
            q = queries[n % len(queries)]
            n += 1
            row = qB[q].clone() if d == "same" else -qB[q]
            if d == "one_off":
                row[(q + v) % K] *= -1
            rB[base + v] = row
            rL[base + v] = qL[q] if shared else False
    return qB, rB, qL.long(), rL.long()


@pytest.fixture(scope="module")
def xr():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from xmh import retrieval
    return retrieval


@pytest.mark.gpu
@pytest.mark.parametrize("C", [24, 80])
@pytest.mark.parametrize("K", [16, 32, 64, 65, 96, 128])
def test_distance_byte_from_the_address(xr, monkeypatch, K, C):
    from oracle import retrieval as orc
    for (Q, R) in SHAPES:
        qB, rB, qL, rL = _case(xr, Q, R, K, C, seed=1000 * K + 10 * C + Q + R)
        q, r = xr.pack_sign(qB.cuda()), xr.pack_sign(rB.cuda())
        ql, rl = xr.pack_labels(qL.cuda()), xr.pack_labels(rL.cuda())
        dist = orc.hamming_packed(_u32(q.bits), _u32(r.bits))
        rel = orc.relevance_packed(_u32(ql), _u32(rl))
        assert dist.min() == 0 and dist.max() == K                                  # the planted rows are what they were made to be
        want_ap = orc.ap_from_ranking(dist, rel)
        want = float(orc.map_k(qB, rB, qL, rL, stable=True))
        outs = []
        for flag in ("1", "0"):
            monkeypatch.setenv("XMH_SCAN_MFMA", flag)
            scan = xr.RankingScan(q, ql, r, rl, C)
            ha, hr = scan.histograms(True)
            ap, cap = scan.ap_sums(None)
            m = float(xr.map_finalize(ap, cap).item())
            outs.append((ha.clone(), hr.clone(), cap.clone(), ap.cpu().numpy(), m))
        monkeypatch.delenv("XMH_SCAN_MFMA")
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), (Q, R, K, C)
        assert torch.equal(outs[0][2], outs[1][2]), (Q, R, K, C)
        assert np.array_equal(outs[0][2].cpu().numpy(), rel.sum(-1)), (Q, R, K, C)
        for o in outs:
            err = np.abs(o[3] - want_ap) / np.maximum(np.abs(want_ap), 1e-30)
            assert np.allclose(o[3], want_ap, rtol=2e-6, atol=1e-9), (Q, R, K, C, float(err.max()))
            assert abs(o[4] - want) < MAP_TOL, (Q, R, K, C, o[4], want)


def test_routes_and_workspaces_keep_their_names_and_sizes(monkeypatch):
    """No GPU: the counter layout changes the LDS of a launch, not the kernels' names, the plans or the workspaces (tests/test_scan_routes_cpu.py)."""
    from xmh import _lib
    rows = ((64, 80, "pass1=k_scan_hist_r2<2, 4, 4, true>;pass2=k_scan_ap_c<false, 8, false>", 605552640, 101716736),
            (16, 24, "pass1=k_scan_hist_r2<1, 4, 4, true>;pass2=k_scan_ap_c<false, 8, false>", 605552640, 27005696),
            (128, 24, "pass1=k_scan_hist_r2w<1, 4, 2, true>;pass2=k_scan_ap_c<false, 8, true>", 908328960, 201331456))
    for name in ("XMH_SCAN_MFMA", "XMH_SCAN_AP_R2", "XMH_SCAN_AP_C", "XMH_SCAN_PACK32", "XMH_SCAN_CACHE_MB", "XMH_SCAN_MASKED"):
        monkeypatch.delenv(name, raising=False)
    for K, C, want, cache_bytes, nocache_bytes in rows:
        buf = ctypes.create_string_buffer(512)
        assert _lib.lib.xmh_scan_describe(*H, K, C, 0, buf, 512) == 0 and buf.value.decode() == want, (K, C, buf.value)
        assert int(_lib.lib.xmh_scan_pair_cache_bytes(*H, K, 0)) == cache_bytes, K
        assert int(_lib.lib.xmh_scan_ws_bytes_nocache(*H, K, 0)) == nocache_bytes, K
