"""The label overlap of 65..128 classes as ONE FP4 matrix instruction (csrc/xmh_scan_mfma.h, label_query_f4 / label_item_f4) in
k_scan_hist_r2 (K <= 64), k_scan_hist_r2w (65..128 bits) and the uncached pass 2 k_scan_ap_r2.

Labels are made for the 128-entry operand: lane group `slot` of a tile holds label word `slot`, so the word boundaries 63 | 64 and
95 | 96 are lane-group boundaries, class C - 1 is the last one in front of the zero padding, and a gallery word index past the last
label word (three words: 65..96 classes) is clamped on the item side and must meet a zero operand on the query side.  Every case has
  * query / gallery rows whose ONLY class is 63, 64, 95, 96 or C - 1 (those below C): such a pair overlaps in exactly one entry;
  * rows with all C classes on both sides (a count of C: 128 is the largest an operand can give);
  * pairs without a common class (single-class rows of different classes, gallery rows without any label);
  * C < 128: one side's entries beyond C are zero padding while the other side's lanes hold whatever the clamped word brought.
Histograms must equal those of the VALU kernels (XMH_SCAN_MFMA=0) bit for bit, mAP@all the stable-order oracle's to the tolerance of
tests/test_gpu_retrieval.py.  C = 64 (two label words: the i8 tile, untouched) runs beside them as the control."""
import ctypes

import pytest
import torch

from test_gpu_retrieval import MAP_TOL

H = (5000, 117218)
SHAPES = [(Q, R) for Q in (17, 260) for R in (70, 1500, 10000)]      # tail batch / one chunk / several chunks; a ragged query tile / several
MARKS = (63, 64, 95, 96)


def _case(Q, R, K, C, seed):
    gen = torch.Generator().manual_seed(seed)
    qL = torch.rand(Q, C, generator=gen) < 0.03
    rL = torch.rand(R, C, generator=gen) < 0.03
    qL[torch.arange(Q), torch.randint(0, C, (Q,), generator=gen)] = True
    marks = [c for c in MARKS if c < C - 1] + [C - 1]
    for t, c in enumerate(marks):                    # single-class rows: queries 0.., gallery rows t, t + 37, ... (every chunk has some)
        qL[t] = False
        qL[t, c] = True
        rL[t::37] = False
        rL[t::37, c] = True
    qL[5] = True                                     # all C classes on both sides
    rL[5::37] = True                                 # (relevant to every query: no query is without a relevant item)
    rL[6::37] = False                                # no label at all
    Wm = torch.randn(C, K, generator=gen)
    qB = (qL.float() @ Wm / 4 + torch.randn(Q, K, generator=gen)).sign()
    rB = (rL.float() @ Wm / 4 + torch.randn(R, K, generator=gen)).sign()
    qB[qB == 0] = 1
    rB[rB == 0] = 1
    return qB, rB, qL.long(), rL.long()


def _scan(xr, qB, rB, qL, rL, C):
    return xr.RankingScan(xr.pack_sign(qB.cuda()), xr.pack_labels(qL.cuda()), xr.pack_sign(rB.cuda()), xr.pack_labels(rL.cuda()), C)


@pytest.fixture(scope="module")
def xr():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from xmh import retrieval
    return retrieval


@pytest.mark.gpu
@pytest.mark.parametrize("C", [64, 65, 80, 96, 97, 127, 128])
@pytest.mark.parametrize("K", [16, 64, 128])
def test_label_overlap_histograms_and_map(xr, monkeypatch, K, C):
    from oracle import retrieval as orc
    for (Q, R) in SHAPES:
        qB, rB, qL, rL = _case(Q, R, K, C, seed=1000 * K + 10 * C + Q + R)
        outs = []
        for flag in ("1", "0"):
            monkeypatch.setenv("XMH_SCAN_MFMA", flag)
            scan = _scan(xr, qB, rB, qL, rL, C)
            ha, hr = scan.histograms(True)
            m = scan.map_all(None)[0]
            outs.append((ha.clone(), hr.clone(), float(m.item())))
        monkeypatch.delenv("XMH_SCAN_MFMA")
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), (Q, R, K, C)
        # the relevant counts themselves, from the labels: the single-class and the all-class rows are in them
        rel = ((qL.float() @ rL.float().T) > 0).sum(1).int()
        assert torch.equal(outs[0][1].sum(1).cpu(), rel), (Q, R, K, C)
        want = float(orc.map_k(qB, rB, qL, rL, stable=True))
        assert abs(outs[0][2] - want) < MAP_TOL and abs(outs[1][2] - want) < MAP_TOL, (Q, R, K, C, outs[0][2], outs[1][2], want)


@pytest.mark.gpu
def test_label_overlap_uncached_pass2(xr, monkeypatch):
    """XMH_SCAN_AP_R2=1: no pair cache, k_scan_ap_r2 evaluates the label chain again (query nibbles -1.0, the mask is max(bits, -1))."""
    from oracle import retrieval as orc
    Q, R, K, C = 260, 10000, 64, 97
    qB, rB, qL, rL = _case(Q, R, K, C, seed=97)
    want = float(orc.map_k(qB, rB, qL, rL, stable=True))
    got = {}
    for flag in ("0", "1"):
        monkeypatch.setenv("XMH_SCAN_AP_R2", flag)
        buf = ctypes.create_string_buffer(512)
        from xmh._lib import lib
        assert lib.xmh_scan_describe(Q, R, K, C, 0, buf, 512) == 0
        assert ("k_scan_ap_r2<2," in buf.value.decode()) == (flag == "1"), buf.value
        scan = _scan(xr, qB, rB, qL, rL, C)
        scan.histograms(False)
        m, ap, cap = scan.map_all(None)
        got[flag] = (float(m.item()), ap.clone(), cap.clone())
    assert abs(got["1"][0] - want) < MAP_TOL and abs(got["0"][0] - want) < MAP_TOL, (got["1"][0], got["0"][0], want)
    assert torch.equal(got["0"][2], got["1"][2])
    assert torch.equal(got["0"][1], got["1"][1])      # the same per-chunk sums in the same order as the cached pass 2


@pytest.mark.parametrize("C", [80, 128])
def test_routes_of_65_to_128_classes_keep_their_names(monkeypatch, C):
    """No GPU: the FP4 label tile changes what NML = 2 expands to, not the kernels' names or plans (tests/test_scan_routes_cpu.py)."""
    from xmh import _lib
    rows = ((None, 64, "pass1=k_scan_hist_r2<2, 4, 4, true>;pass2=k_scan_ap_c<false, 8, false>"),
            (None, 100, "pass1=k_scan_hist_r2w<2, 4, 2, true>;pass2=k_scan_ap_c<false, 8, true>"),
            (("XMH_SCAN_AP_R2", "1"), 64, "pass1=k_scan_hist_r2<2, 4, 4, false>;pass2=k_scan_ap_r2<2, 4, 2, false>"))
    for switch, K, want in rows:
        for name in ("XMH_SCAN_MFMA", "XMH_SCAN_AP_R2", "XMH_SCAN_AP_C", "XMH_SCAN_PACK32", "XMH_SCAN_CACHE_MB", "XMH_SCAN_MASKED"):
            monkeypatch.delenv(name, raising=False)
        if switch:
            monkeypatch.setenv(*switch)
        buf = ctypes.create_string_buffer(512)
        assert _lib.lib.xmh_scan_describe(*H, K, C, 0, buf, 512) == 0 and buf.value.decode() == want, (K, C, buf.value)
