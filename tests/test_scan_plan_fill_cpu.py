"""The scan planner beside the block map that takes any chunk count (csrc/xmh_scan_map.h): the plans of k_scan_hist_r2 still cut the
gallery into whole batches that cover it without an empty chunk and fit one resident set of blocks, and no plan moved -- filling every
block slot (25 chunks at the headline shape) was measured and stays behind an experiment switch.  No GPU: the planner then sizes for 256
CUs, the device these values were read on."""
import ctypes

import pytest


def _plan(Q, R, K, ternary=0):
    from xmh import _lib
    p = _lib.ScanPlan()
    assert _lib.lib.xmh_scan_plan_make(Q, R, K, ternary, ctypes.byref(p)) == 0
    return p


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256


@pytest.mark.parametrize("Q,R,K", [(5000, 117218, 64), (5000, 117218, 40), (5000, 20000, 64), (700, 45000, 64), (700, 1000000, 48), (16, 300, 64), (17, 20000, 33)])
def test_r2_plans_cover_the_gallery_in_whole_batches(Q, R, K):
    p = _plan(Q, R, K)
    assert p.chunk % 64 == 0 and p.chunk * p.nchunk >= R and (p.nchunk - 1) * p.chunk < R
    assert p.qpad % 256 == 0 and p.qpad >= Q and p.nqtile * 64 == p.qpad and p.nbuckets == K + 1
    # every block of pass 1 (256 queries x one chunk) is resident at once: two per CU
    assert (p.qpad // 256) * p.nchunk <= 2 * _cus() or p.chunk == 256


# (Q, R, K, ternary) -> (chunk, nchunk, nqtile, qpad, nbuckets, ws_bytes) as the library of the commit before this change planned them on
# 256 CUs: the VALU kernels (512 bits), k_scan_hist_b (256 bits, ternary codes), k_scan_hist_r2 / r2w (at most 128 bits)
BEFORE = {
    (5000, 117218, 64, 0): (4928, 24, 80, 5120, 65, 707269376),            # the headline: 20 query blocks x 24 chunks = 480 of 512 block slots
    (5000, 117218, 40, 0): (4928, 24, 80, 5120, 41, 669913856),
    (700, 45000, 64, 0): (320, 141, 12, 768, 65, 120385024),
    (700, 45000, 40, 0): (320, 141, 12, 768, 41, 88903168),
    (5000, 20000, 64, 0): (896, 23, 80, 5120, 65, 203215616),
    (17, 20000, 16, 0): (256, 79, 4, 256, 17, 9487872),
    (17, 20000, 128, 0): (256, 79, 2, 128, 129, 19874816),
    (17, 20000, 256, 0): (256, 79, 1, 64, 257, 17851136),
    (17, 20000, 64, 1): (256, 79, 1, 64, 129, 9954048),
    (700, 45000, 16, 0): (320, 141, 12, 768, 17, 57421312),
    (700, 45000, 32, 0): (320, 141, 12, 768, 33, 78409216),
    (700, 45000, 128, 0): (320, 141, 12, 768, 129, 221662720),
    (700, 45000, 256, 0): (640, 71, 11, 704, 257, 205266176),
    (700, 45000, 512, 0): (944, 48, 11, 704, 513, 213973248),
    (700, 45000, 64, 1): (384, 118, 11, 704, 129, 178266368),
    (700, 45000, 128, 1): (640, 71, 11, 704, 257, 205266176),
    (5000, 117218, 16, 0): (4928, 24, 80, 5120, 17, 632558336),
    (5000, 117218, 32, 0): (4928, 24, 80, 5120, 33, 657462016),
    (5000, 117218, 128, 0): (4928, 24, 80, 5120, 129, 1109660416),
    (5000, 117218, 256, 0): (14656, 8, 79, 5056, 257, 1034956288),
    (5000, 117218, 512, 0): (19544, 6, 79, 5056, 513, 228423168),
    (5000, 117218, 64, 1): (7360, 16, 79, 5056, 129, 1029131776),
    (5000, 117218, 128, 1): (14656, 8, 79, 5056, 257, 1034956288),
    (5000, 1000000, 32, 0): (32768, 31, 80, 5120, 33, 5267182336),
    (5000, 1000000, 128, 0): (32768, 31, 80, 5120, 129, 8058360576),
    (5000, 1000000, 256, 0): (20864, 48, 79, 5056, 257, 8365428224),
    (5000, 1000000, 512, 0): (32768, 31, 79, 5056, 513, 1007047168),
    (5000, 1000000, 128, 1): (20864, 48, 79, 5056, 257, 8365428224),
}


def test_every_plan_is_what_it_was():
    if _cus() != 256:
        pytest.skip("the plans of another device")
    for (Q, R, K, t), want in BEFORE.items():
        p = _plan(Q, R, K, t)
        assert (p.chunk, p.nchunk, p.nqtile, p.qpad, p.nbuckets, p.ws_bytes) == want, (Q, R, K, t)
