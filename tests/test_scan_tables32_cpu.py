"""When the ranking scan keeps its chunk-offset table between the passes in the packed form (one 32-bit word per cell): the host's rule
(csrc/xmh_scan.hip, tables_packed, stated above scan_route and in DESIGN 3.1) as xmh_scan_tables_packed reports it.  Like
xmh_scan_describe it is the launches' own route and needs no GPU.  Packed exactly when the call is unsharded, its pass 2 is
k_scan_ap_c alone, and twice the fullest bucket of random codes, 2 R C(K, K/2) / 2^K, fits 16 bits."""
import ctypes
from math import comb

import pytest

SWITCHES = ("XMH_SCAN_MFMA", "XMH_SCAN_AP_R2", "XMH_SCAN_AP_C", "XMH_SCAN_PACK32", "XMH_SCAN_CACHE_MB", "XMH_SCAN_MASKED")
H = (5000, 117218)                   # the headline shape
UNSHARDED, BASE_ALL, TOTALS, ALL_TO_ALL = range(4)

# (switch, Q, R, K, C, mode, packed, what pass 2 must (not) be)
ROWS = [
    (None, *H, 64, 80, UNSHARDED, 1, "k_scan_ap_c<false, 8, false>"),                   # the headline
    (None, *H, 16, 24, UNSHARDED, 1, "k_scan_ap_c<false, 8, false>"),
    (None, *H, 64, 255, UNSHARDED, 1, "k_scan_ap_c<false, 8, false>"),                  # pass 1 on the VALU (more than 128 classes): the other counter format
    (None, 70, 5000, 64, 80, UNSHARDED, 1, "k_scan_ap_c<false, 8, false>"),
    # the sharded entry points: offsets from the caller, from gathered totals, from all-to-all slices
    (None, *H, 64, 80, BASE_ALL, 0, None),
    (None, *H, 64, 80, TOTALS, 0, None),
    (None, *H, 64, 80, ALL_TO_ALL, 0, None),
    # k_scan_ap_s routes, k_scan_ap_r2, and k_scan_ap_c with a second launch behind or beside it
    (("XMH_SCAN_AP_C", "0"), *H, 64, 24, UNSHARDED, 0, "k_scan_ap_s<"),
    (("XMH_SCAN_PACK32", "all"), *H, 64, 80, UNSHARDED, 0, "k_scan_ap_s<"),
    (None, *H, 512, 80, UNSHARDED, 0, "k_scan_ap_s<"),
    (("XMH_SCAN_CACHE_MB", "0"), *H, 64, 80, UNSHARDED, 0, "k_scan_ap_r2<"),
    (None, *H, 128, 80, UNSHARDED, 0, "k_scan_ap_c<false, 8, true>"),                   # its stand-in is launched behind it
    (None, *H, 256, 80, UNSHARDED, 0, "|k_scan_ap_c<false, 16, false>"),                # beside the packed 32-bit k_scan_ap_s
    # shards whose fullest bucket is not expected to fit 16 bits: 16-bit codes on a million rows (a fifth of them at distance 8), and the
    # sizes on either side of the threshold at 64 bits
    (None, 5000, 1000000, 16, 24, UNSHARDED, 0, "k_scan_ap_c<false, 8, false>"),
    (None, 16, 70000, 64, 24, UNSHARDED, 1, "k_scan_ap_c<false, 8, false>"),
    (None, 16, 329800, 64, 24, UNSHARDED, 1, "k_scan_ap_c<false, 8, false>"),
    (None, 16, 329900, 64, 24, UNSHARDED, 0, "k_scan_ap_c<false, 8, false>"),
    (None, 32, 70000, 16, 24, UNSHARDED, 1, "k_scan_ap_c<false, 8, false>"),
]


@pytest.mark.parametrize("switch, Q, R, K, C, mode, packed, pass2", ROWS)
def test_tables_packed_rule(monkeypatch, switch, Q, R, K, C, mode, packed, pass2):
    from xmh import _lib
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    if switch:
        monkeypatch.setenv(*switch)
    assert int(_lib.lib.xmh_scan_tables_packed(Q, R, K, C, 0, mode)) == packed, _lib.lib.xmh_last_error()
    if pass2:
        buf = ctypes.create_string_buffer(512)
        assert _lib.lib.xmh_scan_describe(Q, R, K, C, 0, buf, 512) == 0 and pass2 in buf.value.decode(), buf.value
    if packed:                                                                          # the estimate the rule states
        assert 2 * R * comb(K, K // 2) / 2.0 ** K <= 65535
    assert R // (K + 1) <= 65535 or not packed                                          # pigeonhole: no such shard can fit


def test_bad_arguments():
    from xmh import _lib
    assert int(_lib.lib.xmh_scan_tables_packed(*H, 64, 80, 0, 4)) < 0
    assert int(_lib.lib.xmh_scan_tables_packed(*H, 64, 80, 0, -1)) < 0
    assert int(_lib.lib.xmh_scan_gate_offset(*H, 64, 0)) % 4 == 0
