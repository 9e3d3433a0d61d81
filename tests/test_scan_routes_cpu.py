"""The route of the ranking scan (csrc/xmh_scan.hip, scan_route) as xmh_scan_describe reports it, with the pair-cache and workspace
sizes of the same plan: the rows of DESIGN 3.1's table, each XMH_SCAN_* switch, and shapes without a kernel instance.  The library
plans and describes without a GPU (device_cu_count() falls back to the MI355X's 256 CUs, the self-check needs a device), so this runs
anywhere; describe is the launches' own route, so a drift between the two shows up here as a changed string."""
import ctypes

import pytest

SWITCHES = ("XMH_SCAN_MFMA", "XMH_SCAN_AP_R2", "XMH_SCAN_AP_C", "XMH_SCAN_PACK32", "XMH_SCAN_CACHE_MB", "XMH_SCAN_MASKED")
ENOTSUP = -95
H = (5000, 117218)                   # the headline shape (configs[1])

# (switch, Q, R, K, C, ternary, describe or error code, xmh_scan_pair_cache_bytes, xmh_scan_ws_bytes_nocache)
ROUTES = [
    (None, *H, 16, 24, 0, "pass1=k_scan_hist_r2<1, 4, 4, true>;pass2=k_scan_ap_c<false, 8, false>", 605552640, 27005696),
    (None, *H, 64, 80, 0, "pass1=k_scan_hist_r2<2, 4, 4, true>;pass2=k_scan_ap_c<false, 8, false>", 605552640, 101716736),
    (None, *H, 100, 80, 0, "pass1=k_scan_hist_r2w<2, 4, 2, true>;pass2=k_scan_ap_c<false, 8, true>", 908328960, 157750016),
    (None, *H, 128, 24, 0, "pass1=k_scan_hist_r2w<1, 4, 2, true>;pass2=k_scan_ap_c<false, 8, true>", 908328960, 201331456),
    (None, *H, 256, 80, 0, "pass1=k_scan_hist_b<4, 4, 2, 2, true, false>;pass2=k_scan_ap_s<8, 1, false, false, 8, true, false, 1, true>|"
                           "k_scan_ap_c<false, 16, false>", 889208832, 145747456),
    (None, *H, 512, 80, 0, "pass1=k_scan_hist_s<16, 3, false, 32, 1, false>;pass2=k_scan_ap_s<16, 3, false, true, 32, true, false, 1, false>|"
                           "k_scan_ap_s<16, 3, false, true, 32, false, false, 1, false>", 0, 228423168),
    (None, *H, 2048, 24, 0, "pass1=k_scan_hist_s<64, 1, false, 64, 8, false>;pass2=k_scan_ap_s<64, 1, false, true, 64, true, false, 8, false>|"
                            "k_scan_ap_s<64, 1, false, true, 64, false, false, 8, false>", 0, 663158272),
    (None, *H, 64, 255, 0, "pass1=k_scan_hist_s<2, 8, false, 4, 1, true>;pass2=k_scan_ap_c<false, 8, false>", 605552640, 101716736),
    (None, *H, 256, 255, 0, "pass1=k_scan_hist_s<8, 8, false, 8, 1, true>;pass2=k_scan_ap_s<8, 1, false, false, 8, true, false, 1, true>|"
                            "k_scan_ap_c<false, 16, false>", 889208832, 145747456),
    (None, *H, 16, 24, 1, "pass1=k_scan_hist_b<2, 4, 2, 2, true, true>;pass2=k_scan_ap_c<false, 16, false>", 893091840, 35081728),
    (None, *H, 64, 80, 1, "pass1=k_scan_hist_b<2, 4, 2, 2, true, true>;pass2=k_scan_ap_c<false, 16, false>", 893091840, 136039936),
    (None, *H, 128, 80, 1, "pass1=k_scan_hist_b<4, 4, 2, 2, true, true>;pass2=k_scan_ap_s<8, 1, false, false, 8, true, false, 1, true>|"
                           "k_scan_ap_c<false, 16, false>", 889208832, 145747456),
    (None, *H, 256, 24, 1, "pass1=k_scan_hist_b<8, 4, 2, 1, true, true>;pass2=k_scan_ap_s<8, 1, false, false, 8, true, false, 1, true>|"
                           "k_scan_ap_c<false, 16, false>", 889208832, 290713088),
    (None, 5000, 1250000, 256, 80, 0, "pass1=k_scan_hist_b<4, 4, 2, 2, true, false>;pass2=k_scan_ap_s<8, 1, false, false, 8, true, false, 1, true>|"
                                      "k_scan_ap_c<false, 16, false>", 9486188544, 895168000),
    (None, 16, 2, 64, 24, 0, "pass1=k_scan_hist_r2<1, 4, 4, true>;pass2=k_scan_ap_c<false, 8, false>", 65536, 501248),
    (("XMH_SCAN_MFMA", "0"), *H, 64, 80, 0, "pass1=k_scan_hist_s<2, 3, false, 4, 1, true>;pass2=k_scan_ap_c<false, 8, false>", 597983232, 100445696),
    (("XMH_SCAN_MFMA", "0"), *H, 64, 80, 1, "pass1=k_scan_hist_s<2, 3, true, 8, 1, false>;pass2=k_scan_ap_s<2, 3, true, true, 8, false, false, 1, false>",
     0, 198815232),
    (("XMH_SCAN_AP_R2", "1"), *H, 64, 80, 0, "pass1=k_scan_hist_r2<2, 4, 4, false>;pass2=k_scan_ap_r2<2, 4, 2, false>", 0, 101716736),
    (("XMH_SCAN_AP_C", "0"), *H, 64, 24, 0, "pass1=k_scan_hist_r2<1, 4, 4, true>;pass2=k_scan_ap_s<2, 1, false, false, 4, false, false, 1, true>",
     605552640, 101716736),
    # one-byte entries of 65..128-bit codes: the cached k_scan_ap_s cannot read them, pass 2 evaluates the pairs from the codes
    (("XMH_SCAN_AP_C", "0"), *H, 128, 80, 0, "pass1=k_scan_hist_r2w<2, 4, 2, true>;pass2=k_scan_ap_s<4, 3, false, true, 8, true, false, 1, false>|"
                                             "k_scan_ap_s<4, 3, false, true, 8, false, false, 1, false>", 908328960, 201331456),
    (("XMH_SCAN_AP_C", "0"), *H, 256, 80, 0, "pass1=k_scan_hist_b<4, 4, 2, 2, true, false>;pass2=k_scan_ap_s<8, 1, false, false, 8, true, false, 1, true>|"
                                             "k_scan_ap_s<8, 1, false, false, 8, false, false, 1, true>", 889208832, 145747456),
    (("XMH_SCAN_PACK32", "0"), 70, 21000, 256, 24, 0, "pass1=k_scan_hist_b<4, 4, 2, 2, true, false>;pass2=k_scan_ap_c<false, 16, false>", 4079616, 33367040),
    (("XMH_SCAN_PACK32", "all"), *H, 64, 80, 0, "pass1=k_scan_hist_r2<2, 4, 4, true>;pass2=k_scan_ap_s<2, 1, false, false, 4, true, false, 1, true>|"
                                                "k_scan_ap_s<2, 1, false, false, 4, false, false, 1, true>", 605552640, 101716736),
    (("XMH_SCAN_PACK32", "all"), *H, 16, 24, 0, "pass1=k_scan_hist_r2<1, 4, 4, true>;pass2=k_scan_ap_s<1, 1, false, false, 4, true, false, 1, true>|"
                                                "k_scan_ap_s<1, 1, false, false, 4, false, false, 1, true>", 605552640, 27005696),
    (("XMH_SCAN_CACHE_MB", "0"), *H, 64, 80, 0, "pass1=k_scan_hist_r2<2, 4, 4, false>;pass2=k_scan_ap_r2<2, 4, 2, false>", 0, 101716736),
    (("XMH_SCAN_CACHE_MB", "0"), *H, 256, 80, 0, "pass1=k_scan_hist_b<4, 4, 2, 2, false, false>;pass2=k_scan_ap_s<8, 3, false, true, 8, true, false, 1, false>|"
                                                 "k_scan_ap_s<8, 3, false, true, 8, false, false, 1, false>", 0, 145747456),
    # more than 128 classes on ternary codes and on binary codes beyond 256 bits: no kernel instance (the launch says the same)
    (None, *H, 64, 255, 1, ENOTSUP, 893091840, 136039936),
    (None, 90, 7000, 256, 255, 1, ENOTSUP, 1376256, 23161856),
    (None, *H, 512, 255, 0, ENOTSUP, 0, 228423168),
]


@pytest.mark.parametrize("switch, Q, R, K, C, tern, want, cache_bytes, nocache_bytes", ROUTES)
def test_scan_route(monkeypatch, switch, Q, R, K, C, tern, want, cache_bytes, nocache_bytes):
    from xmh import _lib
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    if switch:
        monkeypatch.setenv(*switch)
    buf = ctypes.create_string_buffer(512)
    rc = _lib.lib.xmh_scan_describe(Q, R, K, C, tern, buf, 512)
    if isinstance(want, str):
        assert rc == 0 and buf.value.decode() == want, (rc, buf.value, _lib.lib.xmh_last_error())
    else:
        assert rc == want and b"unsupported shape" in _lib.lib.xmh_last_error(), (rc, buf.value)
    assert int(_lib.lib.xmh_scan_pair_cache_bytes(Q, R, K, tern)) == cache_bytes
    assert int(_lib.lib.xmh_scan_ws_bytes_nocache(Q, R, K, tern)) == nocache_bytes
