"""The route of the exact top-k (csrc/xmh_topk.hip: plan_topk, filter_route) as xmh_topk_describe reports it, with the workspace sizes of
the same plan for binary and ternary codes, and the shapes the plan refuses.  The library plans and describes without a GPU
(device_cu_count() falls back to the MI355X's 256 CUs), so this runs anywhere.  The values were recorded from the library before the
host side was split from the kernels: the workspace layout (byte offsets of every piece), the filter instance per (code words, queries)
and every refusal text are part of what callers and profiles rely on, and a drift in any of them shows up here."""
import ctypes

import pytest

EINVAL, ENOTSUP = -22, -95

# (Q, R, K, k, xmh_topk_describe, xmh_topk_ws_bytes, xmh_topk_ternary_ws_bytes): every code length, every transition of the queries per
# pass (1 / 2 / 4 / 8) and of the matrix-core tiles per pass (1 / 2 / 4; 2 at most at 512 bits), galleries below one tile, at the
# headline size and at 10 M rows, k at both ends.  Ternary 0: the plan refuses (LDS of the 4097-bucket histograms beside 1024 candidates).
ROUTES = [
    (1, 15, 16, 1, "filter=k_topk_filter_short<1, 4, 1>", 69120, 69120),
    (2, 117218, 16, 100, "filter=k_topk_filter_short<1, 4, 2>", 206080, 206336),
    (5, 10000000, 16, 1024, "filter=k_topk_filter_short<1, 4, 8>", 7865856, 7866112),
    (3, 15, 32, 100, "filter=k_topk_filter_short<1, 4, 4>", 206336, 206848),
    (8, 117218, 32, 1024, "filter=k_topk_filter_short<1, 4, 8>", 3393792, 3394816),
    (64, 10000000, 32, 1, "filter=k_topk_filter_short<1, 4, 8>", 4429056, 4437248),
    (1, 15, 64, 1024, "filter=k_topk_filter_short<2, 4, 1>", 75264, 75520),
    (4, 117218, 64, 1, "filter=k_topk_filter_short<2, 4, 4>", 274176, 275200),
    (5, 10000000, 64, 100, "filter=k_topk_filter_short<2, 4, 8>", 1075712, 1076992),
    (17, 15, 64, 1, "filter=k_topk_filter_short<2, 4, 8>", 1154816, 1159168),
    (2, 117218, 128, 100, "filter=k_topk_filter_seq<4, 4, 2>", 207104, 208128),
    (4, 10000000, 128, 1024, "filter=k_topk_filter_seq<4, 4, 4>", 6294784, 6296832),
    (5, 15, 128, 100, "filter=k_topk_filter_mfma<4, 1>", 344832, 347392),
    (16, 117218, 128, 1024, "filter=k_topk_filter_mfma<4, 1>", 6792448, 6800640),
    (17, 10000000, 128, 1, "filter=k_topk_filter_mfma<4, 2>", 1184000, 1192704),
    (32, 15, 128, 1024, "filter=k_topk_filter_mfma<4, 2>", 2376960, 2393344),
    (33, 117218, 128, 1, "filter=k_topk_filter_mfma<4, 4>", 2259968, 2276864),
    (1, 10000000, 256, 100, "filter=k_topk_filter_seq<8, 4, 1>", 363520, 364544),
    (2, 15, 256, 1, "filter=k_topk_filter_seq<8, 4, 2>", 138752, 140800),
    (3, 117218, 256, 100, "filter=k_topk_filter_seq<8, 4, 4>", 414208, 417280),
    (4, 10000000, 256, 1024, "filter=k_topk_filter_seq<8, 4, 4>", 6444288, 6448384),
    (5, 15, 256, 100, "filter=k_topk_filter_mfma<8, 1>", 347392, 352512),
    (8, 117218, 256, 1024, "filter=k_topk_filter_mfma<8, 1>", 6202624, 6210816),
    (16, 10000000, 256, 1, "filter=k_topk_filter_mfma<8, 1>", 1146112, 1162496),
    (17, 15, 256, 1024, "filter=k_topk_filter_mfma<8, 2>", 1272064, 1289472),
    (32, 117218, 256, 1, "filter=k_topk_filter_mfma<8, 2>", 2219008, 2251776),
    (33, 10000000, 256, 100, "filter=k_topk_filter_mfma<8, 4>", 11947776, 11981568),
    (64, 15, 256, 1, "filter=k_topk_filter_mfma<8, 4>", 4392704, 4458240),
    (1, 117218, 512, 100, "filter=k_topk_filter_seq<16, 4, 1>", 345856, 347904),
    (4, 10000000, 512, 1024, "filter=k_topk_filter_seq<16, 4, 4>", 12764416, 6579456),
    (5, 15, 512, 100, "filter=k_topk_filter_mfma<16, 1>", 352512, 362752),
    (16, 117218, 512, 1024, "filter=k_topk_filter_mfma<16, 1>", 46138624, 23659776),
    (17, 10000000, 512, 1, "filter=k_topk_filter_mfma<16, 2>", 1287424, 1298176),
    (33, 15, 512, 1024, "filter=k_topk_filter_mfma<16, 2>", 2501888, 2569472),
    (64, 117218, 512, 1, "filter=k_topk_filter_mfma<16, 2>", 4633600, 4764672),
    (2, 10000000, 1024, 100, "filter=k_topk_filter_seq<32, 4, 2>", 1063936, 460032),
    (3, 15, 1024, 1, "filter=k_topk_filter_seq<32, 4, 4>", 216576, 228864),
    (5, 117218, 1024, 100, "filter=k_topk_filter_seq<32, 4, 8>", 1733888, 1067264),
    (33, 10000000, 1024, 1024, "filter=k_topk_filter_seq<32, 4, 8>", 54271232, 54406400),
    (1, 15, 2048, 100, "filter=k_topk_filter_seq<64, 4, 1>", 77824, 86016),
    (4, 117218, 2048, 1024, "filter=k_topk_filter_seq<64, 4, 4>", 5932288, 0),
    (8, 10000000, 2048, 1, "filter=k_topk_filter_seq<64, 4, 8>", 632064, 685312),
    (64, 15, 2048, 1024, "filter=k_topk_filter_seq<64, 4, 8>", 5244160, 0),
    (5, 10000000, 256, 100, "filter=k_topk_filter_mfma<8, 1>", 1811456, 1816576),        # the benchmark's shapes
    (64, 10000000, 256, 100, "filter=k_topk_filter_mfma<8, 4>", 23169792, 23235328),
    (1, 10000000, 64, 1024, "filter=k_topk_filter_short<2, 4, 1>", 1574400, 1574656),
    (8, 15, 2048, 1024, "filter=k_topk_filter_seq<64, 4, 8>", 656640, 0),
]

# (Q, R, K, k, ternary, error code, error text): what plan_topk refuses, through the entry points that plan without touching a device
UNSUPPORTED_K = "topk: K=%d unsupported (code words must be a power of two up to 64, i.e. K <= 2048)"
REFUSALS = [
    (8, 1000, 96, 10, 0, ENOTSUP, UNSUPPORTED_K % 96),                                   # three code words
    (8, 1000, 96, 10, 1, ENOTSUP, UNSUPPORTED_K % 96),
    (8, 1000, 4096, 10, 0, ENOTSUP, UNSUPPORTED_K % 4096),
    (8, 1000, 64, 0, 0, EINVAL, "topk: k=0 out of range (1..1024)"),
    (8, 1000, 64, 0, 1, EINVAL, "topk: k=0 out of range (1..1024)"),
    (8, 1000, 64, 1025, 0, EINVAL, "topk: k=1025 out of range (1..1024)"),
    (8, 1000, 64, 1025, 1, EINVAL, "topk: k=1025 out of range (1..1024)"),
    (8, 2**31 - 65536, 64, 10, 0, ENOTSUP, "topk: shard of 2147418112 rows (max 2^31-1)"),
    (8, 2**31 - 65536, 64, 10, 1, ENOTSUP, "topk: shard of 2147418112 rows (max 2^31-1)"),
    (0, 1000, 64, 10, 0, EINVAL, "topk: bad shape Q=0 R=1000 K=64"),
    (8, 1000, 2048, 1024, 1, ENOTSUP, "topk: k=1024, K=2048 (ternary) needs 195776 B of LDS (max 163840)"),      # Layout beyond 160 KB
]


def _describe(lib, Q, R, K, k):
    buf = ctypes.create_string_buffer(256)
    rc = lib.xmh_topk_describe(Q, R, K, k, buf, 256)
    return rc, buf.value.decode()


@pytest.mark.parametrize("Q, R, K, k, want, ws_bytes, ternary_ws_bytes", ROUTES)
def test_topk_route(Q, R, K, k, want, ws_bytes, ternary_ws_bytes):
    from xmh import _lib
    rc, got = _describe(_lib.lib, Q, R, K, k)
    assert rc == 0 and got == want, (rc, got, _lib.lib.xmh_last_error())
    assert int(_lib.lib.xmh_topk_ws_bytes(Q, R, K, k)) == ws_bytes
    assert int(_lib.lib.xmh_topk_ternary_ws_bytes(Q, R, K, k)) == ternary_ws_bytes


@pytest.mark.parametrize("Q, R, K, k, tern, code, text", REFUSALS)
def test_topk_refusal(Q, R, K, k, tern, code, text):
    from xmh import _lib
    lib = _lib.lib
    ws_bytes, ws_init = (lib.xmh_topk_ternary_ws_bytes, lib.xmh_topk_ternary_ws_init) if tern else (lib.xmh_topk_ws_bytes, lib.xmh_topk_ws_init)
    assert int(ws_bytes(Q, R, K, k)) == 0
    assert ws_init(Q, R, K, k, None, 0, None) == code and lib.xmh_last_error().decode() == text
    if not tern:
        assert _describe(lib, Q, R, K, k)[0] == code and lib.xmh_last_error().decode() == text


def test_topk_largest_shard_and_workspace_argument_checks():
    """one row under the refused shard size plans; a planned shape refuses a null or short workspace before it touches the device"""
    from xmh import _lib
    lib = _lib.lib
    assert int(lib.xmh_topk_ws_bytes(8, 2**31 - 65537, 64, 10)) == 666880 and int(lib.xmh_topk_ternary_ws_bytes(8, 2**31 - 65537, 64, 10)) == 668928
    assert int(lib.xmh_topk_ws_bytes(8, 1000, 2048, 1024)) == 804096                  # binary codes of the shape ternary codes are refused at
    host = ctypes.create_string_buffer(64)
    for name, ws_init, need in (("xmh_topk_ws_init", lib.xmh_topk_ws_init, 544512), ("xmh_topk_ternary_ws_init", lib.xmh_topk_ternary_ws_init, 546560)):
        assert ws_init(8, 1000, 64, 10, None, 0, None) == EINVAL and lib.xmh_last_error().decode() == "%s: null workspace" % name
        assert ws_init(8, 1000, 64, 10, ctypes.addressof(host), 1, None) == EINVAL
        assert lib.xmh_last_error().decode() == "%s: workspace too small (1 < %d)" % (name, need)
