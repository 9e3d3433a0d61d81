"""Parity-mode numerics of the encoder against float64: the fp16 operand planes bit for bit, componentwise error bounds for the
GEMM, LayerNorm and attention, and whole towers (synthetic and outlier weights, three precisions) with a per-row metric.

Unit roundoff u = 2^-24.  Parity mode splits every fp32 operand x into fp16 planes hi + lo (csrc/xmh_planes.h): the split
loses at most 2^-21 |x| for |x| >= 2^-3 and at most 2^-23 absolutely below that (the planes turn subnormal), so every bound
below carries a relative term and a small absolute one.  Fast mode rounds x to one fp16 plane (2^-11 relative)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import encode_numerics as N

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from xmh import ops as o
    o.set_precision("f32")
    return o


def g_(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------------------------------------
# the planes, bit for bit: A @ I^T with K = N = 64 returns every element of A as the GEMM saw it (one nonzero product per
# output, each exact, summed in fp32 with zeros)
# ---------------------------------------------------------------------------------------------------------------------------
def crafted_values():
    rng = np.random.default_rng(11)
    f32 = np.float32
    tiny = np.array([1.4e-45, 1e-40, 5.877e-39, 1.1754942e-38], dtype=f32)                     # fp32 subnormals, largest one
    sub16 = np.concatenate([[2.0 ** -24, 2.0 ** -24 * 1.5, 2.0 ** -25, 2.0 ** -25 * 1.9, 2.0 ** -14, 2.0 ** -14 * (1 - 2.0 ** -11),
                             2.0 ** -14 * (1 - 2.0 ** -23), 2.0 ** -14 * (1 + 2.0 ** -23)],
                            np.exp2(rng.uniform(-24, -14, 40))])                                 # fp16 subnormal range and its edges
    lo_sub = np.concatenate([[2.0 ** -5, 2.0 ** -2, 2.0 ** -3, 2.0 ** -3 * (1 - 2.0 ** -23)], np.exp2(rng.uniform(-5, -2, 40))])
    wide = np.exp2(rng.uniform(-30, 16, 200)) * rng.uniform(1, 2, 200)                            # exponents -30 .. +15
    wide = wide[wide < 65504]
    band = np.array([65504.0, 65504.5, 65510.0, 65519.0, 65519.99, 65520.0, 65535.99, 65535.996], dtype=f32)
    sat = np.array([65536.0, 65600.0, 70000.0, 1.0e5, 3.0e5, 1.0e6, 1.0e10, 3.4e38], dtype=f32)
    body = np.concatenate([[0.0], tiny, sub16, lo_sub, wide, band, sat]).astype(f32)
    bits = body.view(np.uint32) | rng.integers(0, 1 << 13, body.size, dtype=np.uint32) * (body > 2.0 ** -14)   # random low bits too
    body = np.concatenate([body, bits.view(f32)])
    body = np.concatenate([body, -body])
    rows = -(-body.size // 64)
    return np.concatenate([body, np.zeros(rows * 64 - body.size, f32)]).reshape(rows, 64)


def nonfinite_rows():
    A = np.ones((6, 64), np.float32)
    for r, v in enumerate((np.inf, -np.inf, np.nan, -np.nan)):
        A[r, 7 * r] = v
    A[4, 0], A[5, 63] = np.nan, np.inf
    return A


def _identity_gemm(ops, A, prec):
    from xmh import _lib
    eye = torch.eye(64).cuda()
    _lib.prof_enable(True)
    try:
        got = ops.gemm_nt(torch.from_numpy(A).cuda(), eye, precision=prec).cpu().numpy()
        torch.cuda.synchronize()
        kernel = "gemm_s16" if prec == ops.PREC_F32 else "gemm_f16"
        ran = _lib.prof_read(kernel)[1]
    finally:
        _lib.prof_enable(False)
    return got, ran


def _assert_same_values(got, want, what):
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    if bad.any():
        i = np.argwhere(bad)[:8]
        raise AssertionError("%s: %d elements differ, e.g. %s" % (what, bad.sum(), [(float(got[tuple(j)]), float(want[tuple(j)])) for j in i]))


def test_parity_planes_are_the_emulated_split_bit_for_bit(ops):
    A = crafted_values()
    got, ran = _identity_gemm(ops, A, ops.PREC_F32)
    assert ran >= 1                                                            # the split kernel, not the exact fallback
    want = N.split_value(A)
    _assert_same_values(got, want, "parity planes")
    # the domain: below 65536 the two planes hold x to 2^-21 (relative) / 2^-23 (absolute); from 65536 on hi saturates at 65504
    a, g = np.abs(A.astype(np.float64)), np.abs(got.astype(np.float64))
    inside = a < 65536.0
    assert (np.abs(got[inside] - A[inside]) <= np.maximum(2.0 ** -21 * a[inside], 2.0 ** -23)).all()
    assert np.isfinite(got).all() and (g[~inside] < a[~inside]).all() and (g <= 2 * 65504.0).all()


def test_parity_planes_propagate_nan_and_inf(ops):
    A = nonfinite_rows()
    got, _ = _identity_gemm(ops, A, ops.PREC_F32)
    want = A.astype(np.float64) @ np.eye(64)                                   # inf * 0 = NaN: the whole row is non-finite
    assert np.array_equal(np.isfinite(got), np.isfinite(want))
    _assert_same_values(got, N.split_value(A) @ np.eye(64, dtype=np.float32), "non-finite rows")


def test_fast_mode_plane_rounds_to_nearest_and_overflows_to_inf(ops):
    """fast mode: hi = half(x) rounded to nearest.  From 65520 up that is inf, so a finite activation >= 65520 makes its whole output
    row non-finite (inf * 0 in the other columns) -- the documented edge of fast mode, pinned here."""
    A = crafted_values()
    got, ran = _identity_gemm(ops, A, ops.PREC_F16)
    assert ran >= 1
    want = N.fast_value(A).astype(np.float64) @ np.eye(64)
    assert np.array_equal(np.isfinite(got), np.isfinite(want))
    fin = np.isfinite(want)
    _assert_same_values(got[fin], want[fin].astype(np.float32), "fast plane")
    over = (np.abs(A) >= 65520).any(axis=1)
    assert over.any() and not np.isfinite(got[over]).all(axis=1).any()
    x = torch.from_numpy(np.concatenate([A.ravel(), nonfinite_rows().ravel()]))
    h = ops.cast_f16(x[: x.numel() // 8 * 8].reshape(-1, 8).cuda()).cpu().ravel()
    w = x[: h.numel()].half()
    assert torch.equal(torch.isnan(h), torch.isnan(w)) and torch.equal(h[~torch.isnan(w)].view(torch.int16), w[~torch.isnan(w)].view(torch.int16))
    got, _ = _identity_gemm(ops, nonfinite_rows(), ops.PREC_F16)
    assert np.array_equal(np.isfinite(got), np.isfinite(nonfinite_rows().astype(np.float64) @ np.eye(64)))


# ---------------------------------------------------------------------------------------------------------------------------
# GEMM, componentwise:  |got - want| <= c |A||W|^T + a (1^T|W|) + epilogue terms
# ---------------------------------------------------------------------------------------------------------------------------
def _acts(ops):
    return {ops.ACT_NONE: (lambda x: x, 1.0), ops.ACT_QUICKGELU: (lambda x: x * torch.sigmoid(1.702 * x), 1.2),
            ops.ACT_GELU_ERF: (F.gelu, 1.2), ops.ACT_TANH: (torch.tanh, 1.0), ops.ACT_RELU: (torch.relu, 1.0)}


def gemm_bound(mode, K, A, W, w_exact):
    """(relative c, absolute per-|w| a) of one output: the planes' loss per operand plus fp32 accumulation (sqrt(K) u, x2)"""
    acc = 2.0 * np.sqrt(K) * U
    if mode == "f32":
        return 2.0 ** -21 + (0.0 if w_exact else 2.0 ** -22) + acc, 2.0 ** -23
    if mode == "f32x":
        return acc + 2 * U, 0.0
    return 2.0 ** -11 + (0.0 if w_exact else 2.0 ** -11) + acc, 2.0 ** -24


def check_gemm(ops, mode, A, W, bias=None, res=None, act=0, rows=None, pad=0, what=""):
    """run gemm_nt and check every element (or the given rows) against float64 with the componentwise bound; pad > 0 passes A as
    a strided view (row stride K + pad) of a wider device tensor"""
    prec = ops._NAMES[mode]
    Ad = torch.cat([A, torch.full((A.shape[0], pad), float("nan"))], 1).cuda()[:, :A.shape[1]] if pad else A.cuda()
    assert Ad.stride(0) == A.shape[1] + pad
    out = ops.gemm_nt(Ad, W.cuda(), None if bias is None else bias.cuda(), residual=None if res is None else res.cuda(), act=act,
                      precision=prec).cpu()
    if rows is not None:
        A, out = A[rows], out[rows]
        res = None if res is None else res[rows]
    K = A.shape[1]
    w_exact = torch.equal(W.half().float(), W)
    c, a = gemm_bound(mode, K, A, W, w_exact)
    Ad64, Wd64 = A.double(), W.double()
    pre = Ad64 @ Wd64.t() + (0 if bias is None else bias.double())
    pre_bound = c * N.gemm_abs(A, W) + a * Wd64.abs().sum(1)[None, :] + (0 if bias is None else U * bias.double().abs())
    if mode == "f32" and not w_exact:
        pre_bound = pre_bound + 2.0 ** -24 * Ad64.abs().sum(1)[:, None]           # the weight's own lo plane turns subnormal
    fn, slope = _acts(ops)[act]
    y = fn(pre)
    want = y + (0 if res is None else res.double())
    bound = slope * pre_bound + 8 * U * (pre.abs() + y.abs() + (0 if res is None else res.double().abs())) + 1e-37
    err = (out.double() - want).abs()
    ratio = float((err / bound).max())
    assert ratio <= 1.0, "%s %s: max err/bound %.3g (max err %.3g)" % (what, mode, ratio, float(err.max()))
    return ratio


def scaled_rows(M, K, gen, lo=-20, hi=15):
    """rows at scales 2^lo .. 2^hi (|A| < 65504 everywhere: randn clamped to +-1.9 times at most 2^15)"""
    e = torch.randint(lo, hi + 1, (M, 1), generator=gen).float()
    return torch.randn(M, K, generator=gen).clamp(-1.9, 1.9) * torch.exp2(e)


@pytest.mark.parametrize("mode", ["f32", "f32x", "f16"])
@pytest.mark.parametrize("w_kind", ["fp16_exact", "full_mantissa"])
def test_gemm_componentwise_scales_outliers_cancellation(ops, mode, w_kind):
    gen = g_(21)
    for M, N_, K in ((257, 193, 768), (33, 64, 32), (130, 129, 3072)):
        W = torch.randn(N_, K, generator=gen) * 0.05
        if w_kind == "fp16_exact":
            W = W.half().float()
        lo = -20 if mode != "f16" else -10                                    # fast mode: keep clear of fp16 subnormals
        A = scaled_rows(M, K, gen, lo=lo)
        A[:, 5] = 6.0e4 * torch.sign(torch.randn(M, generator=gen))          # outlier K-columns up to 6e4
        A[:, K // 2] = -5.9e4
        check_gemm(ops, mode, A, W, what="scales %dx%dx%d" % (M, N_, K))
        # cancellation: W = [W0 | W0], A = [a | -a (1 + d)]: outputs near 0, |A||W| large
        W0 = W[:, :K // 2]
        Wc = torch.cat([W0, W0], 1)
        a = torch.randn(M, K // 2, generator=gen) * 100
        Ac = torch.cat([a, -a * (1 + 1e-3 * torch.randn(M, K // 2, generator=gen))], 1)
        check_gemm(ops, mode, Ac, Wc, what="cancel %dx%dx%d" % (M, N_, K))


@pytest.mark.parametrize("mode", ["f32", "f32x", "f16"])
def test_gemm_componentwise_epilogues_and_strided_a(ops, mode):
    gen = g_(22)
    M, N_, K = 301, 255, 96
    W = (torch.randn(N_, K, generator=gen) * 0.1).half().float()
    bias, res = torch.randn(N_, generator=gen), torch.randn(M, N_, generator=gen) * 10
    A = torch.randn(M, K, generator=gen) * 2
    for act in range(5):
        check_gemm(ops, mode, A, W, bias, res, act, what="act %d" % act)
    check_gemm(ops, mode, scaled_rows(M, K, gen, lo=-8, hi=8), W, bias, None, ops.ACT_TANH, pad=8, what="strided A")


# One ragged (M, N, K) per tile instance of k_gemm_g16 that the tile rules of gemm_planes (xmh_gemm.hip) reach on the MI355X's 256
# CUs, with the tile each mode must run on.  Names: g16_<TBM>x<TBN>_w<waves>_a<A planes>w<W planes>_bk<BK> (xmh_gemm.hip,
# g16_tile_name), read back through prof_read.  Parity mode runs every shape twice: fp16-exact weights (two planes of A, one of W)
# and full-mantissa weights (the three-term product: 64x128 tiles up to two 128x128 tiles per CU, 128x128 above).  Four instances are
# unreachable with the shipped rules, each shadowed by an earlier rule for every grid it could take: parity's 128x128 BK 64 tiles
# (8 waves, and 4 waves with one block per CU) behind the 64x128 8-wave rule, fast mode's 64x128 2-wave and 128x128 4-wave BK 64 tiles behind
# the 64x128 and 128x128 8-wave rules.
TILES = [  # (M, N, K),          fast mode,                     parity mode, fp16-exact W,       parity, full-mantissa W
    ((20001, 2303, 768),  "g16_128x128_w8_a1w1_bk64",  "g16_128x256_w8_a2w1_bk32",  "g16_128x128_w8_a2w2_bk32"),
    ((4097, 3071, 2048),  "g16_256x256_w8_a1w1_bk64",  "g16_128x256_w8_a2w1_bk32",  "g16_128x128_w8_a2w2_bk32"),
    ((5001, 2303, 768),   "g16_192x128_w4_a1w1_bk64",  "g16_128x192_w4_a2w1_bk32",  "g16_128x128_w8_a2w2_bk32"),
    ((5003, 769, 3072),   "g16_128x128_w8_a1w1_bk64",  "g16_64x128_w8_a2w1_bk64",   "g16_64x128_w8_a2w2_bk32"),
    ((3201, 513, 2048),   "g16_64x128_w8_a1w1_bk64",   "g16_64x128_w8_a2w1_bk64",   "g16_64x128_w8_a2w2_bk32"),
    ((1601, 2049, 96),    "g16_128x128_w4_a1w1_bk32",  "g16_128x128_w4_a2w1_bk32",  "g16_64x128_w8_a2w2_bk32"),
    ((301, 511, 96),      "g16_64x128_w2_a1w1_bk32",   "g16_64x128_w2_a2w1_bk32",   "g16_64x128_w8_a2w2_bk32"),
    ((127, 65, 32),       "g16_64x128_w2_a1w1_bk32",   "g16_64x128_w2_a2w1_bk32",   "g16_64x128_w8_a2w2_bk32"),
]


@pytest.mark.parametrize("w_kind", ["fp16_exact", "full_mantissa"])
@pytest.mark.parametrize("mode", ["f32", "f16"])
@pytest.mark.parametrize("shape,fast_tile,parity_tile,parity3_tile", TILES, ids=["%dx%dx%d" % t[0] for t in TILES])
def test_gemm_componentwise_ragged_tiles(ops, shape, fast_tile, parity_tile, parity3_tile, mode, w_kind):
    from xmh import _lib
    M, N_, K = shape
    gen = g_(M + N_ + K)
    W = torch.randn(N_, K, generator=gen) * 0.05
    if w_kind == "fp16_exact":
        W = W.half().float()
    A = scaled_rows(M, K, gen, lo=-6, hi=6)
    bias = torch.randn(N_, generator=gen)
    rows = None                                                                 # large M: first rows, a sample, the edge tiles' rows
    if M > 600:
        rows = torch.cat([torch.arange(0, 160), torch.randint(160, M - 300, (64,), generator=gen), torch.arange(M - 300, M)])
    tile = fast_tile if mode == "f16" else parity_tile if w_kind == "fp16_exact" else parity3_tile
    _lib.prof_enable(True)
    try:
        check_gemm(ops, mode, A, W, bias, None, ops.ACT_QUICKGELU, rows=rows, what="tiles %dx%dx%d" % shape)
        torch.cuda.synchronize()
        ran = _lib.prof_read(tile)[1]
    finally:
        _lib.prof_enable(False)
    assert ran == 1, (tile, ran)                                                # the one launch ran on the intended tile


# ---------------------------------------------------------------------------------------------------------------------------
# LayerNorm: per element against float64
# ---------------------------------------------------------------------------------------------------------------------------
def ln_bound(x, gamma, D, y64):
    """fp32 two-pass LayerNorm: mean to 24 u mean|x| (sums of <= 16 terms per lane, then 6 tree levels), variance and rsqrt to
    a few u, plus the error the mean's error carries into the variance"""
    x = x.double()
    m = x.mean(1, keepdim=True)
    var = ((x - m) ** 2).mean(1, keepdim=True)
    rstd = (var + 1e-5).rsqrt()
    e_mean = 24 * U * x.abs().mean(1, keepdim=True)
    e_r = 0.5 * (e_mean * rstd) ** 2 + 24 * U
    xhat = (x - m) * rstd
    g = gamma.double().abs()[None, :]
    return 2 * (g * rstd * (e_mean + 2 * U * (x - m).abs()) + g * xhat.abs() * (e_r + 3 * U) + 2 * U * y64.abs()) + 1e-37


@pytest.mark.parametrize("D", [768, 512, 1024, 77, 513, 1023])
def test_layernorm_componentwise_hard_rows(ops, D):
    gen = g_(D)
    rows = [torch.randn(D, generator=gen) * 1e-2 + 1e3,                        # a one-pass variance would cancel to nothing
            torch.randn(D, generator=gen) * 1e-2 - 1e3,
            torch.randn(D, generator=gen), torch.full((D,), 3.0), torch.full((D,), 0.1), torch.zeros(D),   # var 0: rsqrt(eps)
            torch.randn(D, generator=gen) * 1e-6, torch.randn(D, generator=gen) * 1e-3 + 5.0,             # tiny variance
            torch.randn(D, generator=gen) * 3 + 0.5]
    massive = torch.randn(D, generator=gen)
    massive[D // 3] = 1e4                                                        # one massive channel
    rows.append(massive)
    x = torch.stack(rows)
    x = torch.cat([x, torch.randn(37, D, generator=gen) * torch.exp(torch.randn(37, 1, generator=gen) * 3)])
    gamma, beta = 1 + 0.1 * torch.randn(D, generator=gen), 0.1 * torch.randn(D, generator=gen)
    gamma[D // 3] = 0.01
    got = ops.layernorm(x.cuda(), gamma.cuda(), beta.cuda()).cpu().double()
    want = F.layer_norm(x.double(), (D,), gamma.double(), beta.double(), 1e-5)
    ratio = ((got - want).abs() / ln_bound(x, gamma, D, want)).amax(1)
    assert float(ratio.max()) <= 1.0, [round(float(r), 3) for r in ratio[:10]]
    assert torch.equal(got[[3, 5]].float(), beta.expand(2, D))                 # constant rows with an exact mean: exactly beta


def test_layernorm_width_limit(ops):
    from xmh._lib import XmhError
    x = torch.randn(4, 1025).cuda()
    with pytest.raises(XmhError):
        ops.layernorm(x, torch.ones(1025).cuda(), torch.zeros(1025).cuda())


# ---------------------------------------------------------------------------------------------------------------------------
# attention: per element, relative to sum_j P_j |v_j|, with the softmax argument's error u_s sum|q||k_j|
# ---------------------------------------------------------------------------------------------------------------------------
def attn_reference(qkv, H, causal, kpm):
    B, L, D3 = qkv.shape
    q, k, v = [t.view(B, L, H, 64).transpose(1, 2).double() for t in qkv.chunk(3, -1)]
    q = q * 0.125
    s = q @ k.transpose(-1, -2)
    sa = q.abs() @ k.abs().transpose(-1, -2)
    dead = torch.zeros(B, 1, L, L, dtype=torch.bool)
    if causal:
        dead = dead | torch.ones(L, L, dtype=torch.bool).triu(1)
    if kpm is not None:
        dead = dead | kpm[:, None, None, :]
    s = s.masked_fill(dead, float("-inf"))
    p = torch.softmax(s, -1)
    want = (p @ v).transpose(1, 2).reshape(B, L, -1)
    pv = (p @ v.abs()).transpose(1, 2).reshape(B, L, -1)
    vsum = (torch.ones_like(p).masked_fill(dead, 0) @ v.abs()).transpose(1, 2).reshape(B, L, -1)
    ds = sa.masked_fill(dead, 0).amax(-1, keepdim=True)                         # max_j sum |q||k_j| per query row
    qk1 = (q.abs().sum(-1, keepdim=True) + k.abs().sum(-1)[:, :, None, :].masked_fill(dead, 0).amax(-1, keepdim=True))

    def per_channel(t):                                                         # [B, H, L, 1] -> [B, L, H * 64]
        return t.expand(-1, -1, -1, 64).transpose(1, 2).reshape(B, L, -1)
    return want, pv, vsum, per_channel(ds), per_channel(qk1)


def attn_cases():
    g = g_(31)
    cases = []
    for L, causal in ((50, False), (32, True), (64, False), (77, True), (128, False), (33, False)):
        B, H = 3, 2
        qkv = torch.randn(B, L, 3 * 128, generator=g)
        q, k, v = qkv[..., :128], qkv[..., 128:256], qkv[..., 256:]
        q.mul_(7.0)
        k.mul_(7.0)                                                              # logits ~ +-50 .. +-200
        k[0, 3] = k[0, 1]                                                        # exact ties at the row max in sample 0
        q[0, :, :] = q[0, :, :].abs()
        k[0, 1] = k[0, 1].abs()
        k[0, 3] = k[0, 1]
        v[1] *= 1e-6                                                             # V at 1e-6
        v[2, :, 5] *= 1e3                                                        # V outlier channels
        v[2, :, 64 + 9] *= -2e3
        kpm = torch.zeros(B, L, dtype=torch.bool)
        kpm[1, 2:5] = True                                                       # holes in the middle
        kpm[1, L // 2] = True
        kpm[2, L - 3:] = True
        if causal:
            kpm[2, 0] = True                                                     # causal + padding: query 0 of sample 2 sees nothing
        cases.append((qkv, L, causal, kpm))
    return cases


@pytest.mark.parametrize("mode", ["f32", "f32x"])        # fast mode runs the parity kernel (ops.attention: split16 unless f32x)
def test_attention_componentwise_logits_ties_masks(ops, mode):
    before = ops.get_precision()
    ops.set_precision(mode)
    try:
        for qkv, L, causal, kpm in attn_cases():
            got = ops.attention(qkv.cuda(), 2, causal=causal, key_padding_mask=kpm.cuda()).cpu().double()
            want, pv, vsum, ds, qk1 = attn_reference(qkv, 2, causal, kpm)
            nan = torch.isnan(want)
            assert torch.equal(torch.isnan(got), nan), (mode, L, causal)       # fully masked rows: NaN, as the float64 reference
            if causal:
                assert bool(nan[2, 0].all()) and int(nan.sum()) == 128
            split = mode != "f32x"
            cs = 1.5 * 2.0 ** -20 if split else 2.0 ** -20
            ds_err = cs * ds + (2.0 ** -23 * qk1 if split else 0)                # error of the softmax arguments
            cpv = 2.0 ** -19 if split else 2.0 ** -20
            bound = 2 * (2 * ds_err + 16 * U) * pv + cpv * pv + (2.0 ** -23 * (vsum + 1) if split else 0) + 1e-37
            err = (got - want).abs()
            ratio = (err / bound)[~nan]
            assert float(ratio.max()) <= 1.0, (mode, L, causal, float(ratio.max()))
    finally:
        ops.set_precision(before)


# ---------------------------------------------------------------------------------------------------------------------------
# whole towers against the float64 oracle
# ---------------------------------------------------------------------------------------------------------------------------
SEED = 1814
# Measured on the MI355X (per-row error against float64, worst output of each tower; the fp32 CPU oracle's own error in brackets):
#   parity  synthetic 9.2e-7 .. 1.4e-6 (5.6e-7 .. 1.6e-6)   outlier 7.9e-7 .. 1.1e-5 (9.0e-7 .. 6.7e-6)
#   exact   synthetic 1.0e-6 .. 2.1e-6                      outlier 1.5e-6 .. 5.4e-6
#   fast    synthetic 3.0e-4 .. 8.1e-4                      outlier 2.9e-4 .. 9.4e-3
PARITY_K, PARITY_FLOOR = 4.0, 1e-6               # parity / exact: err <= K x (fp32 CPU oracle's err) + FLOOR
FAST_BAND = {"synth": (1e-4, 2e-3), "outlier": (1e-4, 2e-2)}    # fast mode: per-row error inside this band; parity is below 1.1e-5
SENS_LAYER = 5                                   # the block whose fp16-rounded GEMM inputs must fail the parity tolerance 5x over


@pytest.fixture(scope="module")
def towers(ops):
    from oracle import encode as enc
    from xmh.models import weights as W
    from xmh.models.clip import build_model
    threads = torch.get_num_threads()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    image = W.synth_images(SEED, 2)
    ids, _ = W.synth_text(SEED, 4)                                               # 25, 7, 30, 27 of 32 tokens: the packed forms pay
    kpm = ids == 0
    kpm[1, 2] = True                                                             # a hidden token in front of EOS
    out = {}
    try:
        for kind in ("synth", "outlier"):
            raw = W.synth_clip_state_dict(SEED) if kind == "synth" else N.outlier_clip_state_dict(SEED)
            sd32 = enc.fp16_round_like_reference(raw)
            sd64 = N.f64(sd32)
            r = {}
            with torch.no_grad():
                rec = []
                with N.linear_probe(record=rec):
                    r["img64"] = enc.clip_image(sd64, image.double(), return_patches=True)
                    r["txt64"] = enc.clip_text(sd64, ids, key_padding_mask=kpm, return_patches=True)
                r["max_operand"] = max(max(a, b) for a, b in rec)
                r["eos64"] = enc.clip_text(sd64, ids)                            # no key padding mask: exact mode's packed form
                r["img32"] = enc.clip_image(sd32, image, return_patches=True)
                r["txt32"] = enc.clip_text(sd32, ids, key_padding_mask=kpm, return_patches=True)
                r["eos32"] = enc.clip_text(sd32, ids)
                with N.linear_probe(round_calls=N.block_calls(SENS_LAYER)):
                    r["img_sens"] = enc.clip_image(sd64, image.double(), return_patches=True)
                with N.linear_probe(round_calls=N.block_calls(SENS_LAYER)):
                    r["txt_sens"] = enc.clip_text(sd64, ids, key_padding_mask=kpm, return_patches=True)
                with N.linear_probe(round_calls=N.block_calls(SENS_LAYER)):
                    r["eos_sens"] = enc.clip_text(sd64, ids)
            r["model_rp"] = build_model(raw, return_patches=True).cuda()          # CLS / EOS and the token outputs
            r["model"] = build_model(raw).cuda()                                  # CLS / EOS only
            out[kind] = r
    finally:
        torch.set_num_threads(threads)
    return {"image": image, "ids": ids, "kpm": kpm, **out}


class _TextEntrySpy:
    """stands in for the library handle of xmh.models.clip while a text tower runs: counts the calls of the text tower's entry
    points and forwards every call"""
    NAMES = ("xmh_text_forward", "xmh_text_forward_packed", "xmh_text_forward_packed_dev")

    def __init__(self, lib):
        self.lib, self.calls = lib, dict.fromkeys(self.NAMES, 0)

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if name not in self.NAMES:
            return fn

        def counted(*args):
            self.calls[name] += 1
            return fn(*args)
        return counted


def _tower_outputs(ops, towers, kind, mode):
    """(name, got, want64, want32, want_sens) per output: image CLS and tokens; text EOS and the kept token rows through the padded
    entry point (xmh_text_forward) and through the packed one the product path takes -- xmh_text_forward_packed_dev in parity and
    fast mode (key padding mask, token rows behind the last visible position zero), xmh_text_forward_packed (no mask) in exact mode"""
    import xmh.models.clip as C
    r = towers[kind]
    ids, kpm = towers["ids"].cuda(), towers["kpm"].cuda()
    keep = ~r["txt64"][2].T                                                      # [L, B]: rows neither padding nor EOS
    res = []
    before, spy = ops.get_precision(), _TextEntrySpy(C.lib)
    assert C.TEXT_PACKING and C.NATIVE_FORWARD
    ops.set_precision(mode)
    C.lib = spy
    try:
        cls, tok, _ = r["model_rp"].encode_image(towers["image"].cuda())
        res += [("img_cls", cls, r["img64"][0], r["img32"][0], r["img_sens"][0]),
                ("img_tok", tok, r["img64"][1], r["img32"][1], r["img_sens"][1])]
        eos, ttok, _, nm = r["model_rp"].encode_text(ids, key_padding_mask=kpm)
        assert torch.equal(nm.cpu(), r["txt64"][2]) and spy.calls["xmh_text_forward"] == 1
        res += [("txt_eos/padded", eos, r["txt64"][0], r["txt32"][0], r["txt_sens"][0]),
                ("txt_tok/padded", ttok.cpu()[keep], r["txt64"][1][keep], r["txt32"][1][keep], r["txt_sens"][1][keep])]
        if mode == "f32x":
            eos = r["model"].encode_text(ids)
            assert spy.calls["xmh_text_forward_packed"] == 1
            res += [("txt_eos/packed", eos, r["eos64"], r["eos32"], r["eos_sens"])]
        else:
            eos, ttok, _, nm = r["model_rp"].encode_text(ids, key_padding_mask=kpm, masked_rows="zero")
            assert torch.equal(nm.cpu(), r["txt64"][2])
            eos_only = r["model"].encode_text(ids, key_padding_mask=kpm)
            assert spy.calls["xmh_text_forward_packed_dev"] == 2
            res += [("txt_eos/packed", eos, r["txt64"][0], r["txt32"][0], r["txt_sens"][0]),
                    ("txt_eos_only/packed", eos_only, r["txt64"][0], r["txt32"][0], r["txt_sens"][0]),
                    ("txt_tok/packed", ttok.cpu()[keep], r["txt64"][1][keep], r["txt32"][1][keep], r["txt_sens"][1][keep])]
        assert spy.calls["xmh_text_forward"] == 1                                # nothing fell back to the padded entry point
    finally:
        C.lib = spy.lib
        ops.set_precision(before)
    return res


@pytest.mark.parametrize("kind", ["synth", "outlier"])
@pytest.mark.parametrize("mode", ["f32", "f32x", "f16"])
def test_towers_against_float64(ops, towers, kind, mode):
    assert towers[kind]["max_operand"] < N.F16_MAX                            # every GEMM operand inside the fp16 range
    rows = []
    for name, got, w64, w32, sens in _tower_outputs(ops, towers, kind, mode):
        cpu32 = N.rel_rows(w32, w64)
        rows.append(("%s %s %s" % (kind, mode, name), N.rel_rows(got, w64), PARITY_K * cpu32 + PARITY_FLOOR, N.rel_rows(sens, w64), cpu32))
    print("".join("\n%s: err %.3g tol %.3g one-block-fp16 %.3g cpu-fp32 %.3g" % r for r in rows))
    for what, err, tol, sens, _ in rows:
        assert sens >= 5 * tol, (what, sens, tol)                               # the tolerance would see one block in fp16
        if mode == "f16":
            assert FAST_BAND[kind][0] < err < FAST_BAND[kind][1], (what, err)  # near the fp16 level, and fast mode really ran
        else:
            assert err <= tol, (what, err, tol)


def test_fast_mode_code_bits_against_float64(ops, towers):
    r = towers["synth"]
    proj = torch.randn(512, 64, generator=g_(1)).double()
    before = ops.get_precision()
    ops.set_precision("f16")
    try:
        cls = r["model"].encode_image(towers["image"].cuda())
    finally:
        ops.set_precision(before)
    flips = ((cls.cpu().double() @ proj).sign() != (r["img64"][0] @ proj).sign()).double().mean().item()
    assert flips < 0.01
