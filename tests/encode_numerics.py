"""Shared numerics for the encoder tests: float64 references, per-row / componentwise error measures, a CPU emulation of the
fp16 operand planes (csrc/xmh_planes.h) and an "outlier" variant of the synthetic CLIP weights.  Imported like conftest.

Nothing here runs on the GPU; the GPU tests (tests/test_gpu_encode_numerics.py) and the CPU tests
(tests/test_encode_numerics_cpu.py) both use it."""
from __future__ import annotations

import contextlib
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from oracle import encode as enc

F16_MAX = 65504.0


# ---------------------------------------------------------------------------------------------------------------------------
# error measures
# ---------------------------------------------------------------------------------------------------------------------------
def rel_rows(got, want) -> float:
    """max over rows of  max|got - want|_row / max|want|_row  (a row: the last dimension -- one sample's embedding or one token).
    Unlike a global max|err| / max|want|, a wrong row whose values are small next to the largest output still shows."""
    got = torch.as_tensor(got).detach().cpu().double()
    want = torch.as_tensor(want).detach().cpu().double()
    assert got.shape == want.shape, (got.shape, want.shape)
    d = (got - want).abs().reshape(-1, want.shape[-1]).amax(dim=1)
    s = want.abs().reshape(-1, want.shape[-1]).amax(dim=1)
    return float((d / s.clamp_min(1e-300)).max())


def gemm_abs(A, W) -> torch.Tensor:
    """|A| . |W|^T in float64: the componentwise scale of every dot product of A [M, K] with W [N, K]."""
    return torch.as_tensor(A).detach().cpu().double().abs() @ torch.as_tensor(W).detach().cpu().double().abs().t()


# ---------------------------------------------------------------------------------------------------------------------------
# the operand planes, emulated bit for bit (xmh_planes.h: split2 for parity mode, round2 for fast mode)
# ---------------------------------------------------------------------------------------------------------------------------
def rtz_f16(x) -> np.ndarray:
    """float32 -> fp16 rounded toward zero, finite overflow saturating at +-65504 (v_cvt_pkrtz_f16_f32); inf and NaN pass."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    a = np.abs(x)
    with np.errstate(invalid="ignore", divide="ignore"):
        _, e = np.frexp(np.where(np.isfinite(a) & (a > 0), a, 1.0))       # a = m 2^e, m in [0.5, 1)
        q = np.exp2(np.maximum(e - 11, -24).astype(np.float64))           # fp16 quantum at that exponent (subnormal: 2^-24)
        t = np.floor(a / q) * q
    t = np.where(np.isfinite(a), np.minimum(t, F16_MAX), a)
    return (np.copysign(t, x)).astype(np.float16)


def split_planes(x):
    """parity-mode split of float32 x -> (hi, lo) fp16: hi = rtz_f16(x with its low 13 mantissa bits cleared),
    lo = rtz_f16(x - that masked value).  The exact bits split2 produces."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    hm = (x.view(np.uint32) & np.uint32(0xFFFFE000)).view(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        return rtz_f16(hm), rtz_f16(x - hm)


def split_value(x) -> np.ndarray:
    """float32(hi + lo): what a GEMM against the identity returns in parity mode"""
    hi, lo = split_planes(x)
    with np.errstate(invalid="ignore"):
        return (hi.astype(np.float64) + lo.astype(np.float64)).astype(np.float32)


def fast_value(x) -> np.ndarray:
    """fast mode's single plane (round2: round to nearest, inf from 65520 up), as float32"""
    with np.errstate(over="ignore"):
        return np.asarray(x, dtype=np.float32).astype(np.float16).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------
# float64 oracle runs
# ---------------------------------------------------------------------------------------------------------------------------
def f64(sd: dict) -> dict:
    return {k: v.double() for k, v in sd.items()}


@contextlib.contextmanager
def linear_probe(round_calls=(), record=None):
    """Patch F.linear for the duration: calls whose index (0, 1, 2, ... in call order) is in ``round_calls`` get their input
    rounded to fp16 (what a GEMM that lost its lo plane computes); ``record`` (a list) receives max|input| and max|output| of
    every call.  In the oracle's block stack the calls of layer i are 4i (in_proj), 4i+1 (out_proj), 4i+2 (c_fc), 4i+3 (c_proj)."""
    orig = F.linear
    calls = [0]

    def lin(x, w, b=None):
        i = calls[0]
        calls[0] += 1
        if i in round_calls:
            x = x.half().to(x.dtype)
        y = orig(x, w, b)
        if record is not None:
            record.append((float(x.abs().max()), float(y.abs().max())))
        return y
    F.linear = lin
    try:
        yield calls
    finally:
        F.linear = orig


@contextlib.contextmanager
def softmax_probe(record):
    """Patch torch.softmax for the duration: ``record`` (a list) receives every result (the oracle's attention probabilities,
    [batch * heads, L, L] per layer, in layer order)."""
    orig = torch.softmax

    def sm(x, dim=None, **kw):
        p = orig(x, dim=dim, **kw)
        record.append(p)
        return p
    torch.softmax = sm
    try:
        yield record
    finally:
        torch.softmax = orig


def block_calls(layer: int):
    return tuple(range(4 * layer, 4 * layer + 4))


# ---------------------------------------------------------------------------------------------------------------------------
# weights with the magnitudes of released CLIP checkpoints
# ---------------------------------------------------------------------------------------------------------------------------
# per tower; fc_scale / qk_scale: (layer 0, layers 1..): from layer 1 on the two massive channels dominate every LayerNorm's
# variance and shrink the other channels of its output, so those layers need larger factors for the same magnitudes
OUTLIER_SCALES = {"visual.transformer.": dict(residual=300.0, ln_gain=0.02, fc_neurons=3, fc_scale=(48.0, 768.0), qk_scale=(4.0, 40.0)),
                  "transformer.": dict(residual=300.0, ln_gain=0.02, fc_neurons=3, fc_scale=(48.0, 1536.0), qk_scale=(4.0, 112.0))}


def outlier_channels(width: int):
    return (width // 3 + 5, (2 * width) // 3 + 1)


def outlier_clip_state_dict(seed: int = 1814, **overrides) -> dict:
    """synth_clip_state_dict with what real CLIP weights do to activations, deterministically, in both towers:
      * two residual channels pushed to +-residual by layer 0's c_proj bias; every LayerNorm gain (ln_1, ln_2, ln_post /
        ln_final) is small on those channels, so the stream carries them from layer 0 to the end;
      * in every layer, fc_neurons c_fc rows scaled by fc_scale: pre-activations in the hundreds;
      * in every layer, one head (layer % heads) with its q and k rows scaled by qk_scale each: logits qk_scale^2 larger, a
        near one-hot softmax.
    The factors multiply the fp32 draws before fp16_round_like_reference (and build_model) round the GEMM weights to fp16, so the
    model and the oracle hold the same fp16 values."""
    from xmh.models import weights as W
    sd = W.synth_clip_state_dict(seed, **overrides)
    sd = {k: v.clone() for k, v in sd.items()}
    for prefix, final_ln in (("visual.transformer.", "visual.ln_post"), ("transformer.", "ln_final")):
        s = OUTLIER_SCALES[prefix]
        layers = enc._count_layers(sd, prefix)
        width = sd[final_ln + ".weight"].shape[0]
        heads = width // 64
        ch = list(outlier_channels(width))
        b = sd[prefix + "resblocks.0.mlp.c_proj.bias"]
        b[ch[0]], b[ch[1]] = s["residual"], -s["residual"]
        g = torch.Generator().manual_seed((seed * 7919 + zlib.crc32(prefix.encode())) % (2 ** 31))
        for i in range(layers):
            p = "%sresblocks.%d." % (prefix, i)
            for ln in ("ln_1", "ln_2"):
                sd[p + ln + ".weight"][ch] = s["ln_gain"]
            neurons = torch.randperm(4 * width, generator=g)[:s["fc_neurons"]]
            sd[p + "mlp.c_fc.weight"][neurons] *= s["fc_scale"][min(i, 1)]
            h = i % heads
            w_in = sd[p + "attn.in_proj_weight"]
            w_in[h * 64:(h + 1) * 64] *= s["qk_scale"][min(i, 1)]                       # q rows of head h
            w_in[width + h * 64:width + (h + 1) * 64] *= s["qk_scale"][min(i, 1)]       # k rows of head h
        sd[final_ln + ".weight"][ch] = s["ln_gain"]
    return sd
