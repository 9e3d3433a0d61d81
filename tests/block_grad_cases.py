"""Shared by tools/make_golden_block_grad.py, tests/test_block_grad_cpu.py and tests/test_gpu_block_grad.py (not a test module): the
cases of the CLIP block-stack backward (shapes, seeded parameters, inputs, upstream gradients and key padding masks), the float64
restatement -- torch autograd over oracle.encode._blocks with the parameters as leaves -- and the error measure of the golden file.

The reference's own Transformer cannot serve as the float64 side (its LayerNorm casts to fp32 and refuses double parameters); its
fp32 run is what tests/golden/block_grad.npz stores, and the fp32 run of the restatement here equals it to the bit at the committed
shapes (asserted by the generator).  Runs here use one CPU thread, so that the fp32 bits do not depend on how many a machine has.

Tensor kinds: y (the stack's output), g_x, and g_<parameter> for the twelve parameters of a block (pooled over the layers).  Stored
tensors of more than FULL elements keep every THIN-th flat element (`thin`); the error measure e = max|x - fp64| / max|fp64| is
always taken on whole tensors."""
import os
import zlib

import numpy as np
import torch

from oracle import encode as enc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "block_grad.npz")
FULL, THIN = 256, 16
SEED = 1814

# parameter kinds in the member order of xmh_clip_block_grads -> key under resblocks.<i>.
PARAMS = (("ln1_w", "ln_1.weight"), ("ln1_b", "ln_1.bias"), ("qkv_w", "attn.in_proj_weight"), ("qkv_b", "attn.in_proj_bias"),
          ("out_w", "attn.out_proj.weight"), ("out_b", "attn.out_proj.bias"), ("ln2_w", "ln_2.weight"), ("ln2_b", "ln_2.bias"),
          ("fc_w", "mlp.c_fc.weight"), ("fc_b", "mlp.c_fc.bias"), ("proj_w", "mlp.c_proj.weight"), ("proj_b", "mlp.c_proj.bias"))
KINDS = ("y", "g_x") + tuple("g_" + k for k, _ in PARAMS)

# name -> (D, heads, layers, L, B, causal, key padding)
CASES = {
    "d64_l1_b1": (64, 1, 1, 1, 1, False, False),
    "d128_l7_b3_causal": (128, 2, 2, 7, 3, True, False),
    "d192_l50_b2": (192, 3, 2, 50, 2, False, False),
    "d128_l65_b2": (128, 2, 2, 65, 2, False, False),
    "d64_l33_b5_causal_kpm": (64, 1, 3, 33, 5, True, True),
}


def case_seed(name):
    return SEED + 10 * sorted(CASES).index(name)


def _shape(key, D):
    if key.endswith("in_proj_weight"):
        return (3 * D, D)
    if key.endswith("in_proj_bias"):
        return (3 * D,)
    if key.endswith("c_fc.weight"):
        return (4 * D, D)
    if key.endswith("c_fc.bias"):
        return (4 * D,)
    if key.endswith("c_proj.weight"):
        return (D, 4 * D)
    if key.endswith("out_proj.weight"):
        return (D, D)
    return (D,)


def draw_params(seed, D, layers):
    """state_dict of a block stack under the reference's key names: LayerNorm weights around 1, matrices sigma 0.05, vectors sigma 0.1"""
    sd = {}
    for i in range(layers):
        for t, (_, key) in enumerate(PARAMS):
            rng = np.random.default_rng([seed, 7, i, t])
            shape = _shape(key, D)
            if len(shape) == 2:
                v = 0.05 * rng.standard_normal(shape)
            elif key in ("ln_1.weight", "ln_2.weight"):
                v = 1.0 + 0.1 * rng.standard_normal(shape)
            else:
                v = 0.1 * rng.standard_normal(shape)
            sd["resblocks.%d.%s" % (i, key)] = v.astype(np.float32)
    return sd


def draw_batch(seed, B, L, D):
    """x and the upstream gradient, [B, L, D] fp32"""
    rng = np.random.default_rng([seed, 11])
    return rng.standard_normal((B, L, D)).astype(np.float32), rng.standard_normal((B, L, D)).astype(np.float32)


def draw_kpm(seed, B, L):
    """[B, L] bool, True = the key is hidden; key 0 never is, so every query keeps a visible key under the causal mask too"""
    m = np.random.default_rng([seed, 13]).random((B, L)) < 0.3
    m[:, 0] = False
    return m


def case_inputs(name):
    D, heads, layers, L, B, causal, kp = CASES[name]
    seed = case_seed(name)
    x, up = draw_batch(seed, B, L, D)
    return draw_params(seed, D, layers), x, up, (draw_kpm(seed, B, L) if kp else None)


def checksum(arrays):
    c = 0
    for a in arrays:
        c = zlib.crc32(np.ascontiguousarray(a).tobytes(), c)
    return float(c)


def inputs_checksum(sd, x, up, kpm):
    return checksum([sd[k] for k in sorted(sd)] + [x, up] + ([] if kpm is None else [kpm.astype(np.uint8)]))


def additive_mask(B, L, causal, kpm, dtype):
    """[B, L, L] additive mask of the restatement (-inf where a key is hidden), or None"""
    if not causal and kpm is None:
        return None
    m = torch.zeros(B, L, L, dtype=dtype)
    if causal:
        m = m + torch.full((L, L), float("-inf"), dtype=dtype).triu_(1)
    if kpm is not None:
        m = m.masked_fill(torch.as_tensor(kpm)[:, None, :], float("-inf"))
    return m


def run_restatement(sd, x, up, heads, causal, kpm, dtype):
    """(y . up).sum().backward() over oracle.encode._blocks in `dtype` -> {kind or g_l<i>_<param>: numpy array}; y and g_x [B, L, D]"""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        t = {k: torch.tensor(v).to(dtype).requires_grad_(True) for k, v in sd.items()}
        xt = torch.tensor(x).to(dtype).requires_grad_(True)
        B, L, _ = xt.shape
        layers = len({k.split(".")[1] for k in sd})
        y = enc._blocks(xt.transpose(0, 1), t, "", layers, heads, additive_mask(B, L, causal, kpm, dtype)).transpose(0, 1)
        (y * torch.tensor(up).to(dtype)).sum().backward()
        out = {"y": y.detach().numpy().copy(), "g_x": xt.grad.numpy().copy()}
        for i in range(layers):
            for kind, key in PARAMS:
                out["g_l%d_%s" % (i, kind)] = t["resblocks.%d.%s" % (i, key)].grad.numpy().copy()
        return out
    finally:
        torch.set_num_threads(threads)


def kind_of(tensor):
    """y, g_x, g_l<i>_<param> -> its kind"""
    return tensor if tensor in ("y", "g_x") else "g_" + tensor.split("_", 2)[2]


def rel_err(x, ref):
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(x - ref).max()) / (float(np.abs(ref).max()) or 1.0)


def thin(a):
    a = np.asarray(a).reshape(-1)
    return a if a.size <= FULL else a[::THIN]


def erefs(r32, r64):
    """per tensor and pooled (max) per kind"""
    per = {k: rel_err(r32[k], r64[k]) for k in r64}
    pool = {}
    for k, e in per.items():
        pool[kind_of(k)] = max(pool.get(kind_of(k), 0.0), e)
    return per, pool


_golden = None


def golden():
    global _golden
    if _golden is None:
        _golden = dict(np.load(GOLDEN))
    return _golden


def pool_eref(kind):
    """max of the stored e_ref over every committed case and layer of this tensor kind"""
    G = golden()
    vals = [float(v) for k, v in G.items() if "__eref_" in k and kind_of(k.split("__eref_")[1]) == kind]
    assert vals, kind
    return max(vals)

