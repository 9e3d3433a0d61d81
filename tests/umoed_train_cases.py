"""Cases, seeded draws and the float64 / float32 restatement of UMoED's decoder head in TRAIN mode (reference
models/UMoED/hash/block/transformer.py SoftMoEDecoderLayer with its six dropout sites per layer, hash/block/SoftMoe.py, hash/hash_moe.py
TokenHash), shared by tests/test_umoed_train_cpu.py, tests/test_gpu_umoed_train.py and tools/make_golden_umoed_train.py.
Built on tests/umoed_cases.py (head_params, head_shapes, compare, rel_err), which is not edited.

``head_train`` is umoed_cases.head with explicit keep masks (``t * keep / (1 - p)`` at drop1 .. drop6 of every layer; no mask: the very
operations of umoed_cases.head) and torch's autograd for the gradients of loss = sum(embeds * G).  Parameters, tokens, G and the masks
are drawn from seeds and never stored.

Keep-mask layout (the library's, include/xmh.h): per layer [B, H, M, M] (drop1, on the self-attention probabilities), [B M, d] (drop2),
[B, H, M, T] (drop3, on the cross-attention probabilities), [B M, d] (drop4), [B M, F] (drop5, behind the ReLU), [B M, d] (drop6); the
layers follow one another.

Guard: the ReLU mask is the one discontinuity between G and the gradients, so a case's seed is accepted only if, in float64 and in both
settings (no dropout, p = 0.3), every ReLU pre-activation satisfies |pre| >= RELU_GAP * max|pre| of its tensor -- a hundred float32 ulps.
``find_seed`` is how the seeds below were chosen (seed, seed + 1000, ... at most 8 redraws: edge 7401 and tiles 7402 at once, rows 7403 at
its third redraw, 10403; the golden case 7405 at once); they are fixed here and the CPU test verifies the guard for each.

Error rule (umoed_cases.compare): per tensor e = max|got - f64| / max|f64| <= 4 * max(e_ref of this tensor, pool of its kind), e_ref the
float32 restatement's e on the same inputs, the pool the largest e_ref over every case and setting for that kind of tensor (a
parameter's kind is its name without the layer index)."""
import functools
import math
import os
import re
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

import umoed_cases as UC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "umoed_train.npz")
P_DROP = 0.3
RELU_GAP = 1e-5
MAX_REDRAWS = 8
# B, T, E = d, heads, M, layers, n x p, F, V.  edge: one head, one layer, everything below a tile.  tiles: M = 70 crosses the 64-row tile and
# the wave, 3 x 5 slots, two layers (the residual stream, d_tokens summed over layers).  rows: B M = 296 and B P = 111 reduction rows cross
# the product's 32-row slab, and grad::tn_split cuts the [64, 64] weight gradients over 296 rows into 5 chunks of 64.
TRAIN_CASES = {
    "edge": dict(B=3, T=7, E=64, d=64, heads=1, M=5, layers=1, n=2, p=2, F=24, V=2, moe=True, hash_func="linear_subspace", seed=7401),
    "tiles": dict(B=2, T=50, E=128, d=128, heads=2, M=70, layers=2, n=3, p=5, F=96, V=16, moe=True, hash_func="linear_subspace", seed=7402),
    "rows": dict(B=37, T=33, E=64, d=64, heads=1, M=8, layers=2, n=2, p=3, F=40, V=4, moe=True, hash_func="linear_subspace", seed=10403),
}
# what the unmodified reference can build (its dim_feedforward is always 2048): two layers at the smallest width
GOLDEN_CASE = dict(B=2, T=5, E=64, d=64, heads=1, M=3, layers=2, n=2, p=2, F=2048, V=2, moe=True, hash_func="linear_subspace", seed=7405)
SETTINGS = ("p0", "p03")                     # no dropout; p = 0.3 with masks drawn from the case's seed
# The golden file keeps a tensor whole up to GOLDEN_WHOLE elements and otherwise GOLDEN_SAMPLE of them at seeded positions with the
# tensor's sum and sum of squares: F = 2048 makes the experts' gradient alone a megabyte.
GOLDEN_WHOLE, GOLDEN_SAMPLE = 256, 64


def keep_shapes(c):
    """the six sections of one layer, in the library's order"""
    B, H, M, T, d, F_ = c["B"], c["heads"], c["M"], c["T"], c["d"], c["F"]
    return [(B, H, M, M), (B, M, d), (B, H, M, T), (B, M, d), (B, M, F_), (B, M, d)]


def draw_masks(c, seed, p=P_DROP):
    """-> [layers][6] uint8 arrays, Bernoulli(1 - p)"""
    rng = np.random.default_rng(seed + 900)
    return [[(rng.random(s) >= p).astype(np.uint8) for s in keep_shapes(c)] for _ in range(c["layers"])]


def flat_keep(masks):
    """the library's one buffer"""
    return np.concatenate([m.reshape(-1) for layer in masks for m in layer])


def _mha(q_in, kv_in, in_w, in_b, out_w, out_b, heads, drop):
    d = q_in.shape[-1]
    dh = d // heads
    q = q_in @ in_w[:d].t() + in_b[:d]
    k = kv_in @ in_w[d:2 * d].t() + in_b[d:2 * d]
    v = kv_in @ in_w[2 * d:].t() + in_b[2 * d:]
    split = lambda t: t.reshape(t.shape[0], t.shape[1], heads, dh).transpose(1, 2)            # noqa: E731
    s = (split(q) / math.sqrt(dh)) @ split(k).transpose(-1, -2)
    o = (drop(torch.softmax(s, dim=-1)) @ split(v)).transpose(1, 2).reshape(q.shape)
    return o @ out_w.t() + out_b


def forward_train(mem, W, c, masks=None, p=0.0, probe=None):
    """torch tensors of one dtype -> embeds [B, M, V] with a graph.  masks: draw_masks' lists (or None: no dropout, umoed_cases.head's
    operations); probe: a list that receives every ReLU pre-activation"""
    d, eps = c["d"], 1e-5
    x = W["decoder_learned_parameters"].unsqueeze(0).repeat(mem.shape[0], 1, 1)
    for i in range(c["layers"]):
        g = lambda nm: W["decoder.layers.%d.%s" % (i, nm)]                                    # noqa: E731
        ln = lambda t, nm: F.layer_norm(t, (d,), g(nm + ".weight"), g(nm + ".bias"), eps)     # noqa: E731

        def drop(site):
            if masks is None:
                return lambda t: t
            keep = torch.tensor(masks[i][site]).to(mem.dtype)
            return lambda t: t * keep.reshape(t.shape) * (1.0 / (1.0 - p))
        at = lambda nm, q, kv, site: _mha(q, kv, g(nm + ".in_proj_weight"), g(nm + ".in_proj_bias"), g(nm + ".out_proj.weight"),      # noqa: E731
                                          g(nm + ".out_proj.bias"), c["heads"], drop(site))
        x = ln(x + drop(1)(at("self_attn", x, x, 0)), "norm1")
        x = ln(x + drop(3)(at("multihead_attn", x, mem, 2)), "norm2")
        pre = x @ g("linear.weight").t() + g("linear.bias")
        if probe is not None:
            probe.append(pre.detach())
        h = drop(4)(F.relu(pre))                                                              # [B, M, F]
        S = c["n"] * c["p"]
        logits = h @ g("moe.phi").reshape(-1, S)                                              # [B, M, S]
        Dw, Cw = torch.softmax(logits, dim=1), torch.softmax(logits, dim=2)
        Xs = Dw.transpose(1, 2) @ h                                                           # [B, S, F]
        Xs = Xs.reshape(Xs.shape[0], c["n"], c["p"], -1)
        Ys = torch.einsum("bnpf,nfd->bnpd", Xs, g("moe.experts.weight")) + g("moe.experts.bias")[None, :, None, :]
        x = ln(x + drop(5)(Cw @ Ys.reshape(Ys.shape[0], S, d)), "norm3")
    return x @ W["classifier.weight"].t() + W["classifier.bias"]


def head_train(tokens, P, c, dtype, G, masks=None, p=0.0, probe=None):
    """-> {"embeds", "g_tokens", "g_<parameter name>"...} float64 numpy, computed in `dtype`: the gradients of sum(embeds * G)"""
    W = OrderedDict((k, torch.tensor(np.asarray(v)).to(dtype).requires_grad_(True)) for k, v in P.items())
    mem = torch.tensor(np.asarray(tokens)).to(dtype).requires_grad_(True)
    embeds = forward_train(mem, W, c, masks, p, probe)
    (embeds * torch.tensor(np.asarray(G)).to(dtype)).sum().backward()
    out = {"embeds": embeds.detach().double().numpy(), "g_tokens": mem.grad.double().numpy()}
    for k, v in W.items():
        out["g_" + k] = v.grad.double().numpy()
    return out


def relu_gap(probe):
    """the smallest min|pre| / max|pre| over the recorded pre-activation tensors"""
    return min(float(t.abs().min() / t.abs().max()) for t in probe)


def draw(spec, seed):
    """the inputs of one case at `seed`: parameters (umoed_cases.head_params), tokens, the upstream G, the p = 0.3 masks"""
    P = UC.head_params(spec, seed)
    rng = np.random.default_rng(seed + 500)
    x = rng.standard_normal((spec["B"], spec["T"], spec["E"])).astype(np.float32)
    G = rng.standard_normal((spec["B"], spec["M"], spec["V"])).astype(np.float32)
    return dict(spec, seed=seed, P=P, x=x, G=G, masks=draw_masks(spec, seed))


def setting(c, name):
    """-> (masks, p) of SETTINGS[name]"""
    return (None, 0.0) if name == "p0" else (c["masks"], P_DROP)


def case_gap(c):
    """the case's ReLU guard over both settings, in float64"""
    gaps = []
    for s in SETTINGS:
        probe = []
        masks, p = setting(c, s)
        head_train(c["x"], c["P"], c, torch.float64, c["G"], masks, p, probe)
        gaps.append(relu_gap(probe))
    return min(gaps)


def find_seed(spec):
    """how the seeds in TRAIN_CASES / GOLDEN_CASE were chosen: the first of seed, seed + 1000, ... (at most MAX_REDRAWS redraws) whose
    draw passes the guard"""
    for attempt in range(MAX_REDRAWS + 1):
        seed = spec["seed"] + 1000 * attempt
        if case_gap(draw(spec, seed)) >= RELU_GAP:
            return seed
    raise AssertionError("no guarded draw for %r" % (spec,))


@functools.lru_cache(maxsize=None)
def case(name):
    spec = GOLDEN_CASE if name == "golden" else TRAIN_CASES[name]
    return dict(draw(spec, spec["seed"]), name=name)


@functools.lru_cache(maxsize=None)
def reference(name, which, dtype=torch.float64):
    """the restatement of case `name` in setting `which`; computed once and shared: callers must not write into it"""
    c = case(name)
    masks, p = setting(c, which)
    return head_train(c["x"], c["P"], c, dtype, c["G"], masks, p)


def kind(key):
    """a tensor's kind: its name without the layer index"""
    return re.sub(r"layers\.\d+\.", "layers.", key)


@functools.lru_cache(maxsize=None)
def pool():
    """kind -> the largest float32-against-float64 error of the restatement over TRAIN_CASES and SETTINGS"""
    out = {}
    for name in TRAIN_CASES:
        for which in SETTINGS:
            r64, r32 = reference(name, which), reference(name, which, torch.float32)
            for key in r64:
                out[kind(key)] = max(out.get(kind(key), 0.0), UC.rel_err(r32[key], r64[key]))
    return out


def own_errors(name, which):
    r64, r32 = reference(name, which), reference(name, which, torch.float32)
    return {k: UC.rel_err(r32[k], r64[k]) for k in r64}


def pool_for(keys):
    """umoed_cases.compare looks a pool up by key: every key under its kind's value"""
    P = pool()
    return {k: P[kind(k)] for k in keys}


def golden_vector(result):
    """what the golden file keeps of a result dictionary: one vector, the tensors in sorted key order, each whole (up to GOLDEN_WHOLE
    elements) or as GOLDEN_SAMPLE values at seeded positions followed by its sum and sum of squares -> (vector, {key: slice})"""
    parts, where, at = [], {}, 0
    for key in sorted(result):
        v = np.asarray(result[key], np.float64).reshape(-1)
        if v.size > GOLDEN_WHOLE:
            idx = np.sort(np.random.default_rng(sum(key.encode()) + v.size).choice(v.size, GOLDEN_SAMPLE, replace=False))
            v = np.concatenate([v[idx], [v.sum(), (v * v).sum()]])
        parts.append(v)
        where[key] = slice(at, at + v.size)
        at += v.size
    return np.concatenate(parts), where
