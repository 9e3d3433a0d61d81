"""TEST INFRASTRUCTURE ONLY -- the seeded cases and the restatement of the stage that makes TwDH's transforms (reference
runners/TwDH/transform_matrix_generation/model.py:6-24, train.py:44-96 and 141-176), shared by tests/test_twdh_transform_cpu.py,
tests/test_gpu_twdh_transform.py and tools/make_golden_twdh_transform.py.  numpy only; every function takes the dtype, so the same
code is the float64 reference and the float32 yardstick.

The restatement writes the products as products (x . M and x^T . g_z with the one-hot x), as the reference does.  A NaN is the one
place where the port's gather differs from a product by design (include/xmh.h): a NaN entry reaches only the rows that select it, where
0 * NaN would reach every row.  ``_product`` states that rule: the product over the finite entries, NaN where a selected entry is NaN.

Tolerances (the rule of tests/test_gpu_train_step.py): per tensor e = max|got - f64| / max|f64|; the yardstick is the float32
restatement against the float64 one on the same inputs; the port stays within TOL_FACTOR = 4 of it.  Loss terms: rtol 5e-5, atol 1e-6."""
import math
import os

import numpy as np

TOL_FACTOR = 4.0
ALPHA = 1e-3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "twdh_transform.npz")
SHIPPED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "twdh_transform_shipped.npz")
HYPER = dict(warmup=0.1, schedule="warmup_cosine", b1=0.9, b2=0.98, e=1e-6, weight_decay=0.2, max_grad_norm=1.0)

# the trajectory case of the issue: C 12, L 32, S 8, N 200 labels of 1 to 3 classes, B 64 (the last batch has 8 rows), post_lr 0.01.
# TRAJ_SEED is the first seed for which the reference itself stops lossless by epoch 60 (tools/make_golden_twdh_transform.py looks for
# it and stores the epoch)
TRAJ = dict(C=12, L=32, S=8, N=200, B=64, post_lr=0.01, post_epochs=100)
TRAJ_SEED = 0
TRAJ_STEPS = 20                                  # steps compared tensor by tensor


def rel_err(got, want):
    """max|got - want| / max|want| (absolute where the reference tensor is identically zero)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = np.abs(want).max() if want.size else 0.0
    return float(np.abs(got - want).max() / (scale if scale > 0 else 1.0)) if want.size else 0.0


# ---- targets -------------------------------------------------------------------------------------------------------------------------
def targets(labels, long_c, short_c, tie_l, tie_s):
    """hash_convert(hash_center_multilables(labels, centre)) of both centres as bits [B, L + S] uint8: the sign of the sum of the set
    labels' centres, the tie where the sum is zero, 0 for a row without a label (the reference's NaN mean fails `> 0`)"""
    lab = np.asarray(labels) == 1
    cen = np.concatenate([np.asarray(long_c), np.asarray(short_c)], 1).astype(np.int64)
    tie = np.concatenate([np.asarray(tie_l).reshape(-1), np.asarray(tie_s).reshape(-1)]).astype(np.int64)
    s = lab.astype(np.int64) @ cen
    bits = (s > 0) | ((s == 0) & (tie > 0)[None, :])
    return (bits & (lab.sum(1) > 0)[:, None]).astype(np.uint8)


def pack_bits(bits):
    """[B, K] 0 / 1 -> uint32 [B, ceil(K / 32)], bit k in word k >> 5 at position k & 31 (xmh_twdh_targets' layout)"""
    B, K = bits.shape
    Tw = (K + 31) // 32
    padded = np.zeros((B, Tw * 32), np.uint64)
    padded[:, :K] = bits
    return (padded.reshape(B, Tw, 32) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)


def one_hot(bits, dtype):
    """hash_convert: bit 0 -> (1, 0), bit 1 -> (0, 1): [B, K] -> [B, 2K]"""
    b = np.asarray(bits).astype(dtype)
    return np.stack([1 - b, b], -1).reshape(b.shape[0], -1)


def _product(x, A):
    """x . A for a 0 / 1 matrix x: the product over A's finite entries, NaN where an entry that x selects is NaN"""
    nan = np.isnan(A)
    if not nan.any():
        return x @ A
    out = x @ np.where(nan, 0, A).astype(A.dtype)
    out[(x @ nan.astype(x.dtype)) > 0] = np.nan
    return out


# ---- objective and gradient ------------------------------------------------------------------------------------------------------------
def objective(M, bits, L, S, alpha=ALPHA, dtype=np.float64, up=1.0):
    """-> dict(terms [4] (total, hash, bce, lasso), p [B, 2S], dM [2L, 2S]) in `dtype`"""
    with np.errstate(all="ignore"):
        M = np.asarray(M).astype(dtype)
        B = bits.shape[0]
        x, t = one_hot(bits[:, :L], dtype), one_hot(bits[:, L:L + S], dtype)
        z = _product(x, M).reshape(B, S, 2)
        e = np.exp(z - np.fmax(z[..., :1], z[..., 1:]))
        p = (e / e.sum(-1, keepdims=True)).astype(dtype)
        d = p[..., 0] - p[..., 1]
        hash_ = dtype(1) - (d * d).mean(dtype=dtype)
        pf = p.reshape(B, 2 * S)
        l1, l0 = np.maximum(np.log(pf), dtype(-100)), np.maximum(np.log(dtype(1) - pf), dtype(-100))
        bce = -(t * l1 + (dtype(1) - t) * l0).mean(dtype=dtype)
        lasso = dtype(alpha) * np.abs(M).sum(dtype=dtype)
        g = (pf - t) / np.maximum(pf * (dtype(1) - pf), dtype(1e-12)) / dtype(B * 2 * S)
        g = g.reshape(B, S, 2).copy()
        g[..., 0] += dtype(-2) * d / dtype(B * S)
        g[..., 1] += dtype(2) * d / dtype(B * S)
        gz = (p * (g - (g * p).sum(-1, keepdims=True))).reshape(B, 2 * S).astype(dtype)
        dM = dtype(up) * (_product(x.T.copy(), gz) + dtype(alpha) * np.sign(M))
        return {"terms": np.array([hash_ + bce + lasso, hash_, bce, lasso], dtype), "p": pf, "gz": gz, "dM": dM.astype(dtype)}


def check(M, long_c, short_c, dtype=np.float64):
    """train.py:87-96 -> (wrong [C, S] bool, margin): argmax over each pair of hash_convert(long_c) . M against short_c > 0, equal logits
    giving bit 0; margin = the smallest |z1 - z0|"""
    z = (one_hot(np.asarray(long_c) > 0, dtype) @ np.asarray(M).astype(dtype)).reshape(len(long_c), -1, 2)
    got = z[..., 1] > z[..., 0]
    return got != (np.asarray(short_c) > 0), float(np.abs(z[..., 1] - z[..., 0]).min())


def order_bound(M):
    """the bound of any float32 summation order on a logit, as the issue states it: L 2^-24 sum_l max|M| (the maximum over the pair of
    rows of long bit l)"""
    M = np.abs(np.asarray(M, np.float64))
    L = M.shape[0] // 2
    return L * 2.0 ** -24 * float(M.reshape(L, -1).max(1).sum())


# ---- BertAdam (models/common/optimizer.py:102-167) -------------------------------------------------------------------------------------
def lr_at(step, lr, t_total, warmup=HYPER["warmup"]):
    x = step / t_total
    return lr * (x / warmup if x < warmup else 0.5 * (1.0 + math.cos(math.pi * x)))


def bertadam_step(p, g, m, v, lr, dtype=np.float64, h=HYPER):
    """-> (p, m, v, the clipped gradient), every operation in `dtype`"""
    f = dtype
    norm = np.sqrt((g * g).sum(dtype=f))
    coef = f(h["max_grad_norm"]) / (norm + f(1e-6))
    if coef < 1:
        g = g * coef
    m = m * f(h["b1"]) + f(1.0 - h["b1"]) * g
    v = v * f(h["b2"]) + f(1.0 - h["b2"]) * g * g
    u = m / (np.sqrt(v) + f(h["e"])) + f(h["weight_decay"]) * p
    return (p - f(lr) * u).astype(f), m.astype(f), v.astype(f), g.astype(f)


# ---- one-step cases --------------------------------------------------------------------------------------------------------------------
ONE_STEP = ("straddle", "tile_edge", "wide", "ties_and_empty", "saturated", "zeros_and_signs", "nan")
SHAPES = {"straddle": (7, 40, 12, 5), "tile_edge": (12, 96, 16, 67), "wide": (80, 2048, 64, 200), "ties_and_empty": (6, 40, 12, 9),
          "saturated": (7, 40, 12, 5), "zeros_and_signs": (7, 40, 12, 5), "nan": (7, 40, 12, 5)}       # C x L x S x B
NAN_AT = (2 * 17 + 1, 9)                          # the entry of M that is NaN in the case `nan`


def _labels(rng, B, C, lo=1, hi=3):
    lab = np.zeros((B, C), np.int64)
    for r in range(B):
        lab[r, rng.choice(C, rng.integers(lo, hi + 1), replace=False)] = 1
    return lab


def build(name):
    """-> dict(C, L, S, B, labels, long_c, short_c, tie_l, tie_s, M, bits); the conditions a case stands for are asserted here"""
    C, L, S, B = SHAPES[name]
    rng = np.random.default_rng(7100 + ONE_STEP.index(name))
    long_c = (rng.integers(0, 2, (C, L)) * 2 - 1).astype(np.int8)
    short_c = (rng.integers(0, 2, (C, S)) * 2 - 1).astype(np.int8)
    tie_l, tie_s = (rng.integers(0, 2, L) * 2 - 1).astype(np.int8), (rng.integers(0, 2, S) * 2 - 1).astype(np.int8)
    labels = _labels(rng, B, C)
    M = rng.uniform(-1, 1, (2 * L, 2 * S)).astype(np.float32)
    if name == "ties_and_empty":
        labels[0] = 0                                                                 # no label: all bits 0
        for r in (1, 2, 3):                                                           # two labels: their centres cancel where they differ
            labels[r] = 0
            labels[r, rng.choice(C, 2, replace=False)] = 1
    if name == "saturated":                       # |z0 - z1| = 3 L = 120 > 110 for every row: pair 0 says bit 0, pair 1 says bit 1
        M[:, 0], M[:, 1], M[:, 2], M[:, 3] = 3.0, 0.0, 0.0, 3.0
    if name == "zeros_and_signs":
        M[rng.random(M.shape) < 0.2] = 0.0
    if name == "nan":
        M[NAN_AT] = np.nan
    bits = targets(labels, long_c, short_c, tie_l, tie_s)
    if name == "ties_and_empty":
        s = (labels == 1).astype(np.int64) @ np.concatenate([long_c, short_c], 1).astype(np.int64)
        tie = np.concatenate([tie_l, tie_s])
        zero = (s == 0) & (labels.sum(1) > 0)[:, None]
        assert (zero & (tie > 0)).any() and (zero & (tie < 0)).any(), "a zero sum with each tie value"
        assert (zero[:, :L].any() and zero[:, L:].any()), "ties in both streams"
        assert not bits[0].any()
    if name == "saturated":                       # both pairs are on the wrong side for some row and on the right side for another
        assert len(set(bits[:, L])) == 2 and len(set(bits[:, L + 1])) == 2
    if name == "zeros_and_signs":
        assert (M == 0).sum() > 100 and (M < 0).sum() > 100
    if name == "nan":
        sel = bits[:, NAN_AT[0] // 2] == (NAN_AT[0] & 1)
        assert sel.any() and not sel.all(), "the NaN is selected by some rows and not by others"
    return dict(C=C, L=L, S=S, B=B, labels=labels, long_c=long_c, short_c=short_c, tie_l=tie_l, tie_s=tie_s, M=M, bits=bits)


# ---- the trajectory case ---------------------------------------------------------------------------------------------------------------
def trajectory_inputs(seed=TRAJ_SEED, **over):
    """the replayed draws of a whole run: M0 as np.random.uniform draws it after np.random.seed(seed), the label rows, the centres, the
    batch order of every epoch (a shuffle of all rows, the last partial batch kept) and one pair of tie vectors per step"""
    c = dict(TRAJ, **over)
    C, L, S, N, B = c["C"], c["L"], c["S"], c["N"], c["B"]
    rs = np.random.RandomState(seed)
    M0 = rs.uniform(low=-1, high=1, size=(2 * L, 2 * S)).astype(np.float32)
    rng = np.random.default_rng(7200 + seed)
    long_c = (rng.integers(0, 2, (C, L)) * 2 - 1).astype(np.int8)
    short_c = (rng.integers(0, 2, (C, S)) * 2 - 1).astype(np.int8)
    labels = _labels(rng, N, C)
    per_epoch = math.ceil(N / B)
    batches = []
    for _ in range(c["post_epochs"]):
        perm = rng.permutation(N)
        batches.append([perm[i:i + B].astype(np.int64) for i in range(0, N, B)])
    steps = per_epoch * c["post_epochs"]
    ties = [((rng.integers(0, 2, L) * 2 - 1).astype(np.int8), (rng.integers(0, 2, S) * 2 - 1).astype(np.int8)) for _ in range(steps)]
    return dict(c, seed=seed, M0=M0, long_c=long_c, short_c=short_c, labels=labels, batches=batches, ties=ties, per_epoch=per_epoch,
                t_total=steps)


def run(inp, dtype=np.float64, keep=TRAJ_STEPS, alpha=ALPHA):
    """the recipe on replayed draws -> dict(steps: per-step records (tensors for the first `keep` steps: grad, clipped, M, m, v; always
    terms, lr, next_lr), epoch: the stopping epoch, lossless, M: the final matrix, wrong: per-epoch wrong-bit counts)"""
    L, S = inp["L"], inp["S"]
    M = inp["M0"].astype(dtype)
    m, v = np.zeros_like(M), np.zeros_like(M)
    steps, wrongs, step, lossless, epoch = [], [], 0, False, 0
    for epoch in range(inp["post_epochs"]):
        for idx in inp["batches"][epoch]:
            tl, ts = inp["ties"][step]
            bits = targets(inp["labels"][idx], inp["long_c"], inp["short_c"], tl, ts)
            o = objective(M, bits, L, S, alpha, dtype)
            lr = lr_at(len(steps), inp["post_lr"], inp["t_total"])
            M, m, v, clipped = bertadam_step(M, o["dM"], m, v, lr, dtype)
            rec = {"terms": o["terms"].astype(np.float64), "lr": lr, "next_lr": lr_at(len(steps) + 1, inp["post_lr"], inp["t_total"])}
            if len(steps) < keep:
                rec.update(grad=o["dM"], clipped=clipped, M=M.copy(), m=m.copy(), v=v.copy(), bits=bits)
            steps.append(rec)
            step += 1
        wrong, _ = check(M.astype(np.float32), inp["long_c"], inp["short_c"])
        wrongs.append(int(wrong.sum()))
        if wrongs[-1] == 0:
            lossless = True
            break
    return dict(steps=steps, epoch=epoch, lossless=lossless, M=M, wrong=wrongs)


QUANTITIES = ("grad", "clipped", "delta", "m", "v")


def quantity(rec, q, M0):
    return rec["M"].astype(np.float64) - M0.astype(np.float64) if q == "delta" else rec[q]
