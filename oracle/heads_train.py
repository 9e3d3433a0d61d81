"""TEST INFRASTRUCTURE ONLY -- the train-mode DCMHT / DSPH hash heads in float64: forward and closed-form backward written in numpy
(the reference's text head casts to fp32 inside its LayerNorm, so its module cannot simply be .double()d), the seeded inputs that
tests/golden/head_grad.npz does not store, and the thinning of what it does store.  Pinned against the reference's own HashLayer
classes in .train() mode by that file (oracle/make_golden_head_grad.py) and against torch.autograd by tests/test_head_grad_cpu.py.
Imports neither the reference nor the package.

What the golden file holds.  The heads are E = 512 wide: one [E, E] gradient is 1 MiB in fp32, more than a committed file may be.
So parameters, inputs and upstream gradients are NOT stored: `draw` regenerates them from the stored seeds (numpy PCG64 uniform
doubles only) and the stored checksums pin them; and every stored reference tensor keeps each KEEP-th index of its embedding
axes, named per tensor kind in THIN_AXES (`thin`).  The reference's own fp32 error e_ref = max|golden - fp64| / max|fp64| was measured by the
generator on the FULL tensors and is stored per tensor."""
import os

import numpy as np
import torch

from oracle import losses as OL
from oracle.fixtures import GOLDEN

E = 512
KEEP = 16
EPS32 = float(np.finfo(np.float32).eps)
TIE_FACTOR = 8.0                     # |z64| <= TIE_FACTOR eps32 |n| |w|: fp32 may legitimately put this relu input on the other side
TIE_CAP = 0.005                      # at most this share of (sample, unit) entries of a case
DCMHT_PARAMS = ("in_w", "in_b", "out_w", "out_b", "norm_w", "norm_b", "w2", "b2")
DCMHT_KEYS = {"in_w": "atten.in_proj_weight", "in_b": "atten.in_proj_bias", "out_w": "atten.out_proj.weight",
              "out_b": "atten.out_proj.bias", "norm_w": "norm.weight", "norm_b": "norm.bias", "w2": "fc2.weight", "b2": "fc2.bias"}
# (name, B, K); the first is stepped twice on one instance without zero_grad (running statistics, accumulation)
DCMHT_CASES = [("b100_k16", 100, 16), ("b128_k64", 128, 64), ("b2_k16", 2, 16), ("b37_k128", 37, 128)]
DSPH_CASES = [("b100_k16", 100, 16, 0.2), ("b64_k128", 64, 128, 0.2), ("b64_k16_p0", 64, 16, 0.0)]


# ---- deterministic inputs ---------------------------------------------------------------------------------------------------
def _uniform(rng, shape, a):
    return ((rng.random(shape) * 2.0 - 1.0) * a).astype(np.float32)


def _normalish(rng, shape):
    return ((rng.random(shape + (4,)).sum(-1) - 2.0) * np.sqrt(3.0)).astype(np.float32)       # variance 1, from uniforms only


def draw_dcmht(seed, K, bn, e=E):
    """parameters of one modality head away from their initial values (biases and the affine not 0 / 1), as float32"""
    rng = np.random.default_rng(seed)
    a = 1.0 / np.sqrt(e)
    P = {"in_w": _uniform(rng, (3 * e, e), 1.5 * a), "in_b": _uniform(rng, (3 * e,), 0.1), "out_w": _uniform(rng, (e, e), 1.5 * a),
         "out_b": _uniform(rng, (e,), 0.1), "norm_w": 1.0 + _uniform(rng, (e,), 0.3), "norm_b": _uniform(rng, (e,), 0.2),
         "w2": _uniform(rng, (2 * K, e), 2.0 * a), "b2": _uniform(rng, (2 * K,), 0.1)}
    if bn:
        P["running_mean"], P["running_var"] = _uniform(rng, (e,), 0.1), 1.0 + _uniform(rng, (e,), 0.3)
    return P


def draw_dsph(seed, K, e=E):
    rng = np.random.default_rng(seed)
    return {"w": _uniform(rng, (K, e), 2.0 / np.sqrt(e)), "b": _uniform(rng, (K,), 0.1)}


def draw_batch(seed, B, n_out, e=E):
    """(x [B, e], upstream [B, n_out])"""
    rng = np.random.default_rng(seed)
    return _normalish(rng, (B, e)), _normalish(rng, (B, n_out))


def checksum(arrays):
    return float(sum(np.abs(np.asarray(a, dtype=np.float64)).sum() * (i + 1) for i, a in enumerate(arrays)))


# which axes of a stored tensor run over the E (or 3E) embedding columns, by tensor kind: those are thinned, nothing else is
THIN_AXES = {"probs": (), "g_x": (1,), "g_in_w": (0, 1), "g_in_b": (0,), "g_out_w": (0, 1), "g_out_b": (0,), "g_norm_w": (0,),
             "g_norm_b": (0,), "g_w2": (1,), "g_b2": (), "running": (0,), "y": (), "g_w": (1,), "g_b": (), "g_P": ()}


def thin(a, kind):
    """keep every KEEP-th index of the embedding axes of a tensor of this kind"""
    a = np.asarray(a)
    for d in THIN_AXES[kind]:
        a = np.take(a, np.arange(0, a.shape[d], KEEP), axis=d)
    return a


# ---- float64 restatement ----------------------------------------------------------------------------------------------------
def dcmht_f64(x, P, bn, up, eps=1e-5, mask=None):
    """forward and closed-form backward of one modality head in train mode, float64.  `mask` ([B, 2K] bool) replaces the relu
    mask z > 0 where given.  Returns a dict: probs, z (fc2 pre-activations), tie (the near-tie bound per entry), the gradient
    of sum(up * probs) with respect to every parameter (g_<name>) and to x (g_x), and the batch statistics (mean, var_unbiased)."""
    x, up = np.asarray(x, np.float64), np.asarray(up, np.float64)
    P = {k: np.asarray(v, np.float64) for k, v in P.items()}
    e = x.shape[1]
    wv, bv = P["in_w"][2 * e:], P["in_b"][2 * e:]
    v = x @ wv.T + bv
    o = v @ P["out_w"].T + P["out_b"]
    ax = 0 if bn else 1
    mu = o.mean(ax, keepdims=True)
    var = ((o - mu) ** 2).mean(ax, keepdims=True)
    rstd = 1.0 / np.sqrt(var + eps)
    nh = (o - mu) * rstd
    n = nh * P["norm_w"] + P["norm_b"]
    z = n @ P["w2"].T + P["b2"]
    tie = TIE_FACTOR * EPS32 * np.linalg.norm(n, axis=1)[:, None] * np.linalg.norm(P["w2"], axis=1)[None, :]
    m = (z > 0) if mask is None else np.asarray(mask, bool)
    f = np.where(m, z, 0.0)
    fp = f.reshape(f.shape[0], -1, 2)
    ex = np.exp(fp - fp.max(-1, keepdims=True))
    p = ex / ex.sum(-1, keepdims=True)
    g = up.reshape(p.shape)
    dz = p * (g - (p * g).sum(-1, keepdims=True))
    df = np.where(m, dz.reshape(f.shape), 0.0)
    out = {"probs": p.reshape(f.shape), "z": z, "tie": tie, "mask": m}
    out["g_w2"], out["g_b2"] = df.T @ n, df.sum(0)
    dn = df @ P["w2"]
    out["g_norm_w"], out["g_norm_b"] = (dn * nh).sum(0), dn.sum(0)
    h = dn * P["norm_w"]
    do = rstd * (h - h.mean(ax, keepdims=True) - nh * (h * nh).mean(ax, keepdims=True))
    out["g_out_w"], out["g_out_b"] = do.T @ v, do.sum(0)
    dv = do @ P["out_w"]
    out["g_in_w"] = np.concatenate([np.zeros((2 * e, e)), dv.T @ x])
    out["g_in_b"] = np.concatenate([np.zeros(2 * e), dv.sum(0)])
    out["g_x"] = dv @ wv
    if bn:
        # a bias in front of BatchNorm cancels in o - mean(o): sum_b do and sum_b dv are identically zero (torch and the HIP path
        # leave rounding noise there; compared absolutely, like the q / k thirds)
        out["g_out_b"], out["g_in_b"] = np.zeros(e), np.zeros(3 * e)
        B = x.shape[0]
        out["mean"], out["var_unbiased"] = mu[0], var[0] * B / max(B - 1, 1)
    return out


def dsph_f64(x, P, keep, p, up):
    x, up, w, b = (np.asarray(t, np.float64) for t in (x, up, P["w"], P["b"]))
    s = np.ones_like(up) if keep is None else np.asarray(keep, np.float64) / (1.0 - p)
    y = np.tanh((x @ w.T + b) * s)
    dz = up * (1.0 - y * y) * s
    return {"y": y, "g_w": dz.T @ x, "g_b": dz.sum(0), "g_x": dz @ w}


# ---- the chain loss gradient -> head, through the reference MODEL's own object_function: one case per method -------------------
OBJ_DCMHT = dict(B=48, K=16, C=24, seed=2601)
OBJ_DSPH = dict(B=40, K=16, C=80, seed=2701, alpha=0.8, p=0.2)


def draw_labels(seed, B, C):
    rng = np.random.default_rng(seed)
    L = (rng.random((B, C)) < 0.1).astype(np.float32)
    L[np.arange(B), (rng.random(B) * C).astype(np.int64)] = 1.0
    return L


def obj_dcmht_inputs():
    o = OBJ_DCMHT
    P = {"img": draw_dcmht(o["seed"], o["K"], True), "txt": draw_dcmht(o["seed"] + 1, o["K"], False)}
    x = {"img": draw_batch(o["seed"] + 2, o["B"], 1)[0], "txt": draw_batch(o["seed"] + 3, o["B"], 1)[0]}
    return P, x, draw_labels(o["seed"] + 4, o["B"], o["C"])


def obj_dcmht_f64(P, x, labels):
    """float64: both heads, the DCMHT objective on their outputs (oracle.losses), its gradient carried back through both heads"""
    K = OBJ_DCMHT["K"]
    zero = np.zeros((OBJ_DCMHT["B"], 2 * K))
    fw = {m: dcmht_f64(x[m], P[m], m == "img", zero) for m in ("img", "txt")}
    pi, pt = (torch.tensor(fw[m]["probs"]) for m in ("img", "txt"))
    L = torch.tensor(labels)
    loss = float(OL.our_loss(pi, pt, L, K)["loss"])
    gi, gt = OL.our_loss_grad(pi, pt, L, K)
    return loss, {"img": dcmht_f64(x["img"], P["img"], True, gi.numpy()), "txt": dcmht_f64(x["txt"], P["txt"], False, gt.numpy())}


def obj_dsph_inputs():
    o = OBJ_DSPH
    P = {"img": draw_dsph(o["seed"], o["K"]), "txt": draw_dsph(o["seed"] + 1, o["K"])}
    x = {"img": draw_batch(o["seed"] + 2, o["B"], 1)[0], "txt": draw_batch(o["seed"] + 3, o["B"], 1)[0]}
    rng = np.random.default_rng(o["seed"] + 5)
    proxies = ((rng.random((o["C"], o["K"])) * 2 - 1) * 0.3).astype(np.float32)
    return P, x, draw_labels(o["seed"] + 4, o["B"], o["C"]), proxies


def obj_dsph_f64(P, x, labels, proxies, keep, threshold):
    """float64: both heads with the stored keep masks, the HyP loss (oracle.losses.hyp_oracle), its gradient through both heads"""
    o = OBJ_DSPH
    zero = np.zeros((o["B"], o["K"]))
    y = {m: dsph_f64(x[m], P[m], keep[m], o["p"], zero)["y"] for m in ("img", "txt")}
    terms, gx, gy, gP = OL.hyp_oracle(torch.tensor(y["img"]), torch.tensor(y["txt"]), torch.tensor(proxies, dtype=torch.float64),
                                   torch.tensor(labels), threshold, o["alpha"])
    R = {"img": dsph_f64(x["img"], P["img"], keep["img"], o["p"], np.asarray(gx)),
         "txt": dsph_f64(x["txt"], P["txt"], keep["txt"], o["p"], np.asarray(gy))}
    return float(np.asarray(terms)[0]), R, np.asarray(gP)


def rel_err(got, want):
    """max|got - want| / max|want| (absolute where the reference tensor is identically zero)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = np.abs(want).max()
    return float(np.abs(got - want).max() / (scale if scale > 0 else 1.0))


def golden():
    return np.load(os.path.join(GOLDEN, "head_grad.npz"))
