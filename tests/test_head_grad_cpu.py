"""No GPU: the float64 restatement of the train-mode DCMHT / DSPH hash heads (forward and closed-form backward, written here in
numpy -- the reference's text head casts to fp32 inside its LayerNorm, so its module cannot simply be .double()d) against the
goldens the reference's own HashLayer classes produced in .train() mode (tools/make_golden_head_grad.py) and against
torch.autograd of a float64 torch restatement on other shapes; and the argument checks of the five C entry points.
The restatement is the oracle tests/test_gpu_head_grad.py uses on shapes the goldens do not cover.

What the golden file holds.  The heads are E = 512 wide: one [E, E] gradient is 1 MiB in fp32, more than a committed file may be.
So parameters, inputs and upstream gradients are NOT stored: `draw` regenerates them from the stored seeds (numpy PCG64 uniform
doubles only) and the stored checksums pin them; and every stored reference tensor keeps each KEEP-th index of its embedding
axes, named per tensor kind in THIN_AXES (`thin`).  The reference's own fp32 error e_ref = max|golden - fp64| / max|fp64| was measured by the
generator on the FULL tensors and is stored per tensor."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

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
    from oracle import losses as OL
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
    """float64: both heads with the stored keep masks, the HyP loss (test_hyp_loss_cpu.hyp_oracle), its gradient through both heads"""
    from test_hyp_loss_cpu import hyp_oracle
    o = OBJ_DSPH
    zero = np.zeros((o["B"], o["K"]))
    y = {m: dsph_f64(x[m], P[m], keep[m], o["p"], zero)["y"] for m in ("img", "txt")}
    terms, gx, gy, gP = hyp_oracle(torch.tensor(y["img"]), torch.tensor(y["txt"]), torch.tensor(proxies, dtype=torch.float64),
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


def e_ref_max(G, kind):
    """the reference's own fp32 error for one tensor kind: the largest over the committed cases"""
    vals = [float(G[k]) for k in G.files if k.endswith("__eref_" + kind)]
    assert vals, kind
    return max(vals)


# ---- tests ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c[0] for c in DCMHT_CASES])
@pytest.mark.parametrize("mod", ["img", "txt"])
def test_restatement_reproduces_the_dcmht_goldens(case, mod):
    G = golden()
    _, B, K = next(c for c in DCMHT_CASES if c[0] == case)
    pre = "dcmht_%s_%s_" % (case, mod)
    seed = int(G[pre + "seed"])
    P = draw_dcmht(seed, K, mod == "img")
    x, up = draw_batch(seed + 1, B, 2 * K)
    assert checksum([P[k] for k in sorted(P)] + [x, up]) == float(G[pre + "checksum"])
    # the generator stored where the reference's fp32 relu mask and the float64 one disagree (all inside the near-tie band)
    mask = None
    R = dcmht_f64(x, P, mod == "img", up)
    flips = G[pre + "flips"]
    assert len(flips) <= TIE_CAP * B * 2 * K
    if len(flips):
        mask = R["mask"].copy()
        mask[flips[:, 0], flips[:, 1]] ^= True
        assert (np.abs(R["z"]) <= R["tie"])[flips[:, 0], flips[:, 1]].all()
        R = dcmht_f64(x, P, mod == "img", up, mask=mask)
    for kind in ("probs", "g_x") + tuple("g_" + k for k in DCMHT_PARAMS):
        ref, want = G[pre + kind], R[kind]
        e_ref = float(G[pre + "_eref_" + kind])
        assert e_ref < 1e-3, (kind, e_ref)                       # the reference's fp32 run is a float32 computation of this head
        err = np.abs(ref.astype(np.float64) - thin(want, kind)).max()
        scale = np.abs(want).max() or 1.0
        assert err <= e_ref * scale * (1 + 1e-9) + 1e-300, (kind, err / scale, e_ref)
    if mod == "img":
        m = 0.1
        assert np.allclose(G[pre + "running_mean_after"], thin(0.9 * P["running_mean"] + m * R["mean"], "running"), rtol=1e-5, atol=1e-6)
        assert np.allclose(G[pre + "running_var_after"], thin(0.9 * P["running_var"] + m * R["var_unbiased"], "running"), rtol=1e-5, atol=1e-6)
        assert int(G[pre + "num_batches_tracked"]) == 1


@pytest.mark.parametrize("mod", ["img", "txt"])
def test_second_step_accumulates_and_moves_the_running_statistics(mod):
    """the first case is stepped twice on one instance without zero_grad: .grad holds the sum, num_batches_tracked == 2"""
    G = golden()
    case, B, K = DCMHT_CASES[0]
    pre = "dcmht_%s_%s_" % (case, mod)
    seed = int(G[pre + "seed"])
    P = draw_dcmht(seed, K, mod == "img")
    x1, up1 = draw_batch(seed + 1, B, 2 * K)
    x2, up2 = draw_batch(seed + 2, B, 2 * K)
    R1, R2 = dcmht_f64(x1, P, mod == "img", up1), dcmht_f64(x2, P, mod == "img", up2)
    assert len(G[pre + "flips"]) == 0 and len(G[pre + "step2_flips"]) == 0
    for k in DCMHT_PARAMS:
        want = R1["g_" + k] + R2["g_" + k]
        assert np.abs(G[pre + "step2_g_" + k] - thin(want, "g_" + k)).max() <= 2e-5 * (np.abs(want).max() or 1.0)
    assert rel_err(G[pre + "step2_probs"], R2["probs"]) < 2e-5
    if mod == "img":
        rm = 0.9 * (0.9 * P["running_mean"] + 0.1 * R1["mean"]) + 0.1 * R2["mean"]
        rv = 0.9 * (0.9 * P["running_var"] + 0.1 * R1["var_unbiased"]) + 0.1 * R2["var_unbiased"]
        assert np.allclose(G[pre + "step2_running_mean_after"], thin(rm, "running"), rtol=1e-5, atol=1e-6)
        assert np.allclose(G[pre + "step2_running_var_after"], thin(rv, "running"), rtol=1e-5, atol=1e-6)
        assert int(G[pre + "step2_num_batches_tracked"]) == 2


@pytest.mark.parametrize("case", [c[0] for c in DSPH_CASES])
def test_restatement_reproduces_the_dsph_goldens(case):
    G = golden()
    _, B, K, p = next(c for c in DSPH_CASES if c[0] == case)
    pre = "dsph_%s_" % case
    seed = int(G[pre + "seed"])
    P = draw_dsph(seed, K)
    x, up = draw_batch(seed + 1, B, K)
    assert checksum([P["b"], P["w"], x, up]) == float(G[pre + "checksum"])
    keep = G[pre + "keep"] if p > 0 else None
    assert (pre + "keep" in G.files) == (p > 0)
    if keep is not None:
        assert keep.shape == (B, K) and 0.6 < keep.mean() < 0.95
    R = dsph_f64(x, P, keep, p, up)
    for kind in ("y", "g_w", "g_b", "g_x"):
        e_ref = float(G[pre + "_eref_" + kind])
        assert e_ref < 2e-5, (kind, e_ref)
        want = R[kind]
        assert np.abs(G[pre + kind].astype(np.float64) - thin(want, kind)).max() <= e_ref * np.abs(want).max() * (1 + 1e-9)


def test_restatement_reproduces_the_dcmht_objective_golden():
    """reference DCMHT model: hash heads in train mode -> object_function -> loss.backward(); every head gradient"""
    G = golden()
    P, x, labels = obj_dcmht_inputs()
    assert checksum([P[m][k] for m in ("img", "txt") for k in sorted(P[m])] + [x["img"], x["txt"], labels]) == float(G["dcmht_obj_checksum"])
    assert np.array_equal(G["dcmht_obj_labels"], labels.astype(np.uint8))
    loss, R = obj_dcmht_f64(P, x, labels)
    assert abs(loss - float(G["dcmht_obj_loss"])) <= 2e-6 * abs(loss)
    for m in ("img", "txt"):
        pre = "dcmht_obj_%s_" % m
        assert len(G[pre + "flips"]) == 0
        for kind in ("probs", "g_x") + tuple("g_" + k for k in DCMHT_PARAMS):
            e_ref, want = float(G[pre + "_eref_" + kind]), R[m][kind]
            assert e_ref < 1e-4, (m, kind, e_ref)
            assert np.abs(G[pre + kind].astype(np.float64) - thin(want, kind)).max() <= e_ref * (np.abs(want).max() or 1.0) * (1 + 1e-9)


def test_restatement_reproduces_the_dsph_objective_golden():
    """reference DSPH model: hash heads in train mode (dropout masks recovered and stored) -> object_function (HyP) -> backward"""
    G = golden()
    P, x, labels, proxies = obj_dsph_inputs()
    assert checksum([P["img"]["w"], P["img"]["b"], P["txt"]["w"], P["txt"]["b"], x["img"], x["txt"], labels, proxies]) == float(G["dsph_obj_checksum"])
    keep = {m: G["dsph_obj_%s_keep" % m] for m in ("img", "txt")}
    loss, R, gP = obj_dsph_f64(P, x, labels, proxies, keep, float(G["dsph_obj_threshold"]))
    assert abs(loss - float(G["dsph_obj_loss"])) <= 2e-6 * abs(loss)
    assert np.abs(G["dsph_obj_g_P"] - gP).max() <= float(G["dsph_obj__eref_g_P"]) * np.abs(gP).max() * (1 + 1e-9)
    for m in ("img", "txt"):
        pre = "dsph_obj_%s_" % m
        for kind in ("y", "g_w", "g_b", "g_x"):
            e_ref, want = float(G[pre + "_eref_" + kind]), R[m][kind]
            assert e_ref < 1e-4, (m, kind, e_ref)
            assert np.abs(G[pre + kind].astype(np.float64) - thin(want, kind)).max() <= e_ref * np.abs(want).max() * (1 + 1e-9)


def _torch_dcmht(x, P, bn, up, eps=1e-5):
    t = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in P.items() if k in DCMHT_PARAMS}
    xt = torch.tensor(np.asarray(x, np.float64), requires_grad=True)
    e = xt.shape[1]
    v = torch.nn.functional.linear(xt, t["in_w"][2 * e:], t["in_b"][2 * e:])
    o = torch.nn.functional.linear(v, t["out_w"], t["out_b"])
    if bn:
        nh = (o - o.mean(0)) / torch.sqrt(o.var(0, unbiased=False) + eps)
        n = nh * t["norm_w"] + t["norm_b"]
    else:
        n = torch.nn.functional.layer_norm(o, (e,), t["norm_w"], t["norm_b"], eps)
    f = torch.relu(torch.nn.functional.linear(n, t["w2"], t["b2"]))
    p = torch.softmax(f.view(f.shape[0], -1, 2), -1).view(f.shape[0], -1)
    (p * torch.tensor(np.asarray(up, np.float64))).sum().backward()
    g = {"g_" + k: v.grad.numpy() for k, v in t.items()}
    g["g_x"], g["probs"] = xt.grad.numpy(), p.detach().numpy()
    return g


@pytest.mark.parametrize("B,e,K,bn", [(1, 24, 3, False), (2, 16, 1, True), (2, 16, 1, False), (7, 40, 5, True), (33, 64, 12, False),
                                      (5, 8, 1, True)])
def test_restatement_agrees_with_autograd_in_float64(B, e, K, bn):
    P = draw_dcmht(100 + B + K, K, bn, e)
    x, up = draw_batch(200 + B, B, 2 * K, e)
    R, T = dcmht_f64(x, P, bn, up), _torch_dcmht(x, P, bn, up)
    for k, want in T.items():
        assert rel_err(R[k], want) < 1e-11 or np.abs(R[k] - want).max() < 1e-12, (k, rel_err(R[k], want))
    assert not R["g_in_w"][:2 * e].any() and not R["g_in_b"][:2 * e].any()


@pytest.mark.parametrize("B,e,K,p", [(1, 16, 1, 0.0), (2, 24, 3, 0.2), (19, 40, 7, 0.5)])
def test_dsph_restatement_agrees_with_autograd_in_float64(B, e, K, p):
    P = draw_dsph(7 + B, K, e)
    x, up = draw_batch(9 + B, B, K, e)
    keep = None if p == 0 else (np.random.default_rng(B).random((B, K)) >= p).astype(np.uint8)
    R = dsph_f64(x, P, keep, p, up)
    w, b, xt = (torch.tensor(np.asarray(t, np.float64), requires_grad=True) for t in (P["w"], P["b"], x))
    z = torch.nn.functional.linear(xt, w, b)
    if keep is not None:
        z = z * torch.tensor(keep, dtype=torch.float64) / (1.0 - p)
    y = torch.tanh(z)
    (y * torch.tensor(np.asarray(up, np.float64))).sum().backward()
    for k, want in (("y", y.detach()), ("g_w", w.grad), ("g_b", b.grad), ("g_x", xt.grad)):
        assert rel_err(R[k], want.numpy()) < 1e-11, k


def test_argument_errors_of_the_new_entries_without_a_gpu():
    from xmh import _lib
    L = _lib.lib
    one = ctypes.c_void_p(256)                                  # never dereferenced: every check below fails before a launch
    h = _lib.DcmhtTrain(*([one] * 10), 1, 1e-5, 0.1)
    g = _lib.DcmhtGrads()
    fwd = lambda B, e, N, hh=h, x=one, probs=one, saved=one, ws=one: L.xmh_head_dcmht_train_forward(          # noqa: E731
        ctypes.byref(hh) if hh is not None else None, x, B, e, N, probs, saved, 1 << 40, ws, 1 << 40, None)
    bwd = lambda B, e, N, x=one, gp=one, saved=one: L.xmh_head_dcmht_backward(ctypes.byref(h), x, gp, B, e, N, saved, 1 << 40,          # noqa: E731
                                                                             ctypes.byref(g), 0, one, 1 << 40, None)
    for fn, name in ((fwd, b"xmh_head_dcmht_train_forward"), (bwd, b"xmh_head_dcmht_backward")):
        assert fn(0, 512, 32) == -22 and name in L.xmh_last_error()
        assert fn(4, 512, 0) == -22 and fn(4, -1, 32) == -22
        assert fn(4, 512, 33) == -22 and b"odd" in L.xmh_last_error()
        assert fn(4097, 512, 32) == -95 and fn(4, 2049, 32) == -95 and fn(4, 512, 1026) == -95
        assert fn(4, 512, 32, x=None) == -22
    assert fwd(4, 512, 32, hh=None) == -22 and fwd(4, 512, 32, probs=None) == -22 and fwd(4, 512, 32, saved=None) == -22
    assert fwd(4, 512, 32, saved=ctypes.c_void_p(260)) == -22 and b"aligned" in L.xmh_last_error()
    assert fwd(1, 512, 32) == -22 and b"BatchNorm" in L.xmh_last_error()
    assert L.xmh_head_dcmht_train_forward(ctypes.byref(h), one, 4, 512, 32, one, one, 16, one, 1 << 40, None) == -22
    assert bwd(4, 512, 32, gp=None) == -22
    f = lambda B, e, K, p=0.2, w=one, y=one: L.xmh_head_dsph_train_forward(w, one, one, None, p, B, e, K, y, None)          # noqa: E731
    b = lambda B, e, K, p=0.2, w=one, ws=one, n=1 << 40: L.xmh_head_dsph_backward(w, one, one, None, p, one, B, e, K, one, one, one, 0,          # noqa: E731
                                                                                 ws, n, None)
    for fn, name in ((f, b"xmh_head_dsph_train_forward"), (b, b"xmh_head_dsph_backward")):
        assert fn(0, 512, 16) == -22 and name in L.xmh_last_error()
        assert fn(4, 512, -3) == -22 and fn(4, 512, 16, w=None) == -22 and fn(4, 512, 16, p=1.0) == -22 and fn(4, 512, 16, p=-0.1) == -22
        assert fn(4097, 512, 16) == -95 and fn(4, 4096, 16) == -95 and fn(4, 512, 1025) == -95
    assert b(4, 512, 16, ws=None) == -22 and b(4, 512, 16, n=255) == -22


def test_byte_sizes_grow_with_the_batch():
    from xmh import _lib
    ws = ctypes.c_size_t(0)
    last = (0, 0)
    for B in (1, 2, 3, 64, 100, 128, 1000, 1024, 4096):
        saved = _lib.lib.xmh_head_dcmht_train_bytes(B, 512, 128, ctypes.byref(ws))
        assert saved >= 3 * B * 512 * 4 + 2 * B * 128 * 4 + 512 * 4 and ws.value >= 2 * B * 512 * 4 + B * 128 * 4
        assert saved % 256 == 0 and ws.value % 256 == 0 and saved >= last[0] and ws.value >= last[1]
        last = (saved, ws.value)
    assert _lib.lib.xmh_head_dcmht_train_bytes(4, 512, 33, ctypes.byref(ws)) == 0 and ws.value == 0
    assert _lib.lib.xmh_head_dcmht_train_bytes(4097, 512, 32, None) == 0 and _lib.lib.xmh_head_dcmht_train_bytes(0, 512, 32, None) == 0
