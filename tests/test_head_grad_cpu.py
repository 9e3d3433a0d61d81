"""No GPU: the float64 restatement of the train-mode DCMHT / DSPH hash heads (oracle/heads_train.py: forward and closed-form backward
in numpy, the seeded inputs, what the golden file holds) against the goldens the reference's own HashLayer classes produced in
.train() mode (oracle/make_golden_head_grad.py) and against torch.autograd of a float64 torch restatement on other shapes; and the
argument checks of the five C entry points.  The restatement is the oracle tests/test_gpu_head_grad.py uses on shapes the goldens
do not cover."""
import ctypes

import numpy as np
import pytest
import torch

from oracle.heads_train import (DCMHT_CASES, DCMHT_PARAMS, DSPH_CASES, TIE_CAP, checksum, dcmht_f64, draw_batch, draw_dcmht, draw_dsph,
                                dsph_f64, golden, obj_dcmht_f64, obj_dcmht_inputs, obj_dsph_f64, obj_dsph_inputs, rel_err, thin)


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
