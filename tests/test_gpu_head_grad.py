"""GPU: train-mode forward and backward of the DCMHT / DSPH hash heads (xmh_head_grad.hip behind torch.autograd in
xmh/models/heads.py) against the goldens of the reference's own HashLayer classes in .train() mode and against the float64
restatement of oracle/heads_train.py on other shapes; relu-mask consistency, exact zeros in the q / k thirds, BatchNorm running
statistics, the untouched eval path, frozen parameters, accumulation, bit-reproducibility, no host synchronisation, and a few SGD
steps of the heads behind a frozen synthetic backbone.

Tolerances.  Per tensor, e = max|got - fp64| / max|fp64| (absolute for the tensors that are identically zero).  The yardstick is
the reference's own fp32 error e_ref stored in the golden file per tensor: the port must stay within TOL_FACTOR * max(e_ref over
the committed cases of that tensor kind).  Factor 4: a different but equally long summation order can lose about twice the
reference's bits at each of two chained reductions.  The pool of cases is narrowed where one pool would be absurdly loose (`_tol`):
a BatchNorm head is measured against the BatchNorm goldens and a LayerNorm head against the LayerNorm ones, and the B = 2
BatchNorm golden -- two rows, n-hat = +-1 up to eps / var, every rounding of o amplified: its e_ref is 20-100 x the others' --
counts only for batches of at most 3 rows.  The two tensors of the BatchNorm head that are identically zero (the gradients of
the biases in front of the normalisation) hold rounding noise whose absolute size grows with the batch and with the gradient's
magnitude, which the committed shapes do not span: for them the pool stays all BatchNorm cases.  Against the golden itself (an fp32 result e_ref away from fp64) the bound is
(TOL_FACTOR + 1) * e_ref by the triangle inequality.  A relu input whose float64 value lies within TIE_FACTOR eps |n| |w| of zero
may be masked either way: there the restatement is evaluated with the mask the forward itself stored (at most TIE_CAP of a case's
entries, asserted), never the other way round."""
import copy

import numpy as np
import pytest
import torch

from oracle import heads_train as T

pytestmark = pytest.mark.gpu

TOL_FACTOR = 4.0
DCMHT_KINDS = ("probs", "g_x") + tuple("g_" + k for k in T.DCMHT_PARAMS)


SMALL_BATCH_CASE = "b2_k16"          # the ill-conditioned BatchNorm golden: in the pool only for B <= 3
ZERO_KINDS = ("g_in_b", "g_out_b")   # identically zero on the BatchNorm head: absolute noise, pool of all BatchNorm cases


def _tol(G, method, kind, factor=TOL_FACTOR, mod=None, B=None):
    """factor * max(e_ref of this tensor kind over the pool of committed cases); mod: "img" / "txt" for a DCMHT head"""
    keys = [k for k in G.files if k.startswith(method + "_") and k.endswith("__eref_" + kind)]
    if method == "dcmht":
        keys = [k for k in keys if "_%s__eref_" % mod in k]
        if not (B <= 3 or (mod == "img" and kind in ZERO_KINDS)):
            keys = [k for k in keys if SMALL_BATCH_CASE not in k]
    assert keys, (method, kind, mod)
    return factor * max(float(G[k]) for k in keys)


def _dcmht_head(P, K, bn):
    from xmh.models.heads import DCMHTModalityHash
    e = P["out_w"].shape[0]
    m = DCMHTModalityHash(e, K, 8, layernorm=not bn)
    sd = {T.DCMHT_KEYS[k]: torch.tensor(P[k]) for k in T.DCMHT_PARAMS}
    if bn:
        sd.update({"norm.running_mean": torch.tensor(P["running_mean"]), "norm.running_var": torch.tensor(P["running_var"]),
                   "norm.num_batches_tracked": torch.tensor(0)})
    m.load_state_dict(sd, strict=True)
    return m.cuda().train()


def _grads(m):
    return {"g_" + k: m.get_parameter(T.DCMHT_KEYS[k]).grad for k in T.DCMHT_PARAMS}


def _step(m, x, up):
    """forward + backward of sum(up * probs) through the autograd Function (no zero_grad) -> numpy dict"""
    xt = torch.tensor(x).cuda().requires_grad_(True)
    probs = m(xt)
    assert probs.requires_grad and probs.dtype == torch.float32 and probs.is_cuda
    (probs * torch.tensor(up).cuda()).sum().backward()
    out = {k: v.detach().cpu().numpy() for k, v in _grads(m).items()}
    out["probs"], out["g_x"] = probs.detach().cpu().numpy(), xt.grad.cpu().numpy()
    return out


def _saved_f(m, x):
    """the relu output f [B, N] the train forward stores in its saved buffer (layout: include/xmh.h), read from a forward of a COPY
    of the module (the BatchNorm buffers move with every train forward; two forwards agree to the bit)"""
    c = copy.deepcopy(m)
    with torch.no_grad():
        probs, xs, saved = c._train_forward(torch.as_tensor(x).cuda())
    B, e = xs.shape
    N = probs.shape[1]
    a256 = lambda v: (v + 255) & ~255                                           # noqa: E731
    off = 3 * a256(B * e * 4) + a256(max(B, e) * 4)
    f = saved[off:off + B * N * 4].view(torch.float32).reshape(B, N).cpu().numpy()
    p = saved[off + a256(B * N * 4):off + a256(B * N * 4) + B * N * 4].view(torch.float32).reshape(B, N).cpu().numpy()
    assert np.array_equal(p, probs.cpu().numpy())
    return f


def _oracle(m, x, P, bn, up):
    """the float64 restatement, with the forward's own mask at the near-tie entries"""
    R = T.dcmht_f64(x, P, bn, up, eps=m.norm.eps)
    port = _saved_f(m, x) > 0
    differ = port != R["mask"]
    assert (np.abs(R["z"]) <= R["tie"])[differ].all(), "a relu decision differs from float64 outside the near-tie band"
    assert differ.sum() <= T.TIE_CAP * differ.size
    return T.dcmht_f64(x, P, bn, up, eps=m.norm.eps, mask=np.where(differ, port, R["mask"])) if differ.any() else R


def _check(G, got, R, what, kinds=DCMHT_KINDS, method="dcmht", mod=None):
    B = got[kinds[0]].shape[0]
    report = []
    for kind in kinds:
        e, tol = T.rel_err(got[kind], R[kind]), _tol(G, method, kind, mod=mod, B=B)
        report.append("%s %.2e/%.2e" % (kind, e, tol))
    print(what, " ".join(report))                                                # each figure before any assertion
    for kind in kinds:
        assert got[kind].shape == R[kind].shape
        e, tol = T.rel_err(got[kind], R[kind]), _tol(G, method, kind, mod=mod, B=B)
        assert e <= tol, (what, kind, e, tol)


def _check_golden(G, got, R, pre, kinds, method, mod=None):
    """against the reference's own fp32 numbers (thinned): (TOL_FACTOR + 1) e_ref, relative to the full float64 tensor"""
    B = got[kinds[0]].shape[0]
    for kind in kinds:
        err = np.abs(T.thin(got[kind], kind) - G[pre + kind].astype(np.float64)).max() / (np.abs(R[kind]).max() or 1.0)
        assert err <= _tol(G, method, kind, TOL_FACTOR + 1, mod=mod, B=B), (pre, kind, err)


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c[0] for c in T.DCMHT_CASES])
@pytest.mark.parametrize("mod", ["img", "txt"])
def test_dcmht_forward_and_every_gradient_match_the_reference(case, mod):
    G = T.golden()
    _, B, K = next(c for c in T.DCMHT_CASES if c[0] == case)
    pre, bn = "dcmht_%s_%s_" % (case, mod), mod == "img"
    seed = int(G[pre + "seed"])
    P = T.draw_dcmht(seed, K, bn)
    x, up = T.draw_batch(seed + 1, B, 2 * K)
    assert T.checksum([P[k] for k in sorted(P)] + [x, up]) == float(G[pre + "checksum"])
    m = _dcmht_head(P, K, bn)
    R = _oracle(m, x, P, bn, up)
    got = _step(m, x, up)
    _check(G, got, R, pre, mod=mod)
    _check_golden(G, got, R, pre, DCMHT_KINDS, "dcmht", mod)
    if bn:
        assert np.allclose(T.thin(m.norm.running_mean.cpu().numpy(), "running"), G[pre + "running_mean_after"], rtol=1e-5, atol=1e-6)
        assert np.allclose(T.thin(m.norm.running_var.cpu().numpy(), "running"), G[pre + "running_var_after"], rtol=1e-5, atol=1e-6)
        assert int(m.norm.num_batches_tracked) == int(G[pre + "num_batches_tracked"]) == 1
    if case == T.DCMHT_CASES[0][0]:                                              # second step, .grad accumulates (no zero_grad)
        x2, up2 = T.draw_batch(seed + 2, B, 2 * K)
        R2 = _oracle(m, x2, P, bn, up2)
        got2 = _step(m, x2, up2)
        for k in T.DCMHT_PARAMS:
            kind, want = "g_" + k, R["g_" + k] + R2["g_" + k]
            assert T.rel_err(got2[kind], want) <= _tol(G, "dcmht", kind, mod=mod, B=B), (pre, "step2", kind)
            err = np.abs(T.thin(got2[kind], kind) - G[pre + "step2_" + kind]).max() / (np.abs(want).max() or 1.0)
            assert err <= _tol(G, "dcmht", kind, TOL_FACTOR + 1, mod=mod, B=B), (pre, "step2 golden", kind, err)
        assert T.rel_err(got2["probs"], G[pre + "step2_probs"]) <= _tol(G, "dcmht", "probs", TOL_FACTOR + 1, mod=mod, B=B)
        if bn:
            assert np.allclose(T.thin(m.norm.running_mean.cpu().numpy(), "running"), G[pre + "step2_running_mean_after"], rtol=1e-5, atol=1e-6)
            assert np.allclose(T.thin(m.norm.running_var.cpu().numpy(), "running"), G[pre + "step2_running_var_after"], rtol=1e-5, atol=1e-6)
            assert int(m.norm.num_batches_tracked) == 2


def _dsph_head(P, p):
    from xmh.models.heads import DSPHLinearHash
    K, e = P["w"].shape
    m = DSPHLinearHash(e, K)
    m.fc.load_state_dict({"weight": torch.tensor(P["w"]), "bias": torch.tensor(P["b"])})
    m.drop_out.p = p
    return m.cuda().train()


def _dsph_step(m, x, up, keep):
    xt = torch.tensor(x).cuda().requires_grad_(True)
    y = m._train(xt, keep=None if keep is None else torch.tensor(keep))
    (y * torch.tensor(up).cuda()).sum().backward()
    return {"y": y.detach().cpu().numpy(), "g_w": m.fc.weight.grad.cpu().numpy(), "g_b": m.fc.bias.grad.cpu().numpy(),
            "g_x": xt.grad.cpu().numpy()}


@pytest.mark.parametrize("case", [c[0] for c in T.DSPH_CASES])
def test_dsph_forward_and_every_gradient_match_the_reference(case):
    G = T.golden()
    _, B, K, p = next(c for c in T.DSPH_CASES if c[0] == case)
    pre = "dsph_%s_" % case
    seed = int(G[pre + "seed"])
    P = T.draw_dsph(seed, K)
    x, up = T.draw_batch(seed + 1, B, K)
    keep = G[pre + "keep"] if p > 0 else None
    m = _dsph_head(P, p)
    got = _dsph_step(m, x, up, keep)
    R = T.dsph_f64(x, P, keep, p, up)
    _check(G, got, R, pre, kinds=("y", "g_w", "g_b", "g_x"), method="dsph")
    _check_golden(G, got, R, pre, ("y", "g_w", "g_b", "g_x"), "dsph")


# 2 ---------------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 16), (2, 24), (3, 64), (100, 128), (128, 256), (1024, 16), (1024, 256), (100, 24)]


@pytest.mark.parametrize("B,K", SHAPES)
@pytest.mark.parametrize("mod", ["img", "txt"])
def test_dcmht_against_the_restatement_on_other_shapes(B, K, mod):
    if mod == "img" and B == 1:
        from xmh.models.heads import DCMHTModalityHash                          # noqa: F401
        m = _dcmht_head(T.draw_dcmht(5, K, True), K, True)
        with pytest.raises(ValueError):                                          # as torch's BatchNorm1d does in training mode
            m(torch.zeros(1, T.E, device="cuda"))
        return
    G = T.golden()
    bn = mod == "img"
    P = T.draw_dcmht(300 + B + K, K, bn)
    x, up = T.draw_batch(400 + B + K, B, 2 * K)
    m = _dcmht_head(P, K, bn)
    R = _oracle(m, x, P, bn, up)
    got = _step(m, x, up)
    _check(G, got, R, "dcmht %s B=%d K=%d" % (mod, B, K), mod=mod)


@pytest.mark.parametrize("B,K,p", [(1, 16, 0.2), (2, 24, 0.0), (3, 64, 0.5), (100, 128, 0.2), (128, 256, 0.2), (1024, 16, 0.2), (1024, 256, 0.0)])
def test_dsph_against_the_restatement_on_other_shapes(B, K, p):
    G = T.golden()
    P = T.draw_dsph(500 + B + K, K)
    x, up = T.draw_batch(600 + B + K, B, K)
    keep = None if p == 0 else (np.random.default_rng(B + K).random((B, K)) >= p).astype(np.uint8)
    got = _dsph_step(_dsph_head(P, p), x, up, keep)
    _check(G, got, T.dsph_f64(x, P, keep, p, up), "dsph B=%d K=%d p=%g" % (B, K, p), kinds=("y", "g_w", "g_b", "g_x"), method="dsph")


def test_dsph_draws_its_own_mask_reproducibly():
    P = T.draw_dsph(11, 64)
    x, _ = T.draw_batch(12, 200, 64)
    m = _dsph_head(P, 0.2)
    outs = []
    for _ in range(2):
        m.generator = torch.Generator(device="cuda").manual_seed(7)
        outs.append(m(torch.tensor(x).cuda()))
    assert torch.equal(outs[0], outs[1]) and outs[0].requires_grad
    z = torch.tensor(x).cuda() @ m.fc.weight.detach().t() + m.fc.bias.detach()
    dropped = (outs[0] == 0) & (z.abs() > 1e-3)
    assert 0.15 < float(dropped.float().mean()) < 0.25                          # p = 0.2 of 12800 entries
    kept = outs[0] != 0
    assert torch.allclose(outs[0][kept], torch.tanh(z / 0.8)[kept], atol=1e-5)


def test_dsph_eval_path_is_the_inference_entry(monkeypatch):
    """.eval(): xmh_head_dsph called here directly gives the module's output to the bit (no dropout, no graph); with the composed
    route, ops.gemm_nt + tanh does"""
    import ctypes
    from xmh import ops
    from xmh._lib import check, current_stream, lib, ptr
    from xmh.models import clip as _clip
    m = _dsph_head(T.draw_dsph(13, 64), 0.2).eval()
    x = torch.tensor(T.draw_batch(14, 50, 64)[0]).cuda()
    out = m(x.clone().requires_grad_(True))
    assert not out.requires_grad and out.grad_fn is None and m.fc.weight.requires_grad
    desc, precision = _clip._cached_desc(m, lambda prec, keep: _clip._linear_desc(m.fc.weight, m.fc.bias, prec, keep), slot="dsph")
    nbytes = lib.xmh_head_workspace_bytes(50, T.E, precision)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device="cuda")
    want = torch.empty(50, 64, device="cuda")
    check(lib.xmh_head_dsph(ctypes.byref(desc), ptr(x), 50, precision, ptr(want), None, None, None, None, ptr(ws), nbytes, current_stream()),
          "xmh_head_dsph")
    assert torch.equal(out, want)
    assert float((out - torch.tanh(x @ m.fc.weight.detach().t() + m.fc.bias.detach())).abs().max()) < 1e-3
    monkeypatch.setattr(_clip, "NATIVE_FORWARD", False)
    with torch.no_grad():
        composed = ops.gemm_nt(x, m.fc.weight, m.fc.bias, act=ops.ACT_TANH)
    got = m(x)
    assert torch.equal(got, composed) and not got.requires_grad


def test_dsph_c_entry_accumulates_and_skips_what_is_not_asked_for():
    """xmh_head_dsph_backward straight from the C ABI: accumulate adds to what is there; d_w NULL (bias alone: the column-sum
    kernel) and d_x NULL give the same d_b / d_w as the full call"""
    from xmh._lib import check, current_stream, lib, ptr
    B, K, p = 37, 24, 0.2
    P = T.draw_dsph(15, K)
    x, up = T.draw_batch(16, B, K)
    keep = torch.tensor((np.random.default_rng(3).random((B, K)) >= p).astype(np.uint8)).cuda()
    w, b, xs, g = (torch.tensor(t).cuda() for t in (P["w"], P["b"], x, up))
    y = torch.empty(B, K, device="cuda")
    check(lib.xmh_head_dsph_train_forward(ptr(w), ptr(b), ptr(xs), ptr(keep), p, B, T.E, K, ptr(y), current_stream()), "forward")
    ws = torch.empty(B * K * 4, dtype=torch.uint8, device="cuda")

    def backward(gw, gb, gx, accumulate):
        check(lib.xmh_head_dsph_backward(ptr(w), ptr(xs), ptr(y), ptr(keep), p, ptr(g), B, T.E, K, ptr(gw), ptr(gb), ptr(gx), accumulate,
                                         ptr(ws), ws.numel(), current_stream()), "xmh_head_dsph_backward")

    gw, gb, gx = torch.empty_like(w), torch.empty_like(b), torch.empty_like(xs)
    backward(gw, gb, gx, 0)
    R = T.dsph_f64(x, P, keep.cpu().numpy(), p, up)
    for got, kind in ((y, "y"), (gw, "g_w"), (gb, "g_b"), (gx, "g_x")):
        assert T.rel_err(got.cpu().numpy(), R[kind]) <= _tol(T.golden(), "dsph", kind), kind
    aw, ab, ax = torch.full_like(w, 3.0), torch.full_like(b, 3.0), torch.full_like(xs, 3.0)
    backward(aw, ab, ax, 1)
    assert torch.equal(aw, 3.0 + gw) and torch.equal(ab, 3.0 + gb)
    assert torch.equal(ax, gx)                                                   # an activation gradient: written, never added to
    ow, ob = torch.full_like(w, 3.0), torch.full_like(b, 3.0)
    backward(ow, None, None, 1)                                                  # weight alone
    backward(None, ob, None, 1)                                                  # bias alone: its own kernel, another fixed order
    assert torch.equal(ow, aw) and float((ob - ab).abs().max()) <= 1e-6 * float(gb.abs().max())
    backward(None, None, None, 0)                                                # nothing asked for: no launch, no error


# 3 ---------------------------------------------------------------------------------------------------------------------------
def test_backward_follows_the_forwards_own_relu_mask():
    """fc2 pre-activations that are exactly 0 (zero weight row and zero bias), within rounding of 0 (the bias cancels the
    float64 dot product, so the fp32 sign is decided by the forward's own rounding) and ordinary ones; one-row batch on the text
    head, where db2 = df and d norm.bias = dn are the per-row quantities themselves"""
    G = T.golden()
    K = 64
    P = T.draw_dcmht(77, K, False)
    x, up = T.draw_batch(78, 1, 2 * K)
    P["w2"][0:16] = 0.0
    P["b2"][0:16] = 0.0
    z = T.dcmht_f64(x, P, False, up)["z"][0]
    P["b2"][16:80] = (P["b2"][16:80].astype(np.float64) - z[16:80]).astype(np.float32)    # z ~ 0 up to rounding
    m = _dcmht_head(P, K, False)
    f = _saved_f(m, x)
    own = T.dcmht_f64(x, P, False, up)
    near = np.zeros(2 * K, bool)
    near[16:80] = True
    assert (f[0, :16] == 0).all() and (np.abs(f[0, 16:80]) < 1e-5).all()
    assert 4 <= (f[0, 16:80] > 0).sum() <= 60                                   # both signs occur
    differ = (f > 0) != own["mask"]
    assert differ[0, 16:80].any() and not differ[0, 80:].any() and not differ[0, :16].any()
    got = _step(m, x, up)
    dead = f[0] == 0
    assert (got["g_b2"][dead] == 0).all() and (got["g_w2"][dead] == 0).all()    # a masked unit contributes nothing
    alive = ~dead
    R = T.dcmht_f64(x, P, False, up, mask=f > 0)
    big = np.abs(R["g_b2"]) > 1e-4
    assert (got["g_b2"][alive & big] != 0).all()
    for kind in ("g_b2", "g_w2", "g_norm_b", "g_norm_w", "g_x"):                # g_norm_b is dn of the one row
        assert T.rel_err(got[kind], R[kind]) <= _tol(G, "dcmht", kind, mod="txt", B=1), kind
    assert T.rel_err(got["g_b2"], own["g_b2"]) > 100 * _tol(G, "dcmht", "g_b2", mod="txt", B=1)  # float64's own mask would not have passed


# 4, 7 ------------------------------------------------------------------------------------------------------------------------
def test_qk_thirds_are_exact_zeros_and_frozen_parameters_get_none():
    K, B = 16, 20
    for bn in (True, False):
        P = T.draw_dcmht(31, K, bn)
        x, up = T.draw_batch(32, B, 2 * K)
        m = _dcmht_head(P, K, bn)
        _step(m, x, up)
        gw, gb = m.atten.in_proj_weight.grad, m.atten.in_proj_bias.grad
        assert gw.shape == (3 * T.E, T.E) and not gw[:2 * T.E].any() and not gb[:2 * T.E].any() and gw[2 * T.E:].abs().max() > 0
        full = {k: v.clone() for k, v in _grads(m).items()}
        m.zero_grad(set_to_none=True)
        for name in ("atten.in_proj_weight", "atten.in_proj_bias", "atten.out_proj.weight", "norm.weight", "fc2.bias"):
            m.get_parameter(name).requires_grad_(False)
        xt = torch.tensor(x).cuda()                                              # and no gradient to the embeddings either
        probs = m(xt)
        (probs * torch.tensor(up).cuda()).sum().backward()
        # the running statistics moved between the two forwards but batch statistics normalise: same gradients, to the bit
        # (out_proj.bias without out_proj.weight is summed by a kernel of its own, in another -- fixed -- order of double additions)
        for k, g in _grads(m).items():
            frozen = not m.get_parameter(T.DCMHT_KEYS[k[2:]]).requires_grad
            assert (g is None) == frozen, k
            if not frozen:
                assert torch.equal(g, full[k]) or (k == "g_out_b" and float((g - full[k]).abs().max()) <= 1e-6 * float(full["g_b2"].abs().max())), k
        for p in m.parameters():
            p.requires_grad_(False)
        assert not m(xt).requires_grad                                           # nothing to differentiate: plain train forward


def test_accumulate_flag_upstream_bit_identity_and_double_backward():
    import ctypes
    from xmh import _lib
    from xmh._lib import check, current_stream, lib, ptr
    K, B = 24, 37
    P = T.draw_dcmht(41, K, True)
    x, up = T.draw_batch(42, B, 2 * K)
    m = _dcmht_head(P, K, True)
    a = _step(copy.deepcopy(m), x, up)
    b = _step(copy.deepcopy(m), x, up)
    assert all(np.array_equal(a[k], b[k]) for k in a)                            # two calls agree to the bit
    c = _step(copy.deepcopy(m), x, 0.5 * up)                                     # upstream scales the gradients (0.5: exact in binary)
    assert all(np.array_equal(0.5 * a[k], c[k]) for k in a if k != "probs")
    # the C entry's accumulate flag: parameter gradients are added to what is there
    xs = torch.tensor(x).cuda()
    mm = copy.deepcopy(m)
    probs, xs, saved = mm._train_forward(xs)
    h, keep = mm._train_args()
    nws = ctypes.c_size_t(0)
    nsaved = lib.xmh_head_dcmht_train_bytes(B, T.E, 2 * K, ctypes.byref(nws))
    ws = torch.empty(nws.value, dtype=torch.uint8, device="cuda")
    bufs = [torch.full((T.E, T.E), 3.0, device="cuda"), torch.full((T.E,), 3.0, device="cuda"), torch.full((T.E, T.E), 3.0, device="cuda"),
            torch.full((T.E,), 3.0, device="cuda"), torch.full((T.E,), 3.0, device="cuda"), torch.full((T.E,), 3.0, device="cuda"),
            torch.full((2 * K, T.E), 3.0, device="cuda"), torch.full((2 * K,), 3.0, device="cuda")]
    g = _lib.DcmhtGrads(*[t.data_ptr() for t in bufs], None)
    check(lib.xmh_head_dcmht_backward(ctypes.byref(h), ptr(xs), ptr(torch.tensor(up).cuda()), B, T.E, 2 * K, ptr(saved), nsaved,
                                      ctypes.byref(g), 1, ptr(ws), nws.value, current_stream()), "xmh_head_dcmht_backward")
    plain = [a["g_in_w"][2 * T.E:], a["g_in_b"][2 * T.E:]] + [a["g_" + k] for k in T.DCMHT_PARAMS[2:]]
    for t, want in zip(bufs, plain):
        assert np.array_equal(t.cpu().numpy(), np.float32(3.0) + want)
    xt = torch.tensor(x).cuda().requires_grad_(True)
    probs = m(xt)
    (gx,) = torch.autograd.grad(probs.sum(), xt, create_graph=True)
    with pytest.raises(RuntimeError):
        gx.sum().backward()                                                      # once_differentiable


# 5, 6 ------------------------------------------------------------------------------------------------------------------------
def test_running_statistics_and_the_untouched_eval_path(monkeypatch):
    from xmh import ops
    from xmh.models import clip as _clip
    K, B = 16, 50
    P = T.draw_dcmht(51, K, True)
    m = _dcmht_head(P, K, True)
    xe = torch.tensor(T.draw_batch(50, 9, 2 * K)[0]).cuda()
    m.eval()
    before = m(xe)                                                               # the eval path's weight descriptors exist before training
    m.train()
    rm, rv = P["running_mean"].astype(np.float64), P["running_var"].astype(np.float64)
    for s in range(2):
        x, up = T.draw_batch(52 + s, B, 2 * K)
        R = T.dcmht_f64(x, P, True, up)
        with torch.no_grad():                                                    # train mode under no_grad: batch statistics, buffers move
            out = m(torch.tensor(x).cuda())
        assert not out.requires_grad and T.rel_err(out.cpu().numpy(), R["probs"]) < 1e-5
        rm, rv = 0.9 * rm + 0.1 * R["mean"], 0.9 * rv + 0.1 * R["var_unbiased"]
        assert np.allclose(m.norm.running_mean.cpu().numpy(), rm, rtol=1e-5, atol=1e-6)
        assert np.allclose(m.norm.running_var.cpu().numpy(), rv, rtol=1e-5, atol=1e-6)
        assert int(m.norm.num_batches_tracked) == s + 1
    m.eval()
    after = m(xe)
    assert not torch.equal(before, after)                                        # the new running statistics are in use
    fresh = _dcmht_head(P, K, True)
    fresh.load_state_dict(m.state_dict())
    fresh.eval()
    assert torch.equal(after, fresh(xe))                                         # bit for bit what the eval path gives for these buffers
    for mod in (m, _dcmht_head(T.draw_dcmht(53, K, False), K, False).eval()):
        assert all(p.requires_grad for p in mod.parameters()) and torch.is_grad_enabled()
        out = mod(xe.clone().requires_grad_(True))
        assert not out.requires_grad and out.grad_fn is None
        assert torch.equal(out, mod._native(xe))
        monkeypatch.setattr(_clip, "NATIVE_FORWARD", False)
        e = T.E
        with torch.no_grad():
            v = ops.gemm_nt(xe, mod.atten.in_proj_weight[2 * e:], mod.atten.in_proj_bias[2 * e:])
            o = ops.gemm_nt(v, mod.atten.out_proj.weight, mod.atten.out_proj.bias)
            n = (ops.affine_cols(o, mod.norm.running_mean, mod.norm.running_var, mod.norm.weight, mod.norm.bias, mod.norm.eps)
                 if isinstance(mod.norm, torch.nn.BatchNorm1d) else ops.layernorm(o, mod.norm.weight, mod.norm.bias, mod.norm.eps))
            want = ops.pair_softmax(ops.gemm_nt(n, mod.fc2.weight, mod.fc2.bias, act=ops.ACT_RELU))
        got = mod(xe)
        assert torch.equal(got, want) and not got.requires_grad
        monkeypatch.setattr(_clip, "NATIVE_FORWARD", True)


# 8 ---------------------------------------------------------------------------------------------------------------------------
def test_forward_and_backward_do_not_synchronise():
    K, B = 64, 100
    heads = [_dcmht_head(T.draw_dcmht(61, K, True), K, True), _dcmht_head(T.draw_dcmht(62, K, False), K, False),
             _dsph_head(T.draw_dsph(63, K), 0.2)]
    x, up = T.draw_batch(64, B, 2 * K)
    xs = [torch.tensor(x).cuda().requires_grad_(True) for _ in heads]
    ups = [torch.tensor(up).cuda(), torch.tensor(up).cuda(), torch.tensor(up[:, :K]).cuda()]
    for h, xt, u in zip(heads, xs, ups):                                         # warm the allocator's pools
        (h(xt) * u).sum().backward()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for h, xt, u in zip(heads, xs, ups):
            (h(xt) * u).sum().backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(xt.grad is not None for xt in xs) and all(p.grad is not None for h in heads for p in h.parameters())


# 9 ---------------------------------------------------------------------------------------------------------------------------
def _embeddings(model, B):
    from xmh.models import weights as W
    image, (ids, _) = W.synth_images(2, B), W.synth_text(2, B)
    with torch.no_grad():
        return model.backbone.encode_image(image.cuda()).float(), model.backbone.encode_text(ids.cuda()).float()


def _labels(B, C):
    g = torch.Generator().manual_seed(3)
    L = (torch.rand(B, C, generator=g) < 0.15).float()
    L[torch.arange(B), torch.randint(0, C, (B,), generator=g)] = 1.0
    return L


def _dcmht64(x, t, bn, eps):
    e = x.shape[1]
    F = torch.nn.functional
    o = F.linear(F.linear(x, t["atten.in_proj_weight"][2 * e:], t["atten.in_proj_bias"][2 * e:]), t["atten.out_proj.weight"],
                 t["atten.out_proj.bias"])
    if bn:
        n = (o - o.mean(0)) / torch.sqrt(o.var(0, unbiased=False) + eps) * t["norm.weight"] + t["norm.bias"]
    else:
        n = F.layer_norm(o, (e,), t["norm.weight"], t["norm.bias"], eps)
    f = torch.relu(F.linear(n, t["fc2.weight"], t["fc2.bias"]))
    return torch.softmax(f.view(f.shape[0], -1, 2), -1).view(f.shape[0], -1)


def test_dcmht_sgd_steps_on_the_heads_track_the_restatement():
    """runners/DCMHT/runner.py:120-126 with the backbone frozen: embeddings under no_grad, model.hash -> object_function ->
    backward -> a stock SGD step on the heads; five steps follow the float64 restatement (heads above, loss of oracle.losses)"""
    from oracle import losses as OL
    from xmh.models.dcmht import DCMHT
    from xmh.utils.config import Config
    B, K, C = 12, 16, 10
    model = DCMHT.from_config(Config({"clip_path": "synthetic:1814:vision_layers=1,transformer_layers=1"}), output_dim=K).cuda().eval()
    emb_i, emb_t = _embeddings(model, B)
    labels = _labels(B, C)
    model.hash.train()
    names = [n for n, _ in model.hash.named_parameters()]
    assert len(names) == 16                                                      # 8 tensors per modality
    d = {n: p.detach().cpu().double().clone().requires_grad_(True) for n, p in model.hash.named_parameters()}
    opt = torch.optim.SGD(model.hash.parameters(), lr=0.05)
    opt_d = torch.optim.SGD(list(d.values()), lr=0.05)
    xi, xt = emb_i.cpu().double(), emb_t.cpu().double()
    losses = []
    for _ in range(5):
        opt.zero_grad()
        opt_d.zero_grad()
        hi, ht = model.hash(emb_i, emb_t)
        loss, _ = model.object_function(hi, ht, labels.cuda())
        loss.backward()
        assert all(p.grad is not None for p in model.hash.parameters())
        pi = _dcmht64(xi, {k[len("img_hash."):]: v for k, v in d.items() if k.startswith("img_hash.")}, True, 1e-5)
        pt = _dcmht64(xt, {k[len("txt_hash."):]: v for k, v in d.items() if k.startswith("txt_hash.")}, False, 1e-5)
        want = OL.our_loss(pi, pt, labels, K, vartheta=model.vartheta, threshold=model.threshold, quan_alpha=model.quan_alpha)["loss"]
        want.backward()
        print("dcmht step loss %.8f want %.8f" % (float(loss), float(want)))
        assert abs(float(loss) - float(want)) <= 5e-5 * abs(float(want)) + 1e-6
        losses.append(float(loss))
        opt.step()
        opt_d.step()
    assert losses[-1] != losses[0]
    for n, p in model.hash.named_parameters():
        assert float((p.detach().cpu().double() - d[n].detach()).abs().max()) <= 5e-5 * max(1.0, float(d[n].detach().abs().max())), n
    assert int(model.hash.img_hash.norm.num_batches_tracked) == 5


def test_dsph_sgd_steps_on_the_heads_track_the_restatement():
    """runners/DSPH/runner.py:118-125 with the backbone frozen: the two fc layers and the proxies stepped by a stock SGD"""
    from oracle.losses import hyp_terms
    from xmh.models.dsph import DSPH
    from xmh.utils.config import Config
    B, K, C = 12, 16, 10
    model = DSPH(cfg=Config({}), outputDim=K, clipPath="synthetic:1814:vision_layers=1,transformer_layers=1", numclass=C, alpha=0.8,
                 threshold=0.25).cuda().eval()
    emb_i, emb_t = _embeddings(model, B)
    labels = _labels(B, C)
    model.hash.train()
    heads = (model.hash.img_hash, model.hash.txt_hash)
    for s, h in enumerate(heads):
        h.generator = torch.Generator(device="cuda").manual_seed(100 + s)
    twin = [torch.Generator(device="cuda").manual_seed(100 + s) for s in range(2)]     # draws the same masks for the restatement
    params = list(model.hash.parameters()) + [model.hyp.proxies]
    assert len(params) == 5
    d = [p.detach().cpu().double().clone().requires_grad_(True) for p in params]
    opt, opt_d = torch.optim.SGD(params, lr=0.05), torch.optim.SGD(d, lr=0.05)
    xi, xt = emb_i.cpu().double(), emb_t.cpu().double()
    first = None
    for _ in range(5):
        opt.zero_grad()
        opt_d.zero_grad()
        hi, ht = model.hash(emb_i, emb_t)
        loss, _ = model.object_function(hi, ht, labels.cuda())
        loss.backward()
        assert all(p.grad is not None for p in params)
        codes = []
        for s, x in enumerate((xi, xt)):
            keep = (torch.rand(B, K, device="cuda", generator=twin[s]) >= 0.2).cpu().double()
            codes.append(torch.tanh(torch.nn.functional.linear(x, d[2 * s], d[2 * s + 1]) * keep / 0.8))
        want = hyp_terms(codes[0], codes[1], d[4], labels, 0.25, 0.8)["loss"]
        want.backward()
        print("dsph step loss %.8f want %.8f" % (float(loss), float(want)))
        assert abs(float(loss) - float(want)) <= 5e-5 * abs(float(want)) + 1e-6
        first = float(loss) if first is None else first
        opt.step()
        opt_d.step()
    assert float(loss) != first
    for p, q in zip(params, d):
        assert float((p.detach().cpu().double() - q.detach()).abs().max()) <= 5e-5 * max(1.0, float(q.detach().abs().max()))


# the chain through the reference MODEL's own object_function -------------------------------------------------------------------
def test_dcmht_objective_chain_matches_the_reference():
    """model.hash (train mode) -> DCMHT.object_function -> loss.backward(): loss and every head gradient against the golden of the
    reference model and against the float64 restatement of the whole chain"""
    from xmh.models.dcmht import DCMHT
    from xmh.models.heads import DCMHTHashLayer
    G = T.golden()
    o = T.OBJ_DCMHT
    P, x, labels = T.obj_dcmht_inputs()
    assert np.array_equal(G["dcmht_obj_labels"], labels.astype(np.uint8))
    model = DCMHT.__new__(DCMHT)                                                # the objective reads these attributes only; no backbone
    torch.nn.Module.__init__(model)
    model.output_dim, model.vartheta, model.threshold, model.quan_alpha, model.similarity_function = o["K"], 0.75, 0.1, 0.001, "euclidean"
    model.hash = DCMHTHashLayer(feature_size=T.E, outputDim=o["K"])
    model.hash.img_hash, model.hash.txt_hash = _dcmht_head(P["img"], o["K"], True), _dcmht_head(P["txt"], o["K"], False)
    loss64, R = T.obj_dcmht_f64(P, x, labels)
    for mod in ("img", "txt"):
        assert np.array_equal(_saved_f(getattr(model.hash, mod + "_hash"), x[mod]) > 0, R[mod]["mask"])
    xt = {mod: torch.tensor(x[mod]).cuda().requires_grad_(True) for mod in ("img", "txt")}
    hi, ht = model.hash(xt["img"], xt["txt"])
    loss, _ = model.object_function(hi, ht, torch.tensor(labels).cuda())
    loss.backward()
    print("dcmht objective loss %.8f reference %.8f float64 %.8f" % (float(loss), float(G["dcmht_obj_loss"]), loss64))
    assert abs(float(loss) - loss64) <= 2e-5 * abs(loss64) and abs(float(loss) - float(G["dcmht_obj_loss"])) <= 2e-5 * abs(loss64)
    for mod, probs in (("img", hi), ("txt", ht)):
        head = getattr(model.hash, mod + "_hash")
        got = {k: v.detach().cpu().numpy() for k, v in _grads(head).items()}
        got["probs"], got["g_x"] = probs.detach().cpu().numpy(), xt[mod].grad.cpu().numpy()
        got = {k: got[k] for k in DCMHT_KINDS}
        _check(G, got, R[mod], "dcmht_obj_%s_" % mod, mod=mod)
        _check_golden(G, got, R[mod], "dcmht_obj_%s_" % mod, DCMHT_KINDS, "dcmht", mod)


def test_dsph_objective_chain_matches_the_reference():
    """model.hash (train mode, the reference's own dropout masks replayed) -> DSPH.object_function (HyP) -> loss.backward()"""
    from xmh.models.dsph import DSPH, HyPProxies
    from xmh.models.heads import DSPHHashLayer
    G = T.golden()
    o = T.OBJ_DSPH
    P, x, labels, proxies = T.obj_dsph_inputs()
    keep = {mod: G["dsph_obj_%s_keep" % mod] for mod in ("img", "txt")}
    thr = float(G["dsph_obj_threshold"])
    model = DSPH.__new__(DSPH)
    torch.nn.Module.__init__(model)
    model.hyp = HyPProxies(numclass=o["C"], output_dim=o["K"], alpha=o["alpha"], threshold=thr)
    with torch.no_grad():
        model.hyp.proxies.copy_(torch.tensor(proxies))
    model.hash = DSPHHashLayer(inputDim=T.E, outputDim=o["K"])
    model.hash.img_hash, model.hash.txt_hash = _dsph_head(P["img"], o["p"]), _dsph_head(P["txt"], o["p"])
    model = model.cuda()
    xt = {mod: torch.tensor(x[mod]).cuda().requires_grad_(True) for mod in ("img", "txt")}
    codes = {mod: getattr(model.hash, mod + "_hash")._train(xt[mod], keep=torch.tensor(keep[mod])) for mod in ("img", "txt")}
    loss, _ = model.object_function(codes["img"], codes["txt"], torch.tensor(labels).cuda())
    loss.backward()
    loss64, R, gP = T.obj_dsph_f64(P, x, labels, proxies, keep, thr)
    print("dsph objective loss %.8f reference %.8f float64 %.8f" % (float(loss), float(G["dsph_obj_loss"]), loss64))
    assert abs(float(loss) - loss64) <= 2e-5 * abs(loss64) and abs(float(loss) - float(G["dsph_obj_loss"])) <= 2e-5 * abs(loss64)
    e = T.rel_err(model.hyp.proxies.grad.cpu().numpy(), gP)
    print("dsph_obj g_P %.2e (reference %.2e)" % (e, float(G["dsph_obj__eref_g_P"])))
    kinds = ("y", "g_w", "g_b", "g_x")
    for mod in ("img", "txt"):
        head = getattr(model.hash, mod + "_hash")
        got = {"y": codes[mod].detach().cpu().numpy(), "g_w": head.fc.weight.grad.cpu().numpy(), "g_b": head.fc.bias.grad.cpu().numpy(),
               "g_x": xt[mod].grad.cpu().numpy()}
        _check(G, got, R[mod], "dsph_obj_%s_" % mod, kinds=kinds, method="dsph")
        _check_golden(G, got, R[mod], "dsph_obj_%s_" % mod, kinds, "dsph")
    assert e <= 2e-5, e                                                          # the proxies' gradient is xmh_hyp.hip's: its own tests' bound
