"""GPU: the two CLIP towers trained through their token outputs (xmh_*_train_forward_tokens / xmh_*_backward_tokens behind torch.autograd
in CLIP.encode_image_train_tokens / encode_text_train_tokens) against the goldens of the reference's own
VisionTransformer(return_patches=True) / CLIP.encode_text and against the float64 restatement of tests/tower_tokens_cases.py; either
upstream gradient alone, the forward's bit identity with the exact-mode encode_image / encode_text of a return_patches=True model,
reproducibility, frozen parameters, the C entry points and their accumulate flag, an in-place change, no host synchronisation.

Tolerances.  Per tensor, e = max|got - fp64| / max|fp64|.  The yardstick is the reference's own fp32 error: the port must stay within
TOL_FACTOR * max(e_ref pooled over the committed cases of that tower and tensor kind, e_ref of that very case), the latter measured in
the test from the restatement's fp32 run on the CPU; TOL_FACTOR is the factor of tests/test_gpu_tower_grad.py.  Against the thinned fp32
golden itself the factor is TOL_FACTOR + 1 by the triangle inequality."""
import ctypes

import numpy as np
import pytest
import torch

import tower_tokens_cases as TT

pytestmark = pytest.mark.gpu

TOL_FACTOR = 4.0


def _kpm(kpm):
    return None if kpm is None else torch.tensor(kpm).cuda()


def _forward(tower, m, x, kpm):
    """-> (cls, tokens [LND], new_mask or None)"""
    xt = torch.tensor(x).cuda()
    if tower == "img":
        return (*m.encode_image_train_tokens(xt), None)
    return m.encode_text_train_tokens(xt, key_padding_mask=_kpm(kpm))


def _step(tower, m, x, ups, kpm, use="both"):
    cls, tokens, _ = _forward(tower, m, x, kpm)
    for y in (cls, tokens):
        assert y.requires_grad and y.dtype == torch.float32 and y.is_cuda
    TT.loss_of(cls, tokens, [torch.tensor(u).cuda() for u in ups], use).backward()
    out = {"y_cls": cls.detach().cpu().numpy(), "y_tok": tokens.detach().cpu().numpy()}
    for name, p in TT.tower_parameters(tower, m).items():
        out[name] = None if p.grad is None else p.grad.cpu().numpy()
    assert m.logit_scale.grad is None
    return out


def _module(tower, sd):
    return TT.build_clip(tower, sd).cuda()


_refs = {}


def _reference(key, tower, sd, x, ups, kpm, use="both"):
    """the float64 restatement and the pooled e_ref of its fp32 run, computed once per key and shared"""
    key = (key, use)
    if key not in _refs:
        r64 = TT.run_restatement(tower, sd, x, ups, kpm, torch.float64, use)
        _refs[key] = (r64, TT.erefs(TT.run_restatement(tower, sd, x, ups, kpm, torch.float32, use), r64)[1])
    return _refs[key]


def _check(tower, got, R, what, own):
    """every figure is printed before the first assertion"""
    rows = []
    for k in R:
        if got[k] is None:
            continue
        kind = TT.kind_of(k)
        tol = TOL_FACTOR * max(TT.pool_eref(tower, kind), own.get(kind, 0.0))
        rows.append((k, TT.rel_err(got[k], R[k]), tol))
    print(what, " ".join("%s %.2e/%.2e" % r for r in rows))
    worst = {}
    for k, e, tol in rows:
        worst[TT.kind_of(k)] = max(worst.get(TT.kind_of(k), 0.0), e / (tol / TOL_FACTOR))
    print(what, "e_port / e_ref per kind:", " ".join("%s %.2f" % (k, v) for k, v in worst.items()))
    for k, e, tol in rows:
        assert got[k].shape == R[k].shape and np.isfinite(got[k]).all(), (what, k)
        assert e <= tol, (what, k, e, tol)


def _check_exact_zeros(tower, got, sd, x):
    if tower != "txt":
        return
    L = x.shape[1]
    assert not got["g_pos"][L:].any()                                            # no token sits at these positions
    vocab = sd["token_embedding.weight"].shape[0]
    absent = np.setdiff1d(np.arange(vocab), np.unique(x))
    assert not got["g_tok"][absent].any()                                        # an id that never occurs: an exactly-zero row


# 1 every output and gradient against float64 -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(TT.CASES))
def test_every_output_and_gradient_matches_the_reference(case):
    G = TT.golden()
    tower = TT.tower_of(case)
    sd, x, ups, kpm = TT.case_inputs(case)
    assert TT.inputs_checksum(sd, x, ups, kpm) == float(G[case + "__checksum"])
    R, own = _reference(case, tower, sd, x, ups, kpm)
    got = _step(tower, _module(tower, sd), x, ups, kpm)
    assert sorted(got) == sorted(R) and all(v is not None for v in got.values())
    rows = []
    for k in R:
        err = np.abs(TT.thin(got[k]).astype(np.float64) - G["%s__%s" % (case, k)].astype(np.float64)).max() / (np.abs(R[k]).max() or 1.0)
        rows.append((k, err, (TOL_FACTOR + 1) * max(TT.pool_eref(tower, TT.kind_of(k)), own.get(TT.kind_of(k), 0.0))))
    print(case, "against the fp32 golden:", " ".join("%s %.2e/%.2e" % r for r in rows))
    _check(tower, got, R, case, own)
    for k, err, tol in rows:
        assert err <= tol, (case, "golden", k, err, tol)
    _check_exact_zeros(tower, got, sd, x)


@pytest.mark.parametrize("tower,spec", TT.OTHER, ids=lambda v: v if isinstance(v, str) else "x".join(str(int(s)) for s in v))
def test_against_the_restatement_on_other_shapes(tower, spec):
    seed = 7000 + sum(int(s) for s in spec)
    sd, x, ups, kpm = TT.spec_inputs(tower, spec, seed)
    R, own = _reference((tower, spec), tower, sd, x, ups, kpm)
    print("e_ref of this case:", " ".join("%s %.2e" % (k, own[k]) for k in TT.KINDS[tower]))
    got = _step(tower, _module(tower, sd), x, ups, kpm)
    _check(tower, got, R, "%s %s" % (tower, spec), own)
    _check_exact_zeros(tower, got, sd, x)


# 2 either upstream alone -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use", ["cls", "tokens"])
@pytest.mark.parametrize("case", ["img_r32_p8_d128_b3", "txt_v11_c40_d64_b5_kpm"])
def test_either_upstream_alone(case, use):
    tower = TT.tower_of(case)
    sd, x, ups, kpm = TT.case_inputs(case)
    R, own = _reference(case, tower, sd, x, ups, kpm, use)
    got = _step(tower, _module(tower, sd), x, ups, kpm, use)
    assert all(v is not None for v in got.values())
    _check(tower, got, R, "%s, %s alone" % (case, use), own)
    _check_exact_zeros(tower, got, sd, x)


# 3 forward ---------------------------------------------------------------------------------------------------------------------
TRAIN_ENTRIES = ("xmh_vit_train_forward", "xmh_text_train_forward", "xmh_vit_backward", "xmh_text_backward", "xmh_vit_train_forward_tokens",
                 "xmh_text_train_forward_tokens", "xmh_vit_backward_tokens", "xmh_text_backward_tokens", "xmh_clip_blocks_forward_saved")


def _patches_model(tower, m):
    """the eval path returns the tokens of a return_patches=True model only"""
    m.return_patches = m.visual.return_patches = True
    return m


@pytest.mark.parametrize("case", ["img_r32_p8_d128_b3", "img_r28_p4_d64_b5", "txt_v11_c40_d64_b5_kpm", "txt_v64_c16_d64_b3"])
def test_forward_is_the_exact_mode_encode_and_no_grad_keeps_no_record(case, monkeypatch):
    from xmh import ops
    from xmh._lib import lib
    from xmh.models import clip
    tower = TT.tower_of(case)
    sd, x, ups, kpm = TT.case_inputs(case)
    m = _patches_model(tower, _module(tower, sd))
    cls, tokens, mask = _forward(tower, m, x, kpm)
    assert cls.requires_grad and tokens.requires_grad
    before = ops.get_precision()
    ops.set_precision("f32x")
    monkeypatch.setattr(clip, "TEXT_PACKING", False)
    try:
        xt = torch.tensor(x).cuda()
        if tower == "img":
            want = (*m.encode_image(xt)[:2], None)
        else:
            e, t, _, nm = m.encode_text(xt, key_padding_mask=_kpm(kpm), masked_rows="exact")
            want = (e, t, nm)
    finally:
        ops.set_precision(before)

    def same(got):
        assert got[0].shape == want[0].shape and got[1].shape == want[1].shape
        assert torch.equal(got[0].detach(), want[0]) and torch.equal(got[1].detach(), want[1])
        assert (got[2] is None) == (want[2] is None) and (want[2] is None or (got[2].dtype == want[2].dtype and torch.equal(got[2], want[2])))
    same((cls, tokens, mask))
    assert tokens.stride(2) == 1 and tokens.stride(1) == tokens.shape[0] * tokens.shape[2]          # the LND view of a dense [B, ., E] buffer
    if tower == "txt":
        assert (mask is None) == (kpm is None)

    def boom(*a, **k):
        raise AssertionError("not under no_grad")
    for name in TRAIN_ENTRIES:
        monkeypatch.setattr(lib, name, boom)
    with torch.no_grad():
        z = _forward(tower, m, x, kpm)
    assert not z[0].requires_grad and not z[1].requires_grad and z[0].grad_fn is None
    same(z)
    for p in m.parameters():
        p.requires_grad_(False)
    z = _forward(tower, m, x, kpm)                                               # nothing to differentiate: the same plain forward
    assert not z[0].requires_grad and not z[1].requires_grad
    same(z)


# 4 reproducibility -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["img_r28_p4_d64_b5", "txt_v11_c40_d64_b5_kpm"])
def test_two_backwards_agree_to_the_bit(case):
    tower = TT.tower_of(case)
    sd, x, ups, kpm = TT.case_inputs(case)
    a, b = (_step(tower, _module(tower, sd), x, ups, kpm) for _ in range(2))
    assert all(np.array_equal(a[k], b[k]) for k in a)
    m = _module(tower, sd)                                                       # and two backwards over one module
    c = _step(tower, m, x, ups, kpm)
    m.zero_grad(set_to_none=True)
    d = _step(tower, m, x, ups, kpm)
    assert all(np.array_equal(c[k], d[k]) and np.array_equal(a[k], c[k]) for k in a)


# 5 frozen parameters -------------------------------------------------------------------------------------------------------------
def _frozen_run(case, frozen):
    tower = TT.tower_of(case)
    sd, x, ups, kpm = TT.case_inputs(case)
    full = _step(tower, _module(tower, sd), x, ups, kpm)
    m = _module(tower, sd)
    params = TT.tower_parameters(tower, m)
    for name, p in params.items():
        p.requires_grad_(not frozen(name))
    got = _step(tower, m, x, ups, kpm)
    assert np.array_equal(got["y_cls"], full["y_cls"]) and np.array_equal(got["y_tok"], full["y_tok"])
    for name in params:
        assert (got[name] is None) == bool(frozen(name)), name
        if got[name] is not None:
            assert np.array_equal(got[name], full[name]), name
    return got


def test_frozen_parameters_get_none_and_the_others_keep_their_bits():
    _frozen_run("img_r32_p8_d128_b3", lambda n: n == "g_conv1")
    _frozen_run("txt_v11_c40_d64_b5_kpm", lambda n: n == "g_tok")
    _frozen_run("img_r32_p8_d128_b3", lambda n: n in ("g_pos", "g_ln_pre_b", "g_ln_post_w", "g_proj", "g_l1_fc_w"))
    # everything below the top block: the walk ends there, front end included
    top = lambda n: n.startswith("g_l1_") or n in ("g_proj", "g_ln_post_w", "g_ln_post_b", "g_text_projection", "g_ln_final_w", "g_ln_final_b")      # noqa: E731
    got = _frozen_run("img_r32_p8_d128_b3", lambda n: not top(n))
    assert got["g_l1_qkv_w"] is not None and got["g_l0_qkv_w"] is None and got["g_conv1"] is None
    _frozen_run("txt_v11_c40_d64_b5_kpm", lambda n: not top(n))
    # the back end alone
    _frozen_run("img_r32_p8_d128_b3", lambda n: n not in ("g_proj", "g_ln_post_b"))
    _frozen_run("txt_v64_c16_d64_b3", lambda n: n not in ("g_text_projection", "g_ln_final_b"))


# 6 the C entry points ------------------------------------------------------------------------------------------------------------
class _CEntry:
    """forward kept once through the C ABI; backward with chosen gradient buffers"""

    def __init__(self, case):
        from xmh import _lib
        from xmh._lib import check, current_stream, lib, ptr
        from xmh.models import clip_train as CT
        self.tower = TT.tower_of(case)
        sd, x, ups, kpm = TT.case_inputs(case)
        self.m = _module(self.tower, sd)
        self.x = torch.tensor(x).cuda()
        self.up_cls = torch.tensor(ups[0]).cuda()
        self.up_tok = torch.tensor(ups[1]).cuda().permute(1, 0, 2).contiguous()     # the C entry takes the tokens' gradient [B, ., E]
        self.kpm = None if kpm is None else torch.tensor(kpm).cuda().to(torch.uint8)
        self.keep = []
        named = TT.tower_parameters(self.tower, self.m)
        self.order = list(named)
        B = self.x.shape[0]
        if self.tower == "img":
            vis = self.m.visual
            self.struct, self.table = _lib.VitGrads, CT.VIT
            self.params = CT.tower_params(vis, CT.VIT)
            self.desc = d = CT.vit_desc(vis, self.params, self.keep)
            self.L = vis.positional_embedding.shape[0]
            self.sbytes = lib.xmh_vit_train_tokens_saved_bytes(B, self.L, d.width, d.layers)
            self.nbytes = lib.xmh_vit_train_tokens_ws_bytes(B, self.L, d.width, d.conv1.k, d.out_dim)
            assert self.sbytes > lib.xmh_vit_train_saved_bytes(B, self.L, d.width, d.layers)
            rows = self.L - 1
        else:
            self.struct, self.table = _lib.TextGrads, CT.TEXT
            self.params = CT.tower_params(self.m, CT.TEXT)
            self.desc = d = CT.text_desc(self.m, self.params, self.keep)
            self.L = self.x.shape[1]
            self.sbytes = lib.xmh_text_train_tokens_saved_bytes(B, self.L, d.width, d.layers)
            self.nbytes = lib.xmh_text_train_tokens_ws_bytes(B, self.L, d.width, d.out_dim)
            rows = self.L
        assert [named[n].data_ptr() for n in self.order] == [p.data_ptr() for p in self.params]
        assert self.sbytes > 0 and self.nbytes > 0
        self.B = B
        self.buf = torch.empty(self.sbytes // 4, dtype=torch.float32, device="cuda")
        self.ws = torch.empty(self.nbytes, dtype=torch.uint8, device="cuda")
        self.y = torch.empty(B, d.out_dim, dtype=torch.float32, device="cuda")
        self.tokens = torch.empty(B, rows, d.out_dim, dtype=torch.float32, device="cuda")
        self.eos = torch.empty(B, dtype=torch.int32, device="cuda")
        self.CT, self.lib, self.ptr, self.stream = CT, lib, ptr, current_stream
        check(self.forward(), "train forward")

    def forward(self, saved_bytes=None, ws_bytes=None, y="y", tokens="tokens"):
        lib, ptr = self.lib, self.ptr
        sb, nb = self.sbytes if saved_bytes is None else saved_bytes, self.nbytes if ws_bytes is None else ws_bytes
        yp, tp = ptr(self.y) if y == "y" else None, ptr(self.tokens) if tokens == "tokens" else None
        if self.tower == "img":
            return lib.xmh_vit_train_forward_tokens(ctypes.byref(self.desc), ptr(self.x), self.B, yp, tp, ptr(self.buf), sb, ptr(self.ws), nb, self.stream())
        return lib.xmh_text_train_forward_tokens(ctypes.byref(self.desc), ptr(self.x), ptr(self.kpm), self.B, self.L, yp, tp, ptr(self.eos),
                                                 ptr(self.buf), sb, ptr(self.ws), nb, self.stream())

    def backward(self, want=lambda n: True, accumulate=0, init=None, saved_bytes=None, ws_bytes=None, g=("cls", "tokens")):
        """-> ({name: gradient buffer}, rc); init: what the buffers hold before the call (NaN when not given)"""
        lib, ptr = self.lib, self.ptr
        bufs = {}
        for n, p in zip(self.order, self.params):
            if want(n):
                bufs[n] = torch.full_like(p, float("nan")) if init is None else init[n].clone()
        grads = self.CT.tower_grads(self.struct, self.table, [bufs.get(n) for n in self.order])
        sb, nb = self.sbytes if saved_bytes is None else saved_bytes, self.nbytes if ws_bytes is None else ws_bytes
        gc, gt = ptr(self.up_cls) if "cls" in g else None, ptr(self.up_tok) if "tokens" in g else None
        if self.tower == "img":
            rc = lib.xmh_vit_backward_tokens(ctypes.byref(self.desc), ptr(self.x), self.B, ptr(self.buf), sb, gc, gt, ctypes.byref(grads), accumulate,
                                             ptr(self.ws), nb, self.stream())
        else:
            rc = lib.xmh_text_backward_tokens(ctypes.byref(self.desc), ptr(self.x), ptr(self.kpm), ptr(self.eos), self.B, self.L, ptr(self.buf), sb, gc, gt,
                                              ctypes.byref(grads), accumulate, ptr(self.ws), nb, self.stream())
        return bufs, rc


@pytest.mark.parametrize("case", ["img_r32_p8_d128_b3", "txt_v11_c40_d64_b5_kpm"])
def test_c_entry_reproduces_autograd_and_accumulate_adds(case):
    c = _CEntry(case)
    sd, x, ups, kpm = TT.case_inputs(case)
    auto = _step(c.tower, _module(c.tower, sd), x, ups, kpm)
    a, rc = c.backward()
    assert rc == 0 and len(a) == len(c.params)
    assert np.array_equal(c.y.cpu().numpy(), auto["y_cls"]) and np.array_equal(c.tokens.permute(1, 0, 2).cpu().numpy(), auto["y_tok"])
    assert all(np.array_equal(a[n].cpu().numpy(), auto[n]) for n in a)
    b, rc = c.backward()
    assert rc == 0 and all(torch.equal(a[n], b[n]) for n in a)
    for use in ("cls", "tokens"):                                               # a NULL upstream counts as zeros
        one, rc = c.backward(g=(use,))
        alone = _step(c.tower, _module(c.tower, sd), x, ups, kpm, use)
        assert rc == 0 and all(np.array_equal(one[n].cpu().numpy(), alone[n]) for n in one), use
    g = torch.Generator(device="cuda").manual_seed(3)
    g0 = {n: torch.randn(t.shape, device="cuda", generator=g) for n, t in a.items()}
    acc, rc = c.backward(accumulate=1, init=g0)
    assert rc == 0
    for n in a:
        assert torch.equal(acc[n], g0[n] + a[n]), n
    none, rc = c.backward(want=lambda n: False)                                  # nothing asked for: nothing launched, nothing written
    assert rc == 0 and not none


def test_c_entry_argument_errors():
    from xmh._lib import lib
    for case in ("img_r8_p4_d64_b1", "txt_v64_c16_d64_b3"):
        c = _CEntry(case)
        assert c.forward(saved_bytes=c.sbytes - 1) == -12 and b"saved" in lib.xmh_last_error()
        assert c.forward(ws_bytes=c.nbytes - 1) == -12 and b"workspace" in lib.xmh_last_error()
        assert c.forward(y=None) == -22 and c.forward(tokens=None) == -22
        assert c.backward(saved_bytes=c.sbytes - 1)[1] == -12 and c.backward(ws_bytes=c.nbytes - 1)[1] == -12
        assert c.backward(g=())[1] == -22                                         # both upstream gradients NULL
        assert c.forward() == 0 and c.backward()[1] == 0
    assert lib.xmh_vit_train_tokens_ws_bytes(2, 129, 64, 48, 16) == 0 and lib.xmh_vit_train_tokens_saved_bytes(2, 129, 64, 1) == 0
    assert lib.xmh_text_train_tokens_saved_bytes(2, 8, 66, 1) == 0 and lib.xmh_text_train_tokens_ws_bytes(2, 8, 1088, 16) == 0
    assert lib.xmh_text_train_tokens_saved_bytes(2, 8, 64, 1) > lib.xmh_text_train_saved_bytes(2, 8, 64, 1) > 0


def test_argument_errors_of_the_python_layer():
    sd, x, _, _ = TT.case_inputs("img_r32_p8_d128_b3")
    m = _module("img", sd)
    with pytest.raises(ValueError, match="the tower takes"):
        m.encode_image_train_tokens(torch.zeros(2, 3, 16, 32, device="cuda"))
    sdt, ids, _, _ = TT.case_inputs("txt_v64_c16_d64_b3")
    t = _module("txt", sdt)
    with pytest.raises(ValueError, match="L <= 16"):
        t.encode_text_train_tokens(torch.zeros(2, 17, dtype=torch.int64, device="cuda"))


# 7 a parameter changed in place between forward and backward ---------------------------------------------------------------------
@pytest.mark.parametrize("case,name", [("img_r8_p4_d64_b1", "visual.proj"), ("txt_v64_c16_d64_b3", "text_projection"),
                                       ("txt_v64_c16_d64_b3", "transformer.resblocks.0.mlp.c_fc.weight")])
def test_an_inplace_change_of_a_parameter_before_backward_is_noticed(case, name):
    tower = TT.tower_of(case)
    sd, x, ups, kpm = TT.case_inputs(case)
    m = _module(tower, sd)
    cls, tokens, _ = _forward(tower, m, x, kpm)
    with torch.no_grad():
        m.get_parameter(name).add_(1)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        TT.loss_of(cls, tokens, [torch.tensor(u).cuda() for u in ups]).backward()


# 8 no host synchronisation -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["img_r32_p8_d128_b3", "txt_v11_c40_d64_b5_kpm"])
def test_forward_and_backward_do_not_synchronise(case):
    tower = TT.tower_of(case)
    sd, x, ups, kpm = TT.case_inputs(case)
    m = _module(tower, sd)
    xt, u, mask = torch.tensor(x).cuda(), [torch.tensor(v).cuda() for v in ups], _kpm(kpm)
    run = (lambda: m.encode_image_train_tokens(xt)) if tower == "img" else (lambda: m.encode_text_train_tokens(xt, key_padding_mask=mask)[:2])
    TT.loss_of(*run(), u).backward()                                             # warm the allocator's pools
    m.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        TT.loss_of(*run(), u).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(p.grad is not None for p in TT.tower_parameters(tower, m).values())
