"""GPU: backward of the two CLIP towers (xmh_tower_grad.hip behind torch.autograd in CLIP.encode_image_train / encode_text_train) against
the goldens of the reference's own VisionTransformer / CLIP.encode_text and against the float64 restatement of
tests/tower_grad_cases.py on other shapes; the forward's bit identity with the exact-mode encode_image / encode_text,
reproducibility, frozen parameters, the accumulate flag, no host synchronisation, argument errors, the composition with the heads
and the loss, and train_epoch of the DCMHT and DSPH runners.

Tolerances.  Per tensor, e = max|got - fp64| / max|fp64|.  The yardstick is the reference's own fp32 error e_ref stored in the golden
file per tensor: the port must stay within TOL_FACTOR * max(e_ref over the committed cases of that tower and tensor kind) -- the
factor and pooling rule of tests/test_gpu_block_grad.py; against the thinned fp32 golden itself the factor is TOL_FACTOR + 1 by the
triangle inequality.  On the other shapes the yardstick per kind is TOL_FACTOR * max(pool, e_ref of that very case), the latter
measured in the test from the restatement's fp32 run on the CPU."""
import ctypes
import re
import types

import numpy as np
import pytest
import torch

import tower_grad_cases as TC

pytestmark = pytest.mark.gpu

TOL_FACTOR = 4.0


def _kpm(kpm):
    return None if kpm is None else torch.tensor(kpm).cuda()


def _forward(tower, m, x, kpm):
    xt = torch.tensor(x).cuda()
    return m.encode_image_train(xt) if tower == "img" else m.encode_text_train(xt, key_padding_mask=_kpm(kpm))


def _step(tower, m, x, up, kpm):
    y = _forward(tower, m, x, kpm)
    assert y.requires_grad and y.dtype == torch.float32 and y.is_cuda
    (y * torch.tensor(up).cuda()).sum().backward()
    out = {"y": y.detach().cpu().numpy()}
    for name, p in TC.tower_parameters(tower, m).items():
        out[name] = None if p.grad is None else p.grad.cpu().numpy()
    assert m.logit_scale.grad is None
    return out


def _module(tower, sd):
    return TC.build_clip(tower, sd).cuda()


_refs = {}


def _reference(key, tower, sd, x, up, kpm, with_f32=False):
    """the float64 restatement (and its fp32 run where asked for), computed once per key and shared"""
    if key not in _refs:
        r64 = TC.run_restatement(tower, sd, x, up, kpm, torch.float64)
        pool = TC.erefs(TC.run_restatement(tower, sd, x, up, kpm, torch.float32), r64)[1] if with_f32 else {}
        _refs[key] = (r64, pool)
    return _refs[key]


def _check(tower, got, R, what, own=None):
    """every figure is printed before the first assertion"""
    rows = []
    for k in R:
        if got[k] is None:
            continue
        kind = TC.kind_of(k)
        tol = TOL_FACTOR * max(TC.pool_eref(tower, kind), (own or {}).get(kind, 0.0))
        rows.append((k, TC.rel_err(got[k], R[k]), tol))
    print(what, " ".join("%s %.2e/%.2e" % r for r in rows))
    worst = {}
    for k, e, tol in rows:
        worst[TC.kind_of(k)] = max(worst.get(TC.kind_of(k), 0.0), e / (tol / TOL_FACTOR))
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


# 1 goldens -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(TC.CASES))
def test_every_gradient_matches_the_reference(case):
    G = TC.golden()
    tower = TC.tower_of(case)
    sd, x, up, kpm = TC.case_inputs(case)
    assert TC.inputs_checksum(sd, x, up, kpm) == float(G[case + "__checksum"])
    R, _ = _reference(case, tower, sd, x, up, kpm)
    got = _step(tower, _module(tower, sd), x, up, kpm)
    assert sorted(got) == sorted(R) and all(v is not None for v in got.values())
    rows = []
    for k in R:
        err = np.abs(TC.thin(got[k]).astype(np.float64) - G["%s__%s" % (case, k)].astype(np.float64)).max() / (np.abs(R[k]).max() or 1.0)
        rows.append((k, err, (TOL_FACTOR + 1) * TC.pool_eref(tower, TC.kind_of(k))))
    print(case, "against the fp32 golden:", " ".join("%s %.2e/%.2e" % r for r in rows))
    _check(tower, got, R, case)
    for k, err, tol in rows:
        assert err <= tol, (case, "golden", k, err, tol)
    _check_exact_zeros(tower, got, sd, x)


# 2 other shapes ----------------------------------------------------------------------------------------------------------------
SHAPES = [("txt", (97, 64, 64, 1, 16, 50, 41, False)),      # M = 2050 rows: several chunks of every batch reduction plus a remainder
          ("img", (224, 32, 768, 1, 512, 2)),               # the front and back end at ViT-B/32's width, one block
          ("txt", (300, 77, 512, 2, 512, 32, 2, False))]    # a 512-wide text tower


@pytest.mark.parametrize("tower,spec", SHAPES, ids=lambda v: v if isinstance(v, str) else "x".join(str(int(s)) for s in v))
def test_against_the_restatement_on_other_shapes(tower, spec):
    seed = 6000 + sum(int(s) for s in spec)
    sd, x, up, kpm = (TC.image_inputs if tower == "img" else TC.text_inputs)(spec, seed)
    R, own = _reference((tower, spec), tower, sd, x, up, kpm, with_f32=True)
    print("e_ref of this case:", " ".join("%s %.2e" % (k, own[k]) for k in TC.KINDS[tower]))
    got = _step(tower, _module(tower, sd), x, up, kpm)
    _check(tower, got, R, "%s %s" % (tower, spec), own=own)
    _check_exact_zeros(tower, got, sd, x)


# 3 forward ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["img_r32_p8_d128_b3", "txt_v11_c40_d64_b5_kpm", "txt_v64_c16_d64_b3"])
def test_forward_is_the_exact_mode_encode_and_no_grad_keeps_no_record(case, monkeypatch):
    from xmh import ops
    from xmh._lib import lib
    from xmh.models import clip
    tower = TC.tower_of(case)
    sd, x, up, kpm = TC.case_inputs(case)
    m = _module(tower, sd)
    y = _forward(tower, m, x, kpm)
    assert y.requires_grad
    before = ops.get_precision()
    ops.set_precision("f32x")
    monkeypatch.setattr(clip, "TEXT_PACKING", False)
    try:
        xt = torch.tensor(x).cuda()
        want = m.encode_image(xt) if tower == "img" else m.encode_text(xt, key_padding_mask=_kpm(kpm))
    finally:
        ops.set_precision(before)
    assert not want.requires_grad and torch.equal(y.detach(), want)

    def boom(*a, **k):
        raise AssertionError("not under no_grad")
    for name in ("xmh_vit_train_forward", "xmh_text_train_forward", "xmh_vit_backward", "xmh_text_backward", "xmh_clip_blocks_forward_saved"):
        monkeypatch.setattr(lib, name, boom)
    with torch.no_grad():
        z = _forward(tower, m, x, kpm)
    assert not z.requires_grad and z.grad_fn is None and torch.equal(z, want)
    for p in m.parameters():
        p.requires_grad_(False)
    z = _forward(tower, m, x, kpm)                                               # nothing to differentiate: the same plain forward
    assert not z.requires_grad and torch.equal(z, want)


# 4 reproducibility -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["img_r28_p4_d64_b5", "txt_v11_c40_d64_b5_kpm"])
def test_two_backwards_agree_to_the_bit(case):
    tower = TC.tower_of(case)
    sd, x, up, kpm = TC.case_inputs(case)
    a, b = (_step(tower, _module(tower, sd), x, up, kpm) for _ in range(2))
    if tower == "txt":
        assert np.array_equal(a["g_tok"], b["g_tok"])                            # ids repeat across and within rows: one fixed order
    assert all(np.array_equal(a[k], b[k]) for k in a)
    m = _module(tower, sd)                                                       # and two backwards over one module
    c = _step(tower, m, x, up, kpm)
    m.zero_grad(set_to_none=True)
    d = _step(tower, m, x, up, kpm)
    assert all(np.array_equal(c[k], d[k]) and np.array_equal(a[k], c[k]) for k in a)


# 5 frozen parameters, accumulate ---------------------------------------------------------------------------------------------
def _frozen_run(case, frozen):
    tower = TC.tower_of(case)
    sd, x, up, kpm = TC.case_inputs(case)
    full = _step(tower, _module(tower, sd), x, up, kpm)
    m = _module(tower, sd)
    params = TC.tower_parameters(tower, m)
    for name, p in params.items():
        p.requires_grad_(not frozen(name))
    got = _step(tower, m, x, up, kpm)
    assert np.array_equal(got["y"], full["y"])
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
    _frozen_run("txt_v64_c16_d64_b3", lambda n: n not in ("g_text_projection", "g_ln_final_b"))


class _CEntry:
    """forward kept once through the C ABI; backward with chosen gradient buffers"""

    def __init__(self, case):
        from xmh import _lib
        from xmh._lib import check, current_stream, lib, ptr
        from xmh.models import clip_train as CT
        self.tower = TC.tower_of(case)
        sd, x, up, kpm = TC.case_inputs(case)
        self.m = _module(self.tower, sd)
        self.x, self.up = torch.tensor(x).cuda(), torch.tensor(up).cuda()
        self.kpm = None if kpm is None else torch.tensor(kpm).cuda().to(torch.uint8)
        self.keep = []
        named = TC.tower_parameters(self.tower, self.m)
        self.order = list(named)                                                # the names of the test's cases, in the order of the struct's fields
        B = self.x.shape[0]
        if self.tower == "img":
            vis = self.m.visual
            self.struct, self.table = _lib.VitGrads, CT.VIT
            self.params = CT.tower_params(vis, CT.VIT)
            self.desc = d = CT.vit_desc(vis, self.params, self.keep)
            self.L = vis.positional_embedding.shape[0]
            self.sbytes = lib.xmh_vit_train_saved_bytes(B, self.L, d.width, d.layers)
            self.nbytes = lib.xmh_vit_train_ws_bytes(B, self.L, d.width, d.conv1.k, d.out_dim)
        else:
            self.struct, self.table = _lib.TextGrads, CT.TEXT
            self.params = CT.tower_params(self.m, CT.TEXT)
            self.desc = d = CT.text_desc(self.m, self.params, self.keep)
            self.L = self.x.shape[1]
            self.sbytes = lib.xmh_text_train_saved_bytes(B, self.L, d.width, d.layers)
            self.nbytes = lib.xmh_text_train_ws_bytes(B, self.L, d.width, d.out_dim)
        self.D, self.layers, out_dim = d.width, d.layers, d.out_dim
        assert [named[n].data_ptr() for n in self.order] == [p.data_ptr() for p in self.params]     # the package's tables agree with them
        assert self.sbytes > 0 and self.nbytes > 0
        self.B = B
        self.buf = torch.empty(self.sbytes // 4, dtype=torch.float32, device="cuda")
        self.ws = torch.empty(self.nbytes, dtype=torch.uint8, device="cuda")
        self.y = torch.empty(B, out_dim, dtype=torch.float32, device="cuda")
        self.eos = torch.empty(B, dtype=torch.int32, device="cuda")
        self.CT, self.lib, self.ptr, self.stream = CT, lib, ptr, current_stream
        check(self.forward(), "train forward")

    def forward(self, saved_bytes=None, ws_bytes=None, y="y"):
        lib, ptr = self.lib, self.ptr
        sb, nb = self.sbytes if saved_bytes is None else saved_bytes, self.nbytes if ws_bytes is None else ws_bytes
        yp = ptr(self.y) if y == "y" else None
        if self.tower == "img":
            return lib.xmh_vit_train_forward(ctypes.byref(self.desc), ptr(self.x), self.B, yp, ptr(self.buf), sb, ptr(self.ws), nb, self.stream())
        return lib.xmh_text_train_forward(ctypes.byref(self.desc), ptr(self.x), ptr(self.kpm), self.B, self.L, yp, ptr(self.eos), ptr(self.buf), sb,
                                          ptr(self.ws), nb, self.stream())

    def backward(self, want=lambda n: True, accumulate=0, init=None, saved_bytes=None, ws_bytes=None, g="up", L=None):
        """-> ({name: gradient buffer}, rc); init: what the buffers hold before the call (NaN when not given)"""
        lib, ptr = self.lib, self.ptr
        bufs = {}
        for n, p in zip(self.order, self.params):
            if want(n):
                bufs[n] = torch.full_like(p, float("nan")) if init is None else init[n].clone()
        grads = self.CT.tower_grads(self.struct, self.table, [bufs.get(n) for n in self.order])
        sb, nb = self.sbytes if saved_bytes is None else saved_bytes, self.nbytes if ws_bytes is None else ws_bytes
        gp = ptr(self.up) if g == "up" else None
        if self.tower == "img":
            rc = lib.xmh_vit_backward(ctypes.byref(self.desc), ptr(self.x), self.B, ptr(self.buf), sb, gp, ctypes.byref(grads), accumulate,
                                      ptr(self.ws), nb, self.stream())
        else:
            rc = lib.xmh_text_backward(ctypes.byref(self.desc), ptr(self.x), ptr(self.kpm), ptr(self.eos), self.B, L or self.L, ptr(self.buf), sb, gp,
                                       ctypes.byref(grads), accumulate, ptr(self.ws), nb, self.stream())
        return bufs, rc


@pytest.mark.parametrize("case", ["img_r32_p8_d128_b3", "txt_v64_c16_d64_b3"])
def test_c_entry_reproduces_autograd_and_accumulate_adds(case):
    c = _CEntry(case)
    sd, x, up, kpm = TC.case_inputs(case)
    auto = _step(c.tower, _module(c.tower, sd), x, up, kpm)
    a, rc = c.backward()
    assert rc == 0 and len(a) == len(c.params)
    assert np.array_equal(c.y.cpu().numpy(), auto["y"])
    assert all(np.array_equal(a[n].cpu().numpy(), auto[n]) for n in a)
    b, rc = c.backward()
    assert rc == 0 and all(torch.equal(a[n], b[n]) for n in a)
    g = torch.Generator(device="cuda").manual_seed(3)
    g0 = {n: torch.randn(t.shape, device="cuda", generator=g) for n, t in a.items()}
    acc, rc = c.backward(accumulate=1, init=g0)
    assert rc == 0
    for n in a:
        assert torch.equal(acc[n], g0[n] + a[n]), n
    none, rc = c.backward(want=lambda n: False)                                  # nothing asked for: nothing launched, nothing written
    assert rc == 0 and not none


# 5b a parameter changed in place between forward and backward: the backward reuses the forward's descriptor, so autograd must refuse
@pytest.mark.parametrize("case,name", [("img_r8_p4_d64_b1", "visual.proj"), ("txt_v64_c16_d64_b3", "text_projection")])
def test_an_inplace_change_of_a_parameter_before_backward_is_noticed(case, name):
    tower = TC.tower_of(case)
    sd, x, up, kpm = TC.case_inputs(case)
    m = _module(tower, sd)
    y = _forward(tower, m, x, kpm)
    with torch.no_grad():
        m.get_parameter(name).add_(1)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        (y * torch.tensor(up).cuda()).sum().backward()


def test_an_inplace_change_of_a_block_parameter_before_backward_is_noticed():
    import block_grad_cases as BC
    from xmh.models.clip import Transformer
    D, heads, layers, L, B, causal, _ = BC.CASES["d64_l1_b1"]
    sd, x, up, kpm = BC.case_inputs("d64_l1_b1")
    tr = Transformer(D, layers, heads)
    tr.load_state_dict({k: torch.tensor(v) for k, v in sd.items()}, strict=True)
    tr = tr.cuda()
    y = tr.run_train(torch.tensor(x).cuda(), causal=causal)
    with torch.no_grad():
        tr.resblocks[0].mlp.c_fc.weight.add_(1)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        (y * torch.tensor(up).cuda()).sum().backward()


# 6 no host synchronisation -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["img_r32_p8_d128_b3", "txt_v11_c40_d64_b5_kpm"])
def test_forward_and_backward_do_not_synchronise(case):
    tower = TC.tower_of(case)
    sd, x, up, kpm = TC.case_inputs(case)
    m = _module(tower, sd)
    xt, u, mask = torch.tensor(x).cuda(), torch.tensor(up).cuda(), _kpm(kpm)
    run = (lambda: m.encode_image_train(xt)) if tower == "img" else (lambda: m.encode_text_train(xt, key_padding_mask=mask))
    (run() * u).sum().backward()                                                 # warm the allocator's pools
    m.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        (run() * u).sum().backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(p.grad is not None for p in TC.tower_parameters(tower, m).values())


# 7 argument errors -------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    from xmh._lib import lib
    from xmh.models.clip import CLIP
    sd, x, up, kpm = TC.case_inputs("img_r32_p8_d128_b3")
    m = _module("img", sd)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.encode_image_train(torch.tensor(x))
    with pytest.raises(ValueError, match="the tower takes"):
        m.encode_image_train(torch.zeros(2, 3, 16, 32, device="cuda"))
    with pytest.raises(ValueError, match="the tower takes"):
        m.encode_image_train(torch.zeros(2, 1, 32, 32, device="cuda"))
    sdt, ids, _, _ = TC.case_inputs("txt_v64_c16_d64_b3")
    t = _module("txt", sdt)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        t.encode_text_train(torch.tensor(ids))
    with pytest.raises(ValueError, match="L <= 16"):
        t.encode_text_train(torch.zeros(2, 17, dtype=torch.int64, device="cuda"))
    p = CLIP(16, 8, 1, 64, 4, 8, 16, 64, 1, 1, return_patches=True).cuda()
    with pytest.raises(NotImplementedError, match="MITH"):
        p.encode_image_train(torch.zeros(1, 3, 8, 8, device="cuda"))
    with pytest.raises(NotImplementedError, match="MITH"):
        p.encode_text_train(torch.zeros(1, 8, dtype=torch.int64, device="cuda"))
    for case in ("img_r8_p4_d64_b1", "txt_v64_c16_d64_b3"):
        c = _CEntry(case)
        assert c.forward(saved_bytes=c.sbytes - 1) == -12 and b"saved" in lib.xmh_last_error()
        assert c.forward(ws_bytes=c.nbytes - 1) == -12 and b"workspace" in lib.xmh_last_error()
        assert c.forward(y=None) == -22
        assert c.backward(saved_bytes=c.sbytes - 1)[1] == -12 and c.backward(ws_bytes=c.nbytes - 1)[1] == -12
        assert c.backward(g=None)[1] == -22
        if c.tower == "txt":
            assert c.backward(L=17)[1] == -22                                     # beyond the positional embedding
        assert c.forward() == 0 and c.backward()[1] == 0
    assert lib.xmh_vit_train_ws_bytes(2, 129, 64, 48, 16) == 0 and lib.xmh_text_train_saved_bytes(2, 8, 66, 1) == 0


# 8 composition with the heads and the loss -------------------------------------------------------------------------------------
def _labels(B, C):
    g = torch.Generator().manual_seed(5)
    lab = (torch.rand(B, C, generator=g) < 0.3).float()
    lab[torch.arange(B), torch.arange(B) % C] = 1.0
    return lab


def _method_model(arch):
    import xmh.models  # noqa: F401
    from xmh.common.register import registry
    from xmh.utils.config import Config
    extra = {"numclass": 6, "alpha": 0.8, "threshold": 0.25} if arch == "DSPH" else {}
    cfg = Config(dict({"arch": arch, "clip_path": "synthetic:1814:vision_layers=2,transformer_layers=2"}, **extra))
    return registry.get_model_class(arch).from_config(cfg, output_dim=16, train_num=8).float().cuda().train()


@pytest.mark.parametrize("arch", ["DCMHT", "DSPH"])
def test_backbone_gradients_compose_with_the_heads_and_the_loss(arch):
    from xmh.models import weights as W
    model = _method_model(arch)
    B = 4
    image, ids, labels = W.synth_images(2, B).cuda(), W.synth_text(2, B)[0].cuda(), _labels(B, 6).cuda()
    extra = [model.hyp.proxies] if arch == "DSPH" else []
    watched = dict(model.backbone.named_parameters())
    watched.update({"hyp.proxies": p for p in extra})

    def grads():
        out = {n: None if p.grad is None else p.grad.clone() for n, p in watched.items()}
        model.zero_grad(set_to_none=True)
        return out
    torch.manual_seed(11)                                                        # DSPH's dropout masks
    loss, _ = model.object_function(*model.forward_train(image, ids), labels)
    loss.backward()
    one = grads()
    assert one["logit_scale"] is None and all(v is not None and bool(torch.isfinite(v).all()) for n, v in one.items() if n != "logit_scale")
    torch.manual_seed(11)
    e_img, e_txt = model.backbone.encode_image_train(image), model.backbone.encode_text_train(ids)
    leaf_i, leaf_t = e_img.detach().requires_grad_(True), e_txt.detach().requires_grad_(True)
    loss2, _ = model.object_function(model.hash.encode_img(leaf_i), model.hash.encode_txt(leaf_t), labels)
    loss2.backward()
    assert torch.equal(loss2.detach(), loss.detach())
    proxies = {n: p.grad.clone() for n, p in watched.items() if n == "hyp.proxies"}
    for p in model.hash.parameters():
        p.grad = None
    torch.autograd.backward([e_img, e_txt], [leaf_i.grad, leaf_t.grad])
    two = grads()
    two.update(proxies)
    for n in one:
        assert (one[n] is None) == (two[n] is None) and (one[n] is None or torch.equal(one[n], two[n])), n


# 9 train_epoch -----------------------------------------------------------------------------------------------------------------
def _trainer(tmp_path, arch, runner, **run):
    import xmh.models  # noqa: F401
    import xmh.runners  # noqa: F401
    from xmh.common.register import registry
    from xmh.utils.config import Config
    extra = {"numclass": 6, "alpha": 0.8, "threshold": 0.25} if arch == "DSPH" else {}
    small = "vision_layers=1,transformer_layers=1,vision_width=128,transformer_width=128,embed_dim=64,image_resolution=64"
    cfg = Config({
        "model": dict({"arch": arch, "clip_path": "synthetic:1814:" + small}, **extra),
        "dataset": {"arch": "synthetic", "name": "synth", "num_classes": 6, "retrieval_num": 16, "max_word": 32, "image_resolution": 64},
        "optimizer": {"lr": 0.001, "backbone_lr": 0.00001},
        "run": dict({"arch": runner, "output_dim": 16, "device": 0, "batch_size": 4, "num_workers": 0, "is_train": True, "query_num": 8,
                     "train_num": 8, "epochs": 1, "save_dir": str(tmp_path), "log_dir": str(tmp_path), "seed": 1814}, **run),
    })
    t = registry.get_runner_class(runner).from_config(cfg=cfg, autorun=False)
    t.lines = []
    t.logger = types.SimpleNamespace(info=t.lines.append)
    return t


@pytest.mark.parametrize("arch,runner", [("DCMHT", "DCMHTTrainer"), ("DSPH", "DSPHTrainer")])
def test_train_epoch_moves_every_parameter_and_repeats_to_the_bit(tmp_path, arch, runner):
    finals = []
    for _ in range(2):
        t = _trainer(tmp_path, arch, runner)
        before = {n: p.detach().clone() for n, p in t.model.named_parameters()}
        assert getattr(t, "optimizer", None) is None
        t.train_epoch(0)
        steps = len(t.train_loader)
        assert steps == 2 and t.global_step == steps
        line = t.lines[-1]
        loss = float(re.search(r"loss: (?:tensor\()?([-+0-9.eE]+|nan|inf)", line).group(1))
        print(line)
        assert np.isfinite(loss) and "lr: " in line
        for n, p in t.model.named_parameters():
            if n == "backbone.logit_scale":
                assert torch.equal(p.detach(), before[n]) and p.grad is None
            elif n.startswith("backbone.") or n.startswith("hash."):
                assert not torch.equal(p.detach(), before[n]), n
                assert bool(torch.isfinite(p).all()), n
                assert t.optimizer.state[p]["step"] == steps, n
        if arch == "DSPH":
            assert not torch.equal(t.model.hyp.proxies.detach(), before["hyp.proxies"])
        group = t.optimizer.param_groups[1]
        assert set(t.optimizer.get_lr()) == {t.optimizer._scheduled(g, steps) for g in t.optimizer.param_groups} and group["t_total"] == steps
        finals.append({n: p.detach().clone() for n, p in t.model.named_parameters()})
    assert all(torch.equal(finals[0][n], finals[1][n]) for n in finals[0])


def test_ten_steps_on_one_batch_lower_the_dcmht_loss(tmp_path):
    t = _trainer(tmp_path, "DCMHT", "DCMHTTrainer", epochs=10)
    t.train_loader = [next(iter(t.train_loader))]                                # one fixed batch per epoch
    losses = []
    for epoch in range(10):
        t.train_epoch(epoch)
        losses.append(float(re.search(r"loss: (?:tensor\()?([-+0-9.eE]+|nan|inf)", t.lines[-1]).group(1)))
    print("losses", " ".join("%.6f" % v for v in losses))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]


def test_train_runs_to_the_end_and_the_other_methods_keep_raising(tmp_path):
    t = _trainer(tmp_path, "DCMHT", "DCMHTTrainer")
    t.train()                                                                    # train_epoch and valid for each epoch
    assert any("FINISHED" in line for line in t.lines)
    t.distributed = True
    with pytest.raises(NotImplementedError, match="all-reduce"):
        t.train_epoch(0)
