"""GPU: backward of the CLIP block stack (xmh_block_grad.hip behind torch.autograd in Transformer.run_train) against the goldens of the
reference's own Transformer and against the float64 restatement of tests/block_grad_cases.py on other shapes; the forward's bit
identity with run_saved, reproducibility, the accumulate flag, frozen parameters, the early stop, no host synchronisation, argument
errors, and a few SGD steps.

Tolerances.  Per tensor, e = max|got - fp64| / max|fp64|.  The yardstick is the reference's own fp32 error e_ref stored in the golden
file per tensor: the port must stay within TOL_FACTOR * max(e_ref over the committed cases of that tensor kind) -- the factor and
pooling rule of tests/test_gpu_head_grad.py, whose docstring gives the reason; against the thinned fp32 golden itself the factor is
TOL_FACTOR + 1 by the triangle inequality.  On the other shapes the dot products are longer than in the pool, so the yardstick per
kind is TOL_FACTOR * max(pool, e_ref of that very case), the latter measured in the test from the restatement's fp32 run on the CPU."""
import numpy as np
import pytest
import torch

import block_grad_cases as BC

pytestmark = pytest.mark.gpu

TOL_FACTOR = 4.0


def _stack(sd, D, heads, layers):
    from xmh.models.clip import Transformer
    tr = Transformer(D, layers, heads)
    tr.load_state_dict({k: torch.tensor(v) for k, v in sd.items()}, strict=True)
    return tr.cuda()


def _kpm(kpm):
    return None if kpm is None else torch.tensor(kpm).cuda()


def _collect(tr, y, xt):
    out = {"y": y.detach().cpu().numpy(), "g_x": None if xt.grad is None else xt.grad.cpu().numpy()}
    for i, blk in enumerate(tr.resblocks):
        for (kind, _), p in zip(BC.PARAMS, tr._train_params(blk)):
            out["g_l%d_%s" % (i, kind)] = None if p.grad is None else p.grad.cpu().numpy()
    return out


def _step(tr, x, up, causal, kpm, x_grad=True):
    xt = torch.tensor(x).cuda().requires_grad_(x_grad)
    y = tr.run_train(xt, causal=causal, key_padding_mask=_kpm(kpm))
    assert y.requires_grad and y.dtype == torch.float32 and y.is_cuda and y.data_ptr() != xt.data_ptr()
    assert torch.equal(xt.detach().cpu(), torch.tensor(x))                       # the caller's tensor is not touched
    (y * torch.tensor(up).cuda()).sum().backward()
    return _collect(tr, y, xt)


_refs = {}


def _reference(key, sd, x, up, heads, causal, kpm, with_f32=False):
    """the float64 restatement (and its fp32 run where asked for), computed once per key and shared"""
    if key not in _refs:
        r64 = BC.run_restatement(sd, x, up, heads, causal, kpm, torch.float64)
        pool = BC.erefs(BC.run_restatement(sd, x, up, heads, causal, kpm, torch.float32), r64)[1] if with_f32 else {}
        _refs[key] = (r64, pool)
    return _refs[key]


def _check(got, R, what, own=None, kinds=None):
    """every figure is printed before the first assertion"""
    rows = []
    for k in R:
        kind = BC.kind_of(k)
        if got[k] is None or (kinds is not None and kind not in kinds):
            continue
        tol = TOL_FACTOR * max(BC.pool_eref(kind), (own or {}).get(kind, 0.0))
        rows.append((k, BC.rel_err(got[k], R[k]), tol))
    print(what, " ".join("%s %.2e/%.2e" % r for r in rows))
    worst = {}
    for k, e, tol in rows:
        kind = BC.kind_of(k)
        worst[kind] = max(worst.get(kind, 0.0), e / (tol / TOL_FACTOR))
    print(what, "e_port / e_ref per kind:", " ".join("%s %.2f" % (k, v) for k, v in worst.items()))
    for k, e, tol in rows:
        assert got[k].shape == R[k].shape and np.isfinite(got[k]).all(), (what, k)
        assert e <= tol, (what, k, e, tol)
    return rows


# 1 goldens -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(BC.CASES))
def test_every_gradient_matches_the_reference(case):
    G = BC.golden()
    D, heads, layers, L, B, causal, kp = BC.CASES[case]
    sd, x, up, kpm = BC.case_inputs(case)
    assert BC.inputs_checksum(sd, x, up, kpm) == float(G[case + "__checksum"])
    R, _ = _reference(case, sd, x, up, heads, causal, kpm)
    got = _step(_stack(sd, D, heads, layers), x, up, causal, kpm)
    assert sorted(got) == sorted(R) and all(v is not None for v in got.values())
    rows = []
    for k in R:
        err = np.abs(BC.thin(got[k]).astype(np.float64) - G["%s__%s" % (case, k)].astype(np.float64)).max() / (np.abs(R[k]).max() or 1.0)
        rows.append((k, err, (TOL_FACTOR + 1) * BC.pool_eref(BC.kind_of(k))))
    print(case, "against the fp32 golden:", " ".join("%s %.2e/%.2e" % r for r in rows))
    _check(got, R, case)
    for k, err, tol in rows:
        assert err <= tol, (case, "golden", k, err, tol)


# 2 other shapes ----------------------------------------------------------------------------------------------------------------
SHAPES = [(64, 1, 1, 50, 41, False, False),     # M = 2050: several M chunks of the TN product plus a remainder
          (128, 2, 1, 128, 1, True, False),     # the L limit
          (128, 2, 1, 77, 2, True, True),       # CLIP's context
          (128, 2, 1, 64, 2, False, False),     # the forward's attention-kernel boundary, from below
          (768, 12, 1, 50, 2, False, False),    # one ViT-B/32 block
          (512, 8, 2, 32, 2, True, False)]      # the text tower and MITH's token transformer


def _shape_inputs(shape):
    D, heads, layers, L, B, causal, kp = shape
    seed = 5000 + D + 7 * L + B
    x, up = BC.draw_batch(seed, B, L, D)
    return BC.draw_params(seed, D, layers), x, up, (BC.draw_kpm(seed, B, L) if kp else None)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "d%d_h%d_n%d_l%d_b%d%s%s" % (s[:5] + ("_causal" if s[5] else "", "_kpm" if s[6] else "")))
def test_against_the_restatement_on_other_shapes(shape):
    D, heads, layers, L, B, causal, kp = shape
    sd, x, up, kpm = _shape_inputs(shape)
    R, own = _reference(shape, sd, x, up, heads, causal, kpm, with_f32=True)
    print("e_ref of this case:", " ".join("%s %.2e" % (k, own[k]) for k in BC.KINDS))
    got = _step(_stack(sd, D, heads, layers), x, up, causal, kpm)
    _check(got, R, "D=%d heads=%d layers=%d L=%d B=%d" % shape[:5], own=own)


# 3 forward ---------------------------------------------------------------------------------------------------------------------
def test_forward_is_run_saved_in_exact_mode_and_no_grad_keeps_no_record(monkeypatch):
    from xmh import ops
    from xmh._lib import lib
    case = "d64_l33_b5_causal_kpm"
    D, heads, layers, L, B, causal, kp = BC.CASES[case]
    sd, x, up, kpm = BC.case_inputs(case)
    tr = _stack(sd, D, heads, layers)
    xs = torch.tensor(x).cuda()
    y = tr.run_train(xs.clone().requires_grad_(True), causal=causal, key_padding_mask=_kpm(kpm))
    before = ops.get_precision()
    ops.set_precision("f32x")
    try:
        want, _ = tr.run_saved(xs.clone(), causal=causal, key_padding_mask=_kpm(kpm))
        plain = tr.run(xs.clone(), causal=causal, key_padding_mask=_kpm(kpm))
    finally:
        ops.set_precision(before)
    assert torch.equal(y.detach(), want) and torch.equal(want, plain)

    def boom(*a, **k):
        raise AssertionError("not under no_grad")
    monkeypatch.setattr(lib, "xmh_clip_blocks_backward", boom)
    monkeypatch.setattr(lib, "xmh_clip_blocks_forward_saved", boom)
    with torch.no_grad():
        z = tr.run_train(xs, causal=causal, key_padding_mask=_kpm(kpm))
    assert not z.requires_grad and z.grad_fn is None and torch.equal(z, want) and torch.equal(xs.cpu(), torch.tensor(x))
    for p in tr.parameters():
        p.requires_grad_(False)
    z = tr.run_train(xs, causal=causal, key_padding_mask=_kpm(kpm))              # nothing to differentiate: the same plain forward
    assert not z.requires_grad and torch.equal(z, want)


# 4 reproducibility, accumulation, the early stop (through the C entry) ---------------------------------------------------------
class _CEntry:
    """forward kept once; backward through the C ABI with chosen pointers"""

    def __init__(self, case):
        from xmh.models import clip_train as CT
        self.CT = CT
        self.D, self.heads, self.layers, self.L, self.B, self.causal, _ = BC.CASES[case]
        sd, x, up, kpm = BC.case_inputs(case)
        self.tr = _stack(sd, self.D, self.heads, self.layers)
        self.params = CT.block_params(self.tr)
        self.kpm = None if kpm is None else torch.tensor(kpm).cuda().to(torch.uint8)
        self.up = torch.tensor(up).cuda()
        self.y, self.buf, self.blocks, self.keep = CT.blocks_forward(self.tr, torch.tensor(x).cuda(), self.causal, self.kpm, self.params)

    def backward(self, want, need_dx=1, accumulate=0, init=None, buf=None, saved_bytes=None, ws_bytes=None, dy="up", width=None, heads=None,
                 L=None):
        """want(layer, kind) -> bool; init: value the gradient buffers hold before the call -> ({name: tensor}, dy, rc)"""
        from xmh._lib import current_stream, lib, ptr
        bufs, gp = {}, []
        kinds = [(i, kind) for i in range(self.layers) for kind, _ in self.CT.BLOCK]
        for (i, kind), p in zip(kinds, self.params):
            t = None
            if want(i, kind):
                t = torch.full_like(p, float("nan")) if init is None else init["g_l%d_%s" % (i, kind)].clone()
                bufs["g_l%d_%s" % (i, kind)] = t
            gp.append(t)
        grads = self.CT.block_grads(gp)
        dyt = self.up.clone() if dy == "up" else None
        buf = self.buf if buf is None else buf
        n = lib.xmh_clip_blocks_backward_ws_bytes(self.B, self.L, self.D)
        ws = torch.empty(n, dtype=torch.uint8, device="cuda")
        rc = lib.xmh_clip_blocks_backward(self.blocks, self.layers, width or self.D, heads or self.heads, self.B, L or self.L, int(self.causal),
                                          ptr(self.kpm), ptr(buf), buf.numel() * 4 if saved_bytes is None else saved_bytes, ptr(dyt), need_dx,
                                          grads, accumulate, ptr(ws), n if ws_bytes is None else ws_bytes, current_stream())
        return bufs, dyt, rc


def test_two_backwards_agree_to_the_bit_and_accumulate_adds():
    c = _CEntry("d128_l65_b2")
    every = lambda i, k: True                                                    # noqa: E731
    a, dxa, rc = c.backward(every)
    assert rc == 0
    b, dxb, rc = c.backward(every)
    assert rc == 0 and torch.equal(dxa, dxb) and all(torch.equal(a[k], b[k]) for k in a) and len(a) == 24
    assert all(bool(torch.isfinite(t).all()) for t in a.values())
    g = torch.Generator(device="cuda").manual_seed(3)
    g0 = {k: torch.randn(t.shape, device="cuda", generator=g) for k, t in a.items()}
    acc, dxc, rc = c.backward(every, accumulate=1, init=g0)
    assert rc == 0 and torch.equal(dxc, dxa)                                     # an activation gradient: written, never added to
    for k in a:
        assert torch.equal(acc[k], g0[k] + a[k]), k
    # through autograd: two run_train + backward on fresh copies of the stack
    D, heads, layers, L, B, causal, _ = BC.CASES["d128_l65_b2"]
    sd, x, up, kpm = BC.case_inputs("d128_l65_b2")
    s1, s2 = (_step(_stack(sd, D, heads, layers), x, up, causal, kpm) for _ in range(2))
    assert all(np.array_equal(s1[k], s2[k]) for k in s1)
    assert all(np.array_equal(s1[k], a[k].cpu().numpy()) for k in a) and np.array_equal(s1["g_x"], dxa.cpu().numpy())


def test_early_stop_reads_nothing_below_the_lowest_trained_layer():
    c = _CEntry("d64_l33_b5_causal_kpm")                                         # three layers
    full, _, rc = c.backward(lambda i, k: True)
    assert rc == 0
    per_layer = 16 * c.B * c.L * c.D
    for j, kinds in ((2, None), (1, None), (2, ("proj_w", "fc_b")), (1, ("ln2_w",)), (2, ("qkv_b", "ln1_b"))):
        poisoned = c.buf.clone()
        poisoned[:j * per_layer] = float("nan")                                  # the records of layers 0 .. j-1
        want = lambda i, k: i > j or (i == j and (kinds is None or k in kinds))  # noqa: E731
        got, _, rc = c.backward(want, need_dx=0, buf=poisoned)
        assert rc == 0 and got
        for k, t in got.items():
            assert bool(torch.isfinite(t).all()) and torch.equal(t, full[k]), (j, kinds, k)
    none, dy, rc = c.backward(lambda i, k: False, need_dx=0)                     # nothing asked for: no launch
    assert rc == 0 and not none and torch.equal(dy, c.up)


def test_frozen_parameters_get_none_and_the_others_keep_their_bits():
    case = "d128_l7_b3_causal"
    D, heads, layers, L, B, causal, _ = BC.CASES[case]
    sd, x, up, kpm = BC.case_inputs(case)
    full = _step(_stack(sd, D, heads, layers), x, up, causal, kpm)
    tr = _stack(sd, D, heads, layers)
    frozen = {"resblocks.0.attn.out_proj.weight", "resblocks.0.ln_1.weight", "resblocks.0.mlp.c_fc.bias", "resblocks.1.attn.in_proj_weight",
              "resblocks.1.ln_2.bias", "resblocks.1.mlp.c_proj.weight", "resblocks.1.mlp.c_proj.bias"}
    for n, p in tr.named_parameters():
        p.requires_grad_(n not in frozen)
    got = _step(tr, x, up, causal, kpm, x_grad=False)
    assert got["g_x"] is None
    for i in range(layers):
        for kind, key in BC.PARAMS:
            k, name = "g_l%d_%s" % (i, kind), "resblocks.%d.%s" % (i, key)
            assert (got[k] is None) == (name in frozen), k
            if got[k] is not None:
                assert np.array_equal(got[k], full[k]), k
    # layer 0 frozen as a whole, x without grad: the walk ends above it
    tr = _stack(sd, D, heads, layers)
    for n, p in tr.named_parameters():
        p.requires_grad_(n.startswith("resblocks.1."))
    got = _step(tr, x, up, causal, kpm, x_grad=False)
    for k, v in got.items():
        if k.startswith("g_l1_"):
            assert np.array_equal(v, full[k]), k
        elif k != "y":
            assert v is None, k


def test_whole_stack_frozen_with_x_requiring_grad_computes_dx_alone():
    case = "d192_l50_b2"
    D, heads, layers, L, B, causal, _ = BC.CASES[case]
    sd, x, up, kpm = BC.case_inputs(case)
    tr = _stack(sd, D, heads, layers)
    for p in tr.parameters():
        p.requires_grad_(False)
    got = _step(tr, x, up, causal, kpm)
    R, _ = _reference(case, sd, x, up, heads, causal, kpm)
    assert all(v is None for k, v in got.items() if k.startswith("g_l"))
    _check(got, R, "frozen stack", kinds=("y", "g_x"))


# 5 no host synchronisation -----------------------------------------------------------------------------------------------------
def test_forward_and_backward_do_not_synchronise():
    case = "d128_l7_b3_causal"
    D, heads, layers, L, B, causal, _ = BC.CASES[case]
    sd, x, up, kpm = BC.case_inputs(case)
    tr = _stack(sd, D, heads, layers)
    xt, u = torch.tensor(x).cuda().requires_grad_(True), torch.tensor(up).cuda()
    (tr.run_train(xt, causal=causal) * u).sum().backward()                       # warm the allocator's pools
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        (tr.run_train(xt, causal=causal) * u).sum().backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert xt.grad is not None and all(p.grad is not None for p in tr.parameters())


# 6 argument errors -------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    from xmh._lib import lib
    c = _CEntry("d128_l7_b3_causal")
    every = lambda i, k: True                                                    # noqa: E731
    assert c.backward(every, saved_bytes=c.buf.numel() * 4 - 4)[2] == -12 and b"saved" in lib.xmh_last_error()
    assert c.backward(every, ws_bytes=lib.xmh_clip_blocks_backward_ws_bytes(c.B, c.L, c.D) - 1)[2] == -12
    assert c.backward(every, heads=1)[2] == -95 and c.backward(every, heads=4)[2] == -95
    assert c.backward(every, L=129)[2] == -95
    assert c.backward(every, dy=None)[2] == -22
    assert c.backward(every)[2] == 0


# 7 SGD steps -------------------------------------------------------------------------------------------------------------------
def _sgd_cpu(sd, x, heads, dtype, steps, lr):
    from oracle import encode as enc
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        t = {k: torch.tensor(v).to(dtype).requires_grad_(True) for k, v in sd.items()}
        opt = torch.optim.SGD(list(t.values()), lr=lr)
        xt = torch.tensor(x).to(dtype).transpose(0, 1)
        layers = len({k.split(".")[1] for k in sd})
        losses = []
        for _ in range(steps):
            opt.zero_grad()
            loss = 0.5 * (enc._blocks(xt, t, "", layers, heads, None) ** 2).sum()
            loss.backward()
            opt.step()
            losses.append(float(loss))
        return losses
    finally:
        torch.set_num_threads(threads)


def test_five_sgd_steps_follow_the_restatement():
    D, heads, layers, L, B, steps, lr = 128, 2, 2, 7, 3, 5, 1e-3
    sd = BC.draw_params(77, D, layers)
    x, _ = BC.draw_batch(78, B, L, D)
    l64, l32 = _sgd_cpu(sd, x, heads, torch.float64, steps, lr), _sgd_cpu(sd, x, heads, torch.float32, steps, lr)
    tr = _stack(sd, D, heads, layers)
    opt = torch.optim.SGD(tr.parameters(), lr=lr)
    xs = torch.tensor(x).cuda()
    got = []
    for _ in range(steps):
        opt.zero_grad()
        loss = 0.5 * (tr.run_train(xs) ** 2).sum()
        loss.backward()
        assert all(p.grad is not None for p in tr.parameters())
        opt.step()
        got.append(float(loss))
    dev32 = max(abs(a - b) / abs(b) for a, b in zip(l32, l64))
    dev = max(abs(a - b) / abs(b) for a, b in zip(got, l64))
    print("losses float64", " ".join("%.8f" % v for v in l64))
    print("losses port   ", " ".join("%.8f" % v for v in got))
    print("largest relative deviation: port %.3e, fp32 restatement on the CPU %.3e (allowed %.3e)" % (dev, dev32, 4 * dev32))
    assert l64[-1] < 0.9 * l64[0]                                                # the steps move the loss
    assert dev <= 4 * dev32

