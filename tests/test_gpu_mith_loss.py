"""GPU: MITH's training objective (xmh_mith_loss.hip behind MITH.object_function) against the goldens the reference's own MITH
produced (buffer, loss_dict and loss.backward() into the eight inputs, step after step on one instance), and against the float64
restatement of oracle/losses.py at the production shapes; accumulation, bit-reproducibility, no host synchronisation, autograd's
version check and double backward, the trainer, and a few SGD steps."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle.fixtures import grads_close
from oracle.losses import MITH_CASES as CASES, MITH_INPUTS as INPUTS, MITH_WEIGHTS as WEIGHTS, load_mith as load, mith_oracle, mith_terms

pytestmark = pytest.mark.gpu

DEFAULT = dict(zip(WEIGHTS, (1.0, 1.0, 50.0, 10.0, 8.0, 0.01, 0.99)))


def _model(buf0, weights=DEFAULT):
    """a MITH whose loss state is set by hand: the objective reads the weights and the buffer only, no backbone is needed"""
    from xmh.models.mith import MITH
    m = MITH.__new__(MITH)
    torch.nn.Module.__init__(m)
    for k in WEIGHTS:
        setattr(m, k, float(weights[k]))
    m._bind_buffer(torch.as_tensor(np.asarray(buf0), dtype=torch.float32).clone())
    return m


def _leaves(d):
    return [d["All loss"], d["LikeHood"]["intra_tokens"]["image"], d["LikeHood"]["intra_tokens"]["text"], d["LikeHood"]["cls_inter"]["image"],
            d["LikeHood"]["cls_inter"]["text"], d["Quantization"]["image"], d["Quantization"]["text"], d["InfoNCE"]["cls"],
            d["InfoNCE"]["tokens"], d["Distillation"]]


def _raw(xs, Y, S, w=DEFAULT, upstream=None, grads=None, accumulate=0):
    """out10 (float64 [10]) and the eight gradients straight from the C ABI"""
    from xmh import _lib
    from xmh._lib import check, current_stream, lib, ptr
    B, K = xs[2].shape
    D = xs[0].shape[1]
    N = Y.shape[0]
    a = _lib.MithLossArgs(N, B, K, D, *(t.data_ptr() for t in xs), Y.data_ptr(), S.data_ptr(), *(w[k] for k in WEIGHTS), 0.07)
    ws = torch.empty(lib.xmh_mith_loss_ws_bytes(N, B, K, D), dtype=torch.uint8, device="cuda")
    out = torch.empty(10, dtype=torch.float64, device="cuda")
    check(lib.xmh_mith_loss(ctypes.byref(a), ptr(ws), ws.numel(), ptr(out), current_stream()), "xmh_mith_loss")
    g = grads if grads is not None else [torch.empty_like(t) for t in xs]
    gp = (ctypes.c_void_p * 8)(*(t.data_ptr() for t in g))
    check(lib.xmh_mith_loss_grad(ctypes.byref(a), ptr(upstream), gp, accumulate, ptr(ws), ws.numel(), current_stream()), "xmh_mith_loss_grad")
    return out, g


def _random(N, B, K, D, seed, normalise=True):
    g = torch.Generator().manual_seed(seed)
    xs = [torch.randn(B, D, generator=g), torch.randn(B, D, generator=g)] + [torch.tanh(torch.randn(B, K, generator=g) * 1.5)
                                                                             for _ in range(4)] \
        + [torch.randn(K, B, D, generator=g), torch.randn(K, B, D, generator=g)]
    if normalise:
        xs = [F.normalize(x, dim=-1) if i in (0, 1, 6, 7) else x for i, x in enumerate(xs)]
    Y = torch.tanh(torch.randn(N, K, generator=g) * 1.5)
    S = (torch.rand(N, B, generator=g) < 0.1).float()
    return xs, Y, S


@pytest.mark.parametrize("name", CASES)
def test_steps_match_the_reference(name):
    N, B, K, D, w, buf0, steps = load(name)
    m = _model(buf0, w)
    for s, st in enumerate(steps):
        xs = [torch.tensor(x).cuda().requires_grad_(True) for x in st["inputs"]]
        loss, d = m.object_function(**dict(zip(INPUTS, xs)), labels=None, indexs=st["indexs"], label_sim=torch.tensor(st["label_sim"]))
        assert m.img_buffer_cls.is_cuda and m.img_buffer_cls is m.txt_buffer_tokens
        assert np.array_equal(m.img_buffer_cls.cpu().numpy(), st["buf"]), (name, s)
        assert loss.is_cuda and loss.dim() == 0 and loss.dtype == torch.float32 and loss.requires_grad
        got = np.array([float(v) for v in _leaves(d)])
        assert all(not v.requires_grad and v.dim() == 0 and v.is_cuda for v in _leaves(d))
        assert np.allclose(got, st["terms"], rtol=2e-5, atol=1e-6), (name, s, got, st["terms"])
        loss.backward()
        for k, x, ref in zip(INPUTS, xs, st["grads"]):
            assert x.grad.shape == ref.shape
            assert grads_close(x.grad.cpu().numpy(), ref), (name, s, k, np.abs(x.grad.cpu().numpy() - ref).max(), np.abs(ref).max())


SHAPES = [(10000, 100, 16, 512), (10000, 128, 128, 512), (10500, 1, 64, 512), (10000, 100, 32, 512), (10500, 128, 16, 512),
          (10000, 1, 128, 512), (10500, 100, 128, 512), (10000, 128, 64, 512)]


@pytest.mark.parametrize("shape", SHAPES)
def test_production_shapes_against_the_restatement(shape):
    N, B, K, D = shape
    xs, Y, S = _random(N, B, K, D, seed=sum(shape))
    out, grads = _raw([x.cuda() for x in xs], Y.cuda(), S.cuda())
    want, wgrads = mith_oracle(xs, Y, S, DEFAULT)
    got = out.cpu().numpy()
    assert np.allclose(got, want, rtol=2e-5, atol=1e-6), (shape, got, want)
    for k, a, b in zip(INPUTS, grads, wgrads):
        assert grads_close(a.cpu().numpy(), b), (shape, k, np.abs(a.cpu().numpy() - b).max(), np.abs(b).max())


def test_accumulate_upstream_and_null_gradients():
    xs, Y, S = _random(700, 40, 24, 72, seed=9, normalise=False)
    xs, Y, S = [x.cuda() for x in xs], Y.cuda(), S.cuda()
    _, g1 = _raw(xs, Y, S)
    base = [torch.full_like(t, 3.0) for t in g1]
    up = torch.tensor([0.5], device="cuda")
    _, g2 = _raw(xs, Y, S, upstream=up, grads=[t.clone() for t in base], accumulate=1)
    for a, b, c in zip(g2, g1, base):
        assert torch.allclose(a, c + 0.5 * b, rtol=1e-6, atol=1e-6)
    from xmh import _lib
    from xmh._lib import check, current_stream, lib, ptr
    a = _lib.MithLossArgs(700, 40, 24, 72, *(t.data_ptr() for t in xs), Y.data_ptr(), S.data_ptr(), *(DEFAULT[k] for k in WEIGHTS), 0.07)
    ws = torch.empty(lib.xmh_mith_loss_ws_bytes(700, 40, 24, 72), dtype=torch.uint8, device="cuda")
    only = torch.zeros_like(xs[3])
    gp = (ctypes.c_void_p * 8)(*([None] * 3 + [only.data_ptr()] + [None] * 4))     # txt_cls_hash alone
    check(lib.xmh_mith_loss_grad(ctypes.byref(a), None, gp, 0, ptr(ws), ws.numel(), current_stream()), "xmh_mith_loss_grad")
    assert torch.equal(only, g1[3])


def test_two_calls_are_bit_identical():
    xs, Y, S = _random(10000, 100, 64, 512, seed=13)
    xs, Y, S = [x.cuda() for x in xs], Y.cuda(), S.cuda()
    o1, g1 = _raw(xs, Y, S)
    o2, g2 = _raw(xs, Y, S)
    assert torch.equal(o1, o2) and all(torch.equal(a, b) for a, b in zip(g1, g2))


def test_forward_and_backward_do_not_synchronise():
    N, B, K, D = 2000, 32, 16, 128
    xs, Y, S = _random(N, B, K, D, seed=17)
    m = _model(Y)
    xs = [x.cuda().requires_grad_(True) for x in xs]
    idx = torch.randperm(N)[:B].cuda()
    m.object_function(**dict(zip(INPUTS, [x.detach() for x in xs])), indexs=idx, label_sim=S.cuda())   # moves the buffer once
    S, labels = S.cuda(), None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss, _ = m.object_function(**dict(zip(INPUTS, xs)), labels=labels, indexs=idx, label_sim=S)
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(x.grad is not None for x in xs)


def test_in_place_buffer_write_before_backward_fails_the_version_check():
    xs, Y, S = _random(300, 8, 16, 64, seed=19)
    m = _model(Y)
    xs = [x.cuda().requires_grad_(True) for x in xs]
    loss, _ = m.object_function(**dict(zip(INPUTS, xs)), indexs=np.arange(8), label_sim=S)
    m.img_buffer_cls[np.arange(8, 16)] = xs[5].detach()                  # the next step's write, as the reference does it
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        loss.backward()


def test_double_backward_raises():
    xs, Y, S = _random(300, 8, 16, 64, seed=23)
    m = _model(Y)
    xs = [x.cuda().requires_grad_(True) for x in xs]
    loss, _ = m.object_function(**dict(zip(INPUTS, xs)), indexs=np.arange(8), label_sim=S.cuda())
    (g,) = torch.autograd.grad(loss, xs[2], create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()


def test_trainer_compute_loss_reaches_every_input():
    """runners/MITH/runner.py:84-96, :118-121: compute_loss -> loss.backward(); label_sim from the train labels on the device"""
    from xmh.runners.methods import MITHTrainer
    N, B, K, D = 400, 12, 16, 64
    xs, Y, _ = _random(N, B, K, D, seed=29)
    t = MITHTrainer.__new__(MITHTrainer)
    t.model, t.display_step = _model(Y), 20
    g = torch.Generator().manual_seed(5)
    t.train_labels = (torch.rand(N, 24, generator=g) < 0.1).float()
    index = np.arange(100, 100 + B)
    label = t.train_labels[index]                                      # the loader hands labels over on the host
    xs = [x.cuda().requires_grad_(True) for x in xs]
    loss = t.compute_loss(**dict(zip(INPUTS, xs)), label=label, index=index, epoch=0, times=1, global_step=1)
    loss.backward()
    assert all(float(x.grad.abs().sum()) > 0 for x in xs)
    S = ((t.train_labels @ label.T) > 0).float()
    want, _ = mith_oracle([x.detach().cpu() for x in xs], t.model.img_buffer_cls.cpu(), S, DEFAULT)
    assert abs(float(loss) - want[0]) <= 2e-5 * abs(want[0]) + 1e-6


def test_sgd_steps_track_the_restatement():
    """three SGD steps of the eight inputs, each step writing the buffer, follow the float64 trajectory"""
    N, B, K, D = 500, 16, 32, 64
    xs, Y, S = _random(N, B, K, D, seed=31)
    m = _model(Y)
    p = [x.clone().cuda().requires_grad_(True) for x in xs]
    pd = [x.clone().double().requires_grad_(True) for x in xs]
    Yd = Y.clone().double()
    opt, opt_d = torch.optim.SGD(p, lr=0.01), torch.optim.SGD(pd, lr=0.01)
    for step in range(3):
        idx = np.arange(step * 10, step * 10 + B)
        opt.zero_grad()
        opt_d.zero_grad()
        loss, _ = m.object_function(**dict(zip(INPUTS, p)), indexs=idx, label_sim=S.cuda())
        loss.backward()
        Yd[idx] = pd[5].detach()
        want = mith_terms(pd, Yd, S.double(), DEFAULT)[0]
        want.backward()
        assert abs(float(loss) - float(want)) <= 2e-5 * abs(float(want)) + 1e-6
        opt.step()
        opt_d.step()
    for a, b in zip(p, pd):
        assert float((a.detach().cpu().double() - b.detach()).abs().max()) <= 1e-5 * float(b.detach().abs().max()) + 1e-7
