"""GPU: DSPH's HyP loss (xmh_hyp.hip behind HyPProxies.forward / DSPH.object_function) against the goldens the reference's own
HyP produced (loss and loss.backward() into the codes and the proxies), and against the float64 restatement of
oracle/losses.py on other shapes, thresholds and label dtypes; NaN cases, accumulation, bit-reproducibility, no host
synchronisation, and a few SGD steps of the proxies and codes."""
import numpy as np
import pytest
import torch

from oracle.fixtures import grads_close_rows as grads_close
from oracle.losses import HYP_CASES as CASES, HYP_TERMS as TERMS, hyp_oracle, hyp_terms, load_hyp as load

pytestmark = pytest.mark.gpu


def _model(K, C, threshold, alpha, proxies=None):
    from xmh.models.dsph import DSPH, HyPProxies
    m = DSPH.__new__(DSPH)                                     # the loss reads the hyp module only; no backbone needed here
    torch.nn.Module.__init__(m)
    m.hyp = HyPProxies(numclass=C, output_dim=K, alpha=alpha, threshold=threshold)
    if proxies is not None:
        with torch.no_grad():
            m.hyp.proxies.copy_(torch.as_tensor(proxies))
    return m.cuda()


def _raw(x, y, P, labels, threshold, alpha, upstream=None, grads=None, accumulate=0):
    """out8 (float64 [8]) and (gx, gy, gP) straight from the C ABI"""
    from xmh import retrieval as R
    from xmh._lib import check, current_stream, lib, ptr
    B, K = x.shape
    C = P.shape[0]
    lab = R.pack_labels(labels)
    ws = torch.empty(lib.xmh_hyp_loss_ws_bytes(B, K, C), dtype=torch.uint8, device="cuda")
    out = torch.empty(8, dtype=torch.float64, device="cuda")
    args = (ptr(x), ptr(y), ptr(P), B, K, C, ptr(lab), float(threshold), float(alpha))
    check(lib.xmh_hyp_loss(*args, ptr(ws), ws.numel(), ptr(out), current_stream()), "xmh_hyp_loss")
    g = grads if grads is not None else (torch.empty_like(x), torch.empty_like(y), torch.empty_like(P))
    check(lib.xmh_hyp_loss_grad(*args, ptr(upstream), *(ptr(t) for t in g), accumulate, ptr(ws), ws.numel(), current_stream()),
          "xmh_hyp_loss_grad")
    return out, g


def _labels(g, B, C, p):
    L = (torch.rand(B, C, generator=g) < p).float()
    L[torch.arange(B), torch.randint(0, C, (B,), generator=g)] = 1.0
    return L


@pytest.mark.parametrize("name", CASES)
def test_forward_and_gradients_match_the_reference(name):
    x, y, P, labels, threshold, alpha, loss_ref, (rgx, rgy, rgP) = load(name)
    m = _model(x.shape[1], P.shape[0], threshold, alpha, P)
    gx, gy = torch.tensor(x).cuda().requires_grad_(True), torch.tensor(y).cuda().requires_grad_(True)
    loss, d = m.object_function(gx, gy, labels=None if labels is None else torch.tensor(labels).cuda())
    assert loss.is_cuda and loss.dim() == 0 and loss.dtype == torch.float32 and loss.requires_grad
    assert not d["All loss"].requires_grad and float(d["All loss"]) == float(loss.detach())
    assert np.allclose(float(loss), loss_ref, rtol=2e-5, atol=1e-6), (name, float(loss), loss_ref)
    loss.backward()
    for got, ref in ((gx.grad, rgx), (gy.grad, rgy), (m.hyp.proxies.grad, rgP)):
        assert got.shape == ref.shape
        assert grads_close(got.cpu().numpy(), ref), (name, np.abs(got.cpu().numpy() - ref).max(), np.abs(ref).max())


SHAPES = [(1, 16, 1), (1, 64, 21), (33, 16, 21), (33, 2048, 80), (128, 128, 80), (128, 64, 1024), (33, 128, 24),
          (4096, 16, 80), (4096, 128, 24), (128, 2048, 1024), (4096, 512, 21)]
DTYPES = [torch.float32, torch.int64, torch.int32, torch.uint8, torch.bool]


@pytest.mark.parametrize("case", range(len(SHAPES)))
def test_against_the_restatement_on_other_shapes(case):
    B, K, C = SHAPES[case]
    threshold = (-0.2, 0.0, 0.25)[case % 3]
    dtype = DTYPES[case % len(DTYPES)]
    g = torch.Generator().manual_seed(100 + case)
    x, y = torch.tanh(torch.randn(B, K, generator=g) * 1.5), torch.tanh(torch.randn(B, K, generator=g) * 1.5)
    P = torch.randn(C, K, generator=g) * (2.0 / C) ** 0.5
    labels = _labels(g, B, C, 2.5 / C)
    out, (gx, gy, gP) = _raw(x.cuda(), y.cuda(), P.cuda(), labels.to(dtype).cuda(), threshold, 0.8)
    want, wx, wy, wP = hyp_oracle(x, y, P, labels, threshold, 0.8)
    got = out.cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want)), (B, K, C, got, want)
    assert np.allclose(got, want, rtol=2e-5, atol=1e-6, equal_nan=True), (B, K, C, got, want)
    # At B = 4096 there are ~10^7 regulariser pairs: a few similarities sit so close to the threshold that fp32 and float64 put
    # them on different sides, and each such relu' decision moves one code row's gradient by at most 2 alpha / Z * |v_j / |v_j|| /
    # |v_i| per element.  Allow four of them on top of the relative tolerance (the golden cases above get none).
    L = labels != 0
    multi = L[L.sum(1) > 1].double()
    Z = float(((multi @ multi.T) == 0).sum())
    flip = (1.6 / Z if Z else 0.0) * float(max(1.0 / t.norm(dim=1).clamp_min(1e-12).min() for t in (x, y)))
    for a, b in ((gx, wx), (gy, wy), (gP, wP)):
        err = np.abs(a.cpu().numpy().astype(np.float64) - b).max()
        assert err <= 2e-5 * np.abs(b).max() + 4 * flip + 1e-9, (B, K, C, err, np.abs(b).max(), flip)


def test_nan_where_the_reference_divides_zero_by_zero():
    g = torch.Generator().manual_seed(5)
    B, K, C = 20, 32, 6
    x, y, P = torch.randn(B, K, generator=g), torch.randn(B, K, generator=g), torch.randn(C, K, generator=g)
    for labels, nan_terms in ((torch.zeros(B, C), ("pos", "pos_t")), (torch.ones(B, C), ("neg", "neg_t"))):
        out, grads = _raw(x.cuda(), y.cuda(), P.cuda(), labels.cuda(), 0.1, 0.8)
        got = out.cpu().numpy()
        want, *wgrads = hyp_oracle(x, y, P, labels, 0.1, 0.8)
        for k, v, w in zip(TERMS, got, want):
            assert np.isnan(v) == (k in nan_terms or k == "loss") == np.isnan(w), (k, v, w)
        assert np.allclose(got, want, rtol=2e-5, atol=1e-6, equal_nan=True)
        for a, b in zip(grads, wgrads):
            assert torch.isfinite(a).all() and grads_close(a.cpu().numpy(), b)


def test_accumulate_and_upstream():
    g = torch.Generator().manual_seed(9)
    B, K, C = 40, 64, 30
    x, y, P = (torch.randn(*s, generator=g).cuda() for s in ((B, K), (B, K), (C, K)))
    labels = _labels(g, B, C, 0.1).cuda()
    _, g1 = _raw(x, y, P, labels, 0.0, 0.8)
    base = tuple(torch.full_like(t, 3.0) for t in g1)
    up = torch.tensor([0.5], device="cuda")
    _, g2 = _raw(x, y, P, labels, 0.0, 0.8, upstream=up, grads=tuple(t.clone() for t in base), accumulate=1)
    for a, b, c in zip(g2, g1, base):
        assert torch.allclose(a, c + 0.5 * b, rtol=1e-6, atol=1e-6)


def test_two_calls_are_bit_identical():
    g = torch.Generator().manual_seed(13)
    B, K, C = 1000, 128, 80
    x, y = torch.tanh(torch.randn(B, K, generator=g)).cuda(), torch.tanh(torch.randn(B, K, generator=g)).cuda()
    P = torch.randn(C, K, generator=g).cuda()
    labels = _labels(g, B, C, 0.04).cuda()
    o1, g1 = _raw(x, y, P, labels, 0.0, 0.8)
    o2, g2 = _raw(x, y, P, labels, 0.0, 0.8)
    assert torch.equal(o1, o2) and all(torch.equal(a, b) for a, b in zip(g1, g2))


def test_forward_and_backward_do_not_synchronise():
    g = torch.Generator().manual_seed(17)
    m = _model(16, 80, 0.25, 0.8)
    x = torch.tanh(torch.randn(100, 16, generator=g)).cuda().requires_grad_(True)
    y = torch.tanh(torch.randn(100, 16, generator=g)).cuda().requires_grad_(True)
    labels = _labels(g, 100, 80, 0.05).cuda()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss, _ = m.object_function(x, y, labels)
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert x.grad is not None and m.hyp.proxies.grad is not None


def test_object_function_defaults_and_errors():
    m = _model(16, 24, 0.0, 0.8)
    x, y = torch.rand(24, 16).cuda().requires_grad_(True), torch.rand(24, 16).cuda()
    loss, _ = m.object_function(x, y)                                          # identity labels, numclass == B
    loss.backward()
    assert m.hyp.proxies.grad is not None and m.hyp.proxies.grad.abs().sum() > 0 and x.grad is not None and y.grad is None
    with pytest.raises(RuntimeError):
        m.object_function(torch.rand(20, 16).cuda(), torch.rand(20, 16).cuda())        # [B, B] identity against 24 proxies
    with pytest.raises(RuntimeError):
        m.object_function(torch.rand(4, 16), torch.rand(4, 16), torch.ones(4, 24))   # no CPU fallback
    loss2, _ = m.object_function(x.detach(), y, torch.eye(24))                         # labels on the host are moved
    assert float(loss2) == float(loss)


def test_sgd_steps_track_the_restatement():
    """runners/DSPH/runner.py:83-91, 120-125: the proxies stepped by their own SGD (lr 0.02, momentum 0.9, weight decay 5e-4), the
    codes by another; three steps of both follow the float64 restatement's trajectory"""
    g = torch.Generator().manual_seed(21)
    B, K, C = 64, 16, 80
    x0, y0 = torch.tanh(torch.randn(B, K, generator=g) * 1.5), torch.tanh(torch.randn(B, K, generator=g) * 1.5)
    P0 = torch.randn(C, K, generator=g) * (2.0 / C) ** 0.5
    labels = _labels(g, B, C, 0.05)
    m = _model(K, C, 0.25, 0.8, P0)
    x, y = x0.clone().cuda().requires_grad_(True), y0.clone().cuda().requires_grad_(True)
    xd, yd, Pd = (t.clone().double().requires_grad_(True) for t in (x0, y0, P0))
    opt = [torch.optim.SGD(m.hyp.parameters(), lr=0.02, momentum=0.9, weight_decay=5e-4), torch.optim.SGD([x, y], lr=0.05)]
    opt_d = [torch.optim.SGD([Pd], lr=0.02, momentum=0.9, weight_decay=5e-4), torch.optim.SGD([xd, yd], lr=0.05)]
    for _ in range(3):
        for o in opt + opt_d:
            o.zero_grad()
        loss, _ = m.object_function(x, y, labels.cuda())
        loss.backward()
        want = hyp_terms(xd, yd, Pd, labels, 0.25, 0.8)["loss"]
        want.backward()
        assert abs(float(loss) - float(want)) <= 2e-5 * abs(float(want)) + 1e-6
        for o in opt + opt_d:
            o.step()
    for a, b in ((m.hyp.proxies, Pd), (x, xd), (y, yd)):
        assert float((a.detach().cpu().double() - b.detach()).abs().max()) <= 1e-5 * float(b.detach().abs().max())


def test_trainer_compute_loss_is_differentiable():
    """runners/DSPH/runner.py:93-101, :118-125: compute_loss -> loss.backward() reaches the codes and the proxies"""
    from xmh.runners.methods import DSPHTrainer
    t = DSPHTrainer.__new__(DSPHTrainer)
    t.model, t.display_step = _model(16, 7, 0.25, 0.8), 20
    g = torch.Generator().manual_seed(5)
    img = torch.rand(12, 16, generator=g).cuda().requires_grad_(True)
    txt = torch.rand(12, 16, generator=g).cuda().requires_grad_(True)
    label = (torch.rand(12, 7, generator=g) < 0.3).float()                     # the loader hands labels over on the host
    label[:, 0] = 1.0
    loss = t.compute_loss(img_hash=img, txt_hash=txt, label=label, index=None, epoch=0, times=1, global_step=1)
    loss.backward()
    assert img.grad.abs().sum() > 0 and txt.grad.abs().sum() > 0 and t.model.hyp.proxies.grad.abs().sum() > 0
