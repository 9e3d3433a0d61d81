"""GPU: the DCMHT objective and its gradient kernels (xmh_loss.hip behind DCMHT.object_function) against the float64 restatement of
tests/dcmht_loss_cases.py (validated against the reference's own numbers by tests/test_dcmht_loss_cpu.py), where the older
tests/test_gpu_losses.py does not look: saturated codes with pairs beyond the euclidean margin (the inactive hinge branch) and at zero
distance, centred codes on both sides of the cosine clamp, batches above the 256 threads of a block, the width limit of the forward,
the LDS limit of the gradient entry, non-finite inputs, reproducibility, the accumulate flag, and no host synchronisation.

Tolerances.  Per kind (the nine terms as one vector, d loss / d image, d loss / d text), e = max|got - fp64| / max|fp64| on whole
tensors.  The port must stay within TOL_FACTOR * max(pool, e_ref): pool = the reference's own fp32 error over the four golden cases,
e_ref = the float32 restatement against the float64 one at the case's own inputs (both computed here, neither hard-coded).  Factor 4
as in tests/test_gpu_head_grad.py: a different but equally long summation order may lose about twice the reference's bits at each of
two chained reductions (here the sum over the code width inside a distance or cosine, then the sum over j).  Each figure is printed
before the first assertion.  The inputs' conditions (shares beyond the margin, gaps to the clamp edges, zero-distance pairs) are
checked again here on the very codes the device produced."""
import numpy as np
import pytest
import torch

import dcmht_loss_cases as DC

pytestmark = pytest.mark.gpu

TOL_FACTOR = 4.0
UPSTREAM = 3.0                       # the loss is scaled after the Function: the upstream gradient goes through the kernels


def _model(K, sim, vartheta=DC.VARTHETA, threshold=DC.THRESHOLD, alpha=DC.ALPHA):
    from xmh.models.dcmht import DCMHT
    m = DCMHT.__new__(DCMHT)                                   # the loss methods read attributes only; no backbone needed here
    torch.nn.Module.__init__(m)
    m.output_dim, m.vartheta, m.threshold, m.similarity_function, m.quan_alpha = K, vartheta, threshold, sim, alpha
    return m


def _vec(loss, d):
    return np.array([float(loss.detach()), float(d["Intra"]["Positive"]), float(d["Intra"]["Negative"]), float(d["Inter"]["Positive"]["i2t"]),
                     float(d["Inter"]["Negative"]["i2t"]), float(d["Inter"]["Positive"]["t2i"]), float(d["Inter"]["Negative"]["t2i"]),
                     float(d["Quan"]["Image"]), float(d["Quan"]["Text"])], dtype=np.float64)


def _device_inputs(c):
    """-> (image, text) device tensors that carry the gradient: [B, K, 2] outputs of a softmax node, or the centred leaves [B, 2K]"""
    if "image" in c:
        return c["image"].cuda().requires_grad_(True), c["text"].cuda().requires_grad_(True)
    out = []
    for key in ("logits_i", "logits_t"):
        x = torch.softmax(c[key].cuda().requires_grad_(True), -1)
        x.retain_grad()
        out.append(x)
    return out


def _step(c, img, txt, labels):
    """object_function + backward of UPSTREAM * loss -> dict(terms, g_img, g_txt) as float64 numpy, gradients per unit of upstream"""
    loss, d = _model(c["K"], c["sim"]).object_function(img, txt, labels=labels)
    assert loss.is_cuda and loss.dim() == 0 and loss.requires_grad
    (UPSTREAM * loss).backward()
    assert img.grad.shape == img.shape and txt.grad.shape == txt.shape and img.grad.dtype == torch.float32
    B = c["B"]
    return {"terms": _vec(loss, d), "g_img": img.grad.cpu().double().numpy().reshape(B, -1) / UPSTREAM,
            "g_txt": txt.grad.cpu().double().numpy().reshape(B, -1) / UPSTREAM}


def _compare(what, got, image, text, labels, K, sim):
    """prints e_ref, the yardstick, the port's error and their ratio per kind, then asserts e_port <= TOL_FACTOR * yardstick"""
    ref = DC.restate(image, text, labels, K, sim)
    e_ref = DC.errors(DC.restate(image, text, labels, K, sim, dtype=torch.float32), ref)
    yard, e = DC.yardstick(e_ref), DC.errors(got, ref)
    for k in DC.KINDS:
        print("%s %-5s e_ref %.2e  yardstick %.2e  e_port %.2e  e_port/e_ref %.2f  bound %.2e" %
              (what, k, e_ref[k], yard[k], e[k], e[k] / e_ref[k] if e_ref[k] else float("inf"), TOL_FACTOR * yard[k]))
    for k in DC.KINDS:
        assert np.isfinite(got[k]).all(), (what, k)
        assert e[k] <= TOL_FACTOR * yard[k], (what, k, e[k], yard[k])


# 1 routes against float64 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(DC.CASES))
def test_routes_against_float64(name):
    c = DC.build(name)
    img, txt = _device_inputs(c)
    labels = None if c["labels"] is None else c["labels"].cuda()
    got = _step(c, img, txt, labels)
    image, text = img.detach().cpu().reshape(c["B"], -1), txt.detach().cpu().reshape(c["B"], -1)
    print(name, DC.describe(DC.check_conditions(name, image, text)))       # the codes the device produced, before the comparison
    _compare(name, got, image, text, c["labels"], c["K"], c["sim"])


# 2 forward width limit ---------------------------------------------------------------------------------------------------------
def test_forward_width_limit():
    from xmh._lib import XmhError
    g = torch.Generator().manual_seed(DC.SEED + 2)
    B, K = 3, 6144
    labels = torch.tensor([[1.0, 0, 0], [1, 1, 0], [0, 0, 1]])
    c = dict(B=B, K=K, sim="euclidean", logits_i=torch.randn(B, K, 2, generator=g), logits_t=torch.randn(B, K, 2, generator=g))
    img, txt = _device_inputs(c)
    assert img.reshape(B, -1).shape[1] == 12288
    got = _step(c, img, txt, labels.cuda())
    _compare("D=12288", got, img.detach().cpu().reshape(B, -1), txt.detach().cpu().reshape(B, -1), labels, K, "euclidean")
    wide = torch.softmax(torch.randn(B, K + 1, 2, generator=g), -1).cuda()
    with pytest.raises(XmhError, match=r"\(-95\).*xmh_pair_similarity_loss: D=12290 > 12288"):
        _model(K + 1, "euclidean").object_function(wide, wide, labels=labels.cuda())


# 3 gradient LDS limit through the C entry --------------------------------------------------------------------------------------
def _limit_inputs(sim, g, B, D):
    if sim == "euclidean":
        a = torch.softmax(torch.randn(B, D // 2, 2, generator=g), -1).reshape(B, D)
        b = torch.softmax(torch.randn(B, D // 2, 2, generator=g), -1).reshape(B, D)
        return a, b
    b = torch.randn(B, D, generator=g)                           # a: mixtures of the rows of b, so that cosines spread over (0, 1)
    mix = torch.tensor([[1.0, 0.1, 0.6, 0.0], [0.3, 1.0, 0.0, 0.2], [0.0, 0.5, 1.0, 0.1], [0.15, 0.0, 0.25, 1.0]])
    return mix @ b + 0.4 * torch.randn(B, D, generator=g), b


@pytest.mark.parametrize("sim", ["euclidean", "cosine"])
def test_gradient_entry_at_the_lds_limit(sim):
    from xmh import retrieval as R
    from xmh._lib import current_stream, lib, ptr
    g = torch.Generator().manual_seed(DC.SEED + 3)
    B, D, C = 4, 16380, 3
    assert (B + D) * 4 == 65536
    K = D // 2
    a, b = _limit_inputs(sim, g, B, D)
    labels = torch.tensor([[1.0, 0, 0], [1, 1, 0], [0, 0, 1], [0, 1, 1]])
    if sim == "cosine":
        cs = DC.cosines(a, b)[0]
        gap = float(torch.minimum((cs - DC.THRESHOLD).abs(), (cs - (1 - DC.THRESHOLD)).abs()).min())
        inside = int(((cs > DC.THRESHOLD) & (cs < 1 - DC.THRESHOLD)).sum())
        print("lds limit cosine: gap %.3g, %d of 16 pairs inside the clamp" % (gap, inside))
        assert gap >= DC.GAP and 4 <= inside < 16
    m = _model(K, sim)
    cosine, max_value, threshold = m._branch()
    lab = R.pack_labels(labels.cuda())
    da, db = a.cuda(), b.cuda()
    grad = torch.full((B, D), 7.0, device="cuda")
    rc = lib.xmh_pair_similarity_loss_grad(ptr(da), ptr(db), B, D, ptr(lab), C, cosine, max_value, threshold, 1.0, None, ptr(grad), 0, current_stream())
    torch.cuda.synchronize()
    print("lds limit %s: rc %d %s" % (sim, rc, lib.xmh_last_error().decode() if rc else ""))
    assert rc == 0, lib.xmh_last_error()
    ref = DC.pair_grad(a, b, labels, K, sim)
    e_ref = DC.rel_err(DC.pair_grad(a, b, labels, K, sim, dtype=torch.float32), ref)
    pool = DC.golden_pool()
    yard, e = max(pool["g_img"], pool["g_txt"], e_ref), DC.rel_err(grad.cpu().numpy(), ref)
    print("lds limit %s: e_ref %.2e  yardstick %.2e  e_port %.2e  e_port/e_ref %.2f" % (sim, e_ref, yard, e, e / e_ref))
    assert np.abs(ref).max() > 0 and e <= TOL_FACTOR * yard, (sim, e, yard)
    # one element more: refused by the argument check, nothing launched
    wide = torch.zeros(B, D + 1, device="cuda")
    out = torch.full((B, D + 1), 7.0, device="cuda")
    rc = lib.xmh_pair_similarity_loss_grad(ptr(wide), ptr(wide), B, D + 1, ptr(lab), C, cosine, max_value, threshold, 1.0, None, ptr(out), 0,
                                           current_stream())
    assert rc == -95 and b"xmh_pair_similarity_loss_grad: (D + B) * 4 = 65540 bytes > 64 KB of LDS" in lib.xmh_last_error()
    assert bool((out == 7.0).all())


def test_the_python_pre_check_admits_what_the_entry_runs():
    """_Objective.forward repeats the entry's (B + D) * 4 <= 65536.  The forward's own width limit (D <= 12288) binds first for wide
    codes, so the bound is reached through the batch: B = 16382 rows of D = 2 run their backward, one row more is refused up front."""
    B, K = 16382, 1
    assert (B + 2 * K) * 4 == 65536
    g = torch.Generator().manual_seed(DC.SEED + 4)
    m = _model(K, "euclidean")
    labels = (torch.rand(B + 1, 2, generator=g) < 0.5).float().cuda()
    codes = torch.softmax(torch.randn(B + 1, K, 2, generator=g), -1).cuda()
    x = codes[:B].clone().requires_grad_(True)
    loss, _ = m.object_function(x, codes[:B], labels=labels[:B])
    loss.backward()
    print("B=16382: loss %.6f  max|grad| %.3e" % (float(loss.detach()), float(x.grad.abs().max())))
    assert bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 0
    with pytest.raises(ValueError, match="65536 bytes of LDS"):
        m.object_function(codes.clone().requires_grad_(True), codes, labels=labels)


# 4 non-finite parity -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(DC.NONFINITE))
def test_non_finite_inputs_give_the_nans_of_the_reference(name):
    image, text, labels, K, sim, nan_terms = DC.build_nonfinite(name)
    c = dict(B=image.shape[0], K=K, sim=sim)
    img, txt = image.cuda().requires_grad_(True), text.cuda().requires_grad_(True)
    got = _step(c, img, txt, labels.cuda())
    ref = DC.restate(image, text, labels, K, sim)
    r32 = DC.restate(image, text, labels, K, sim, dtype=torch.float32)
    want_nan = np.isnan(ref["terms"])
    assert {t for t, v in zip(DC.TERMS, want_nan) if v} == set(nan_terms)
    fin = ~want_nan
    e_ref, e = DC.rel_err(r32["terms"][fin], ref["terms"][fin]), DC.rel_err(got["terms"][fin], ref["terms"][fin])
    yard = max(DC.golden_pool()["terms"], e_ref)
    print("%s NaN terms: port %s  oracle %s" % (name, [t for t, v in zip(DC.TERMS, got["terms"]) if np.isnan(v)], sorted(nan_terms)))
    print("%s NaN gradient entries: image port %d oracle %d of %d, text port %d oracle %d" %
          (name, np.isnan(got["g_img"]).sum(), np.isnan(ref["g_img"]).sum(), ref["g_img"].size, np.isnan(got["g_txt"]).sum(),
           np.isnan(ref["g_txt"]).sum()))
    print("%s finite terms: e_ref %.2e  yardstick %.2e  e_port %.2e" % (name, e_ref, yard, e))
    assert np.array_equal(np.isnan(got["terms"]), want_nan) and not np.isinf(got["terms"]).any()
    for k in ("g_img", "g_txt"):
        assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k])) and np.isnan(ref[k]).all(), (name, k)
    assert e <= TOL_FACTOR * yard


# 5 reproducibility and flags ---------------------------------------------------------------------------------------------------
def test_backward_is_bit_reproducible_and_the_forward_to_1e14():
    from xmh import retrieval as R
    from xmh._lib import check, current_stream, lib, ptr
    c = DC.build("b300_k64_sat_copy_zero")
    runs = []
    for _ in range(2):
        img, txt = _device_inputs(c)
        _step(c, img, txt, c["labels"].cuda())
        runs.append((img.grad.clone(), txt.grad.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])   # no atomics in the gradient kernels
    image, text = (x.cuda() for x in DC.codes(c))
    lab = R.pack_labels(c["labels"].cuda())
    m = _model(c["K"], c["sim"])
    cosine, max_value, threshold = m._branch()
    outs = []
    for _ in range(2):
        out = torch.empty(2, dtype=torch.float64, device="cuda")
        check(lib.xmh_pair_similarity_loss(ptr(image), ptr(text), c["B"], image.shape[1], ptr(lab), c["C"], cosine, max_value, threshold, ptr(out),
                                           current_stream()), "loss")
        outs.append(out.cpu().numpy())
    print("forward doubles, two runs:", outs[0], outs[1], np.abs(outs[0] - outs[1]) / np.abs(outs[0]))
    assert (np.abs(outs[0] - outs[1]) <= 1e-14 * np.abs(outs[0])).all() and (outs[0] > 0).all()   # per-row doubles added with atomicAdd


def test_accumulate_scale_and_upstream_at_b300():
    from xmh import retrieval as R
    from xmh._lib import check, current_stream, lib, ptr
    c = DC.build("b300_k64_sat_copy_zero")
    image, text = (x.cuda() for x in DC.codes(c))
    B, D = image.shape
    lab = R.pack_labels(c["labels"].cuda())
    cosine, max_value, threshold = _model(c["K"], c["sim"])._branch()
    up = torch.tensor([0.5], device="cuda")
    g1, g2 = torch.empty(B, D, device="cuda"), torch.full((B, D), 7.0, device="cuda")
    args = (ptr(image), ptr(text), B, D, ptr(lab), c["C"], cosine, max_value, threshold)
    check(lib.xmh_pair_similarity_loss_grad(*args, 1.0, None, ptr(g1), 0, current_stream()), "grad")
    check(lib.xmh_pair_similarity_loss_grad(*args, 2.0, ptr(up), ptr(g2), 1, current_stream()), "grad")
    assert bool(g1.abs().max() > 0) and torch.equal(g2, 7.0 + g1)               # scale 2 x upstream 0.5 = 1, added to what was there
    q1, q2 = torch.empty(B, D, device="cuda"), torch.full((B, D), 7.0, device="cuda")
    check(lib.xmh_quant_loss_grad(ptr(image), image.numel(), 1.0, None, ptr(q1), 0, current_stream()), "qgrad")
    check(lib.xmh_quant_loss_grad(ptr(image), image.numel(), 2.0, ptr(up), ptr(q2), 1, current_stream()), "qgrad")
    assert torch.equal(q2, 7.0 + q1)


def test_one_sided_gradient_and_double_backward():
    c = DC.build("b300_k16_nolabels")
    image, text = (x.cuda() for x in DC.codes(c))
    m = _model(c["K"], c["sim"])
    a = image.clone().requires_grad_(True)
    loss, _ = m.object_function(a, text)
    loss.backward()
    assert a.grad is not None and text.grad is None
    b = text.clone().requires_grad_(True)
    loss2, _ = m.object_function(image, b)
    (ga,) = torch.autograd.grad(loss2, b, create_graph=True)
    assert float(loss2) == float(loss) and ga.shape == b.shape
    with pytest.raises(RuntimeError):
        ga.sum().backward()                                                      # the gradient kernels are not differentiable


# 6 no host synchronisation -----------------------------------------------------------------------------------------------------
def test_forward_and_backward_do_not_synchronise():
    c = DC.build("b257_k16_sat")
    m = _model(c["K"], c["sim"])
    labels = c["labels"].cuda()
    leaves = [c[k].cuda().requires_grad_(True) for k in ("logits_i", "logits_t")]

    def step():
        loss, d = m.object_function(torch.softmax(leaves[0], -1), torch.softmax(leaves[1], -1), labels=labels)
        (UPSTREAM * loss).backward()
        return loss, d

    step()                                                                       # warm-up: allocator, kernels loaded
    warm = [x.grad.clone() for x in leaves]
    for x in leaves:
        x.grad = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss, d = step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert np.isfinite(_vec(loss, d)).all()
    assert all(torch.equal(x.grad, w) for x, w in zip(leaves, warm))
