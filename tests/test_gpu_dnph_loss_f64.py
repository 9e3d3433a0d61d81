"""GPU: xmh_dnph_loss / xmh_dnph_loss_grad (csrc/xmh_dnph.hip) against the float64 restatement of tests/dnph_cases.py where
tests/test_gpu_dnph_loss.py does not look (K <= 130, C <= 80 there): the column slots past the first (K = 257, 4096), second and
fourth trips of every class loop (C = 257, 1024; Cp = 300, 1024), label words 1, 2, 15, 16 and 31 with the lowest label at bit 0 and
bit 31, identity labels, the limits K = 4096, C = Cp = 1024 and B = 4096, 2B = 256 and 258, K = 1, rows and proxies clamped by
F.normalize's eps that are not zero, logits whose exp overflows float32, non-finite logits, codes and noise, and the autograd wrapper
with a frozen proxy table and with non-contiguous inputs.  Called through the C ABI with the helpers of tests/test_gpu_dnph_loss.py.

Rule (dnph_cases: edge_errors, edge_table).  Per tensor e = max|got - f64| / max|f64| <= TOL_FACTOR = 4 times max(pool, e_ref): pool
the largest float32-restatement error of that tensor kind over dnph_cases.CASES (unchanged by the cases here), e_ref the float32
restatement's e on the case's own inputs, both computed where the test runs.  Rows clamped by eps are a group of their own within
their gradient (key_clamped: they are about 1e10); at K = 1, where the gradient through F.normalize is an exact zero, each row's
error is divided by max(max|f64|, |du| / |v|), the size of the parts that cancel (dnph_cases.cancel_floor), for the float32
restatement as for the port.  The conditions that the inputs must meet for this to mean anything are asserted on the CPU by
tests/test_dnph_cases_cpu.py.  Every ratio is printed before the first assertion.

Measured on an MI355X, worst e / yardstick over the tensors of a case (the bound is 4): b5_k257_c33 0.91, b3_k4096_c5 0.35,
b9_k100_c1024 1.15, b6_k63_c257 0.54, b129_k65_c65 0.69, b128_k128_c80 0.88, b4096_k16_c2 0.42, b97_k16_c97_eye 0.39, b40_k1_c3 0.35,
b33_k64_c24_clamped 0.68 (the clamped groups: g_f_txt 0.20, g_P 0.31; largest gradient 5.8e10), b37_k48_c24_logits 0.73; the finite
parts of the six non-finite cases 0.71 at most (g_f_txt).

As first written, k_dnph_grad formed the prediction gradient's softmax as exp(p - lse) with lse = max + log(sum) a float: at
b37_k48_c24_logits (max|p| = 355) lse carries half an ulp of 355, 1.5e-5 of every softmax entry, and g_p_img / g_p_txt missed the
bound with ratios 30.2 and 32.2 (e 6.5e-6 and 7.0e-6 where e_ref is 7.8e-8 and 1.3e-7).  The kernel now divides exp(p - max) by the
sum, as torch's softmax does: 0.33 and 0.44 there, and b128_k128_c80 went from 1.70 to 0.88, b4096_k16_c2 from 1.31 to 0.42,
b97_k16_c97_eye from 1.17 to 0.39 (their worst tensor was a g_p each time).

The module was seen to fail under each of these edits of xmh_dnph.hip, one at a time on a scratch copy of the library (the first
failure of each, then what else):
  (a) the code-row branch of k_dnph_grad accumulates into acc[0] only: test_edge_cases_against_float64[b5_k257_c33], g_f_img e 4.7e-2;
      then b3_k4096_c5 (g_f_img 1.2e-3)
  (b) the same in the proxy branch: [b5_k257_c33], g_P e 0.58; then b3_k4096_c5 (g_P 2.1)
  (c) the loop that turns ds[c] into the weight takes one trip: [b9_k100_c1024], g_f not finite; then b6_k63_c257 (g_f_img e 12.4)
  (d) lowest_label without w * 32: [b5_k257_c33], loss e 1.3e-2 (d_loss_img 7.1e-3, g_p_img 1.0); then b9_k100_c1024, b6_k63_c257,
      b129_k65_c65 and b97_k16_c97_eye (loss 2.5e-2)
  (e) normalize_backward_store with s = vd * iv unconditionally: [b33_k64_c24_clamped], g_f_txt_clamped e 7.7e-3 and g_P_clamped
      7.7e-2 (ratios 9e3 and 1.3e5); nothing else, the zero rows included
  (f) the maximum replaced by 0 in the log-sum-exp: [b37_k48_c24_logits], d_loss_img and d_loss_txt inf, g_p NaN; then
      test_nonfinite_inputs_pass_through_as_recorded[posinf_logit] (the loss +inf where NaN is recorded)"""
import numpy as np
import pytest
import torch

import dnph_cases as DC
import test_gpu_dnph_loss as T       # its helpers (_dev, _call, _port) are shared, not copied; importing the module collects none of its tests

pytestmark = pytest.mark.gpu


# 1 the edge cases against float64 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(DC.EDGE_CASES))
def test_edge_cases_against_float64(name):
    c = DC.build_edge(name)
    r64, _, floor, own = DC.edge_reference(name)
    got = T._port(c)
    rows = DC.edge_table(name, DC.edge_errors(c, got, r64, floor), own)
    print(name, "worst ratio %.2f" % max(v / y for _, v, y in rows), " largest |gradient| %.3e" % max(np.abs(got[g]).max() for g in DC.GRADS))
    assert set(got) == set(r64) and all(got[k].shape == r64[k].shape for k in got)
    assert all(np.isfinite(v).all() for v in got.values())                           # the clamped rows too: about 1e10, not inf
    DC.assert_within(name, rows)


# 2 non-finite inputs -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(DC.NONFINITE))
def test_nonfinite_inputs_pass_through_as_recorded(name):
    c = DC.build_nonfinite(name)
    r64, r32 = DC.objective(c, torch.float64), DC.objective(c, torch.float32)
    got = T._port(c)
    want, seen = DC.recorded_classes(name), DC.classes(got)
    for k in want:
        print("%-24s %-10s not finite: port %d  recorded %d of %d" % (name, k, (seen[k] != 0).sum(), (want[k] != 0).sum(), want[k].size))
    rows = DC.edge_table(name, DC.finite_errors(got, r64), DC.finite_errors(r32, r64))
    assert all(np.array_equal(DC.classes(r64)[k], want[k]) for k in want)
    for k in want:                                                                   # entry for entry: NaN, +inf, -inf or finite
        assert np.array_equal(seen[k], want[k]), (name, k, seen[k].tolist(), want[k].tolist())
    for g in DC.GRADS:                                                               # a gradient row is NaN throughout or not at all
        bad = np.isnan(got[g])
        if name == "nan_noise" and g == "g_f_txt":
            assert int(bad.sum()) == 1 and bad[4, 2]
        else:
            assert np.array_equal(bad.any(1), bad.all(1)), (name, g)
    if name == "neginf_logit_off_target":
        assert got["g_p_img"][2, DC.nonfinite_target(c, 2)[1]] == 0                  # exp(-inf - lse): exactly 0
    DC.assert_within(name, rows)


# 3 two calls, and accumulate, at the slot and chunk edges ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["b129_k65_c65", "b5_k257_c33"])
def test_two_calls_bit_identical_and_accumulate_doubles(name):
    c = DC.build_edge(name)
    d = T._dev(c)
    out_a, ga = T._call(c, d)
    out_b, gb = T._call(c, d)
    assert np.isfinite(out_a).all() and all(bool((ga[g] != 3.0).any()) and bool(torch.isfinite(ga[g]).all()) for g in DC.GRADS)
    assert np.array_equal(out_a, out_b) and all(torch.equal(ga[g], gb[g]) for g in DC.GRADS)
    _, twice = T._call(c, d, accumulate=1, into={g: t.clone() for g, t in ga.items()})
    assert all(torch.equal(twice[g], 2 * ga[g]) for g in DC.GRADS)                   # x + x is exact: the same gradient was added


# 4 identity labels through the package -------------------------------------------------------------------------------------------------
def _loss_module(c, frozen=False):
    from xmh.models.dnph import DNPHLoss
    m = DNPHLoss(num_classes=c["C"], output_dim=c["K"], mrg=c["mrg"]).cuda()
    with torch.no_grad():
        m.proxies.copy_(torch.tensor(c["P"]))
    m.proxies.requires_grad_(not frozen)
    return m


def test_identity_labels_of_object_function_equal_the_c_abi():
    """DNPH.object_function without labels builds them as ones(B).diag(): C = B, the lowest label of row b is b"""
    from xmh.models.dnph import DNPH
    c = DC.build_edge("b97_k16_c97_eye")
    d = T._dev(c)
    out, raw = T._call(c, d)
    model = DNPH.__new__(DNPH)                                                       # object_function reads the loss module only
    torch.nn.Module.__init__(model)
    model.loss = _loss_module(c)
    built = {}
    model.compute_loss = lambda *a, **k: built.setdefault("labels", a[4])            # what object_function hands on
    leaves = [d[k].clone().requires_grad_(True) for k in T.INPUTS[:4]]
    model.object_function(*leaves)
    assert tuple(built["labels"].shape) == (97, 97) and not built["labels"].is_cuda
    terms = model.loss.terms(*leaves, built["labels"], built["labels"], noise_1=d["noise_img"], noise_2=d["noise_txt"], noise_alpha=c["alpha"])
    (terms[0] * c["up"]).backward()
    print("identity labels: loss %.6f (C ABI %.6f)" % (float(terms[0].detach()), out[0]))
    assert np.array_equal(terms.detach().cpu().numpy(), out[:6].astype(np.float32)) and np.isfinite(out).all()
    for g, t in zip(DC.GRADS, leaves + [model.loss.proxies]):
        assert torch.equal(t.grad, raw[g]), g


# 5 the autograd wrapper ----------------------------------------------------------------------------------------------------------------
def _through_wrapper(c, d, leaves, frozen=False):
    m = _loss_module(c, frozen)
    labels = torch.tensor(c["labels"])
    terms = m.terms(*leaves, labels, labels, noise_1=d["noise_img"], noise_2=d["noise_txt"], noise_alpha=c["alpha"])
    grads = torch.autograd.grad(terms[0] * c["up"], list(leaves) + ([] if frozen else [m.proxies]))
    return terms.detach(), list(grads), m


def test_wrapper_with_frozen_proxies_and_non_contiguous_inputs():
    c = DC.build_edge("b6_k63_c257")
    d = T._dev(c)
    out, raw = T._call(c, d)
    terms, grads, _ = _through_wrapper(c, d, [d[k].clone().requires_grad_(True) for k in T.INPUTS[:4]])
    assert np.array_equal(terms.cpu().numpy(), out[:6].astype(np.float32))
    assert all(torch.equal(g, raw[k]) for g, k in zip(grads, DC.GRADS))              # all five, as the C ABI gives them
    # the proxies frozen: needs_input_grad hands a NULL grad_P to the library
    leaves = [d[k].clone().requires_grad_(True) for k in T.INPUTS[:4]]
    m = _loss_module(c, frozen=True)
    labels = torch.tensor(c["labels"])
    t2 = m.terms(*leaves, labels, labels, noise_1=d["noise_img"], noise_2=d["noise_txt"], noise_alpha=c["alpha"])
    (t2[0] * c["up"]).backward()
    assert m.proxies.grad is None and torch.equal(t2.detach(), terms)
    assert all(torch.equal(t.grad, g) for t, g in zip(leaves, grads[:4]))
    # codes and logits as [:, ::2] views of tensors twice as wide
    views = []
    for k in T.INPUTS[:4]:
        wide = torch.full((d[k].shape[0], 2 * d[k].shape[1]), 9.0, device="cuda")
        wide[:, ::2] = d[k]
        views.append(wide.requires_grad_(True)[:, ::2])
    assert not any(v.is_contiguous() for v in views) and all(torch.equal(v, d[k]) for v, k in zip(views, T.INPUTS))
    t3, g3, _ = _through_wrapper(c, d, views)
    assert torch.equal(t3, terms)
    for v, g, want in zip(views + [None], g3, grads):
        assert (v is None or g.shape == v.shape) and torch.equal(g, want)
