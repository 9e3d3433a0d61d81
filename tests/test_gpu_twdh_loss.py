"""GPU: TwDH's training objective and its short-code transforms (xmh_twdh.hip behind torch.autograd in xmh/models/twdh.py, DESIGN
3.17) against the float64 restatement of tests/twdh_cases.py.

Targets are compared bit for bit.  Everything else by the project's rule: per tensor e = max|got - f64| / max|f64| must stay within
TOL_FACTOR = 4 times max(pool, e_ref), e_ref the float32 restatement's error on the same inputs and pool the largest e_ref of that
tensor kind over the cases (tests/test_gpu_tower_grad.py's rule and factor).  No entry is left out, and so that none hides behind
another's scale every scalar of the terms is a tensor of its own and every gradient is compared twice: whole (d_*: the saturated
entries, 0.5 / 1e-12 / n, set the scale) and with the saturated entries zeroed (ord_*: the ordinary entries at their own scale,
where the quantisation part is a few per cent of the largest entry).  Every ratio e / yardstick is printed before the first
assertion on a result.  Measured on an MI355X, worst e / yardstick per kind over the cases (the bound is 4): 3.34 for p_short and
1.68 for g_long, both at long 512 (a 1024-term product in another summation order than the CPU's); 1.00 for d_long (the float32
rounding of the saturated entries) and 0.48 for ord_long, 0.47 for d_short and 0.37 for ord_short; 0.46 for the total, 0.43 for
the BCE terms, 0.46 for the quantisation terms; composed through the transforms 0.82 for ord_long."""
import numpy as np
import pytest
import torch

import twdh_cases as TC

pytestmark = pytest.mark.gpu

SMALL = "synthetic:1814:vision_layers=1,transformer_layers=1,vision_width=128,transformer_width=128,embed_dim=64,image_resolution=64"
_models = {}


def _model(c):
    """a TwDH whose centres, transforms and weights are the case's (one module per set of code lengths)"""
    from xmh.models.twdh import TwDH
    lens = c["lens"]
    m = _models.get(lens)
    if m is None:
        m = _models[lens] = TwDH(cfg=None, long_dim=lens[0], clipPath=SMALL, trans="synthetic", short_dims=list(lens[1:]))
    keys, at = [str(k) for k in lens[1:]], 0
    m.trans = {}
    for k in lens[1:]:
        m.trans[str(k)] = torch.tensor(c["T"][:, at:at + 2 * k])
        at += 2 * k
    m.long_center = torch.tensor(c["centres"][0]).float()
    m.short_center = {k: torch.tensor(cen).float() for k, cen in zip(keys, c["centres"][1:])}
    m.quan_alpha, m.low_rate = c["quan_alpha"], c["low_rate"]
    return m


def _ties(c):
    return dict(zip(["long"] + [str(k) for k in c["lens"][1:]], (torch.tensor(t).float() for t in c["ties"])))


def _views(c, short):
    out, at = {}, 0
    for k in c["lens"][1:]:
        out[str(k)] = short[:, at:at + 2 * k]
        at += 2 * k
    return out


def _run(name, frozen=()):
    """one evaluation through the Python layer -> (got: numpy per tensor of TC.reference, the loss_dict, the targets)"""
    from xmh.models.twdh import _Objective
    c = TC.build(name)
    m = _model(c)
    leaves = {k: torch.tensor(c[k]).cuda().requires_grad_(k[:3] not in frozen) for k in ("img_long", "img_short", "txt_long", "txt_short")}
    ties = _ties(c)
    targets = m.hash_targets(c["labels"], torch.device("cuda", 0), ties)
    keys = list(m.trans)
    xs = [leaves["img_long"], leaves["txt_long"]] + [_views(c, leaves["img_short"])[k] for k in keys] + [_views(c, leaves["txt_short"])[k] for k in keys]
    out = _Objective.apply(m, targets, len(keys), *xs)
    (out[0] * c["up"]).backward()
    got = {"terms": out.detach().double().cpu().numpy()}
    for mod in ("img", "txt"):
        for which in ("long", "short"):
            g = leaves["%s_%s" % (mod, which)].grad
            got["d_%s_%s" % (which, mod)] = None if g is None else g.cpu().numpy()
    loss, d = m.object_function(leaves["img_long"].detach(), leaves["txt_long"].detach(), _views(c, leaves["img_short"].detach()),
                                _views(c, leaves["txt_short"].detach()), labels=c["labels"], ties=ties)
    long = torch.tensor(c["img_long"]).cuda().requires_grad_(True)
    p = m._short_train(long)
    p_all = torch.cat([p[k] for k in keys], 1)
    p_all.backward(torch.tensor(c["g_short"]).cuda())
    got["p_short"], got["g_long"] = p_all.detach().cpu().numpy(), long.grad.cpu().numpy()
    return got, (loss, d), targets


@pytest.mark.parametrize("name", list(TC.CASES))
def test_targets_are_bit_exact(name):
    c = TC.build(name)
    targets = _model(c).hash_targets(c["labels"], torch.device("cuda", 0), _ties(c))
    want = TC.pack_bits(c["bits"])
    assert targets.dtype == torch.int32 and tuple(targets.shape) == want.shape
    assert np.array_equal(targets.cpu().numpy().view(np.uint32), want)
    if c["B"] >= 3:
        s = c["labels"] @ np.concatenate(c["centres"], 1).astype(np.int64)
        ties = (s == 0) & (c["labels"].sum(1) > 0)[:, None]
        assert ties.any() and c["bits"][ties].any() and not c["bits"][ties].all(), "the case has no tie, or the ties all fall one way"
        assert c["labels"][0].sum() == 0 and not c["bits"][0].any() and c["labels"][1].all()


@pytest.mark.parametrize("name", list(TC.CASES))
def test_loss_gradients_and_transforms_against_float64(name):
    c = TC.build(name)
    frozen = ("txt",) if name == "b3_c33" else ()                                # one modality without requires_grad
    got, (loss, d), _ = _run(name, frozen)
    ref = TC.reference(name, torch.float64)
    n = len(c["lens"])
    zero_short = c["low_rate"] == 0                                              # an exact zero, skipped (None) or not
    check = {k: v for k, v in got.items() if not (k[-3:] in frozen and k.startswith("d_")) and not (zero_short and k.startswith("d_short"))}
    expanded = TC.expand(name, check)
    worst = TC.compare(name, expanded, ref)                                      # prints every ratio, then asserts
    print(name, "worst ratio %.2f" % worst)
    assert set(expanded) == {k for k in ref if not (k[-3:] in frozen and k[:2] in ("d_", "or")) and not (zero_short and "_short_" in k)}
    for mod in ("img", "txt"):
        for which in ("long", "short"):
            key = "d_%s_%s" % (which, mod)
            if mod in frozen:
                assert got[key] is None, key
            elif which == "short" and zero_short:
                assert not ref[key].any() and (got[key] is None or not got[key].any()), key
    # the saturated pairs of the case sit on and off target: the -100 clamp and the 1e-12 floor are both hit
    row = 2 if c["B"] >= 3 else 0
    for mat in ("img_long", "txt_short"):
        assert set(c[mat][row, :8].tolist()) == {0.0, 1.0} and TC.saturated(c[mat]).sum() == 8 * (1 if mat == "img_long" else n - 1)
    b0, b1 = int(c["bits"][row, 0]), int(c["bits"][row, 1])
    assert c["img_long"][row, b0] == 1.0 and c["img_long"][row, 2 + b1] == 0.0    # pair 0 on target, pair 1 off target
    assert abs(ref["d_long_img"][row, 2 + b1]) == pytest.approx(c["up"] * (0.5 / 1e-12 - 2 * c["quan_alpha"]) / c["img_long"].size, rel=1e-9)
    # the dictionary the reference's keys name: detached slices of the same vector
    t = torch.tensor(got["terms"]).float()
    assert not loss.requires_grad and float(loss) == float(t[0]) == float(d["All loss"])
    assert [float(d["Long"]["NCE"]["image"]), float(d["Long"]["Quan"]["image"]), float(d["Long"]["NCE"]["text"]), float(d["Long"]["Quan"]["text"])] == \
        [float(t[1]), float(t[2]), float(t[1 + 2 * n]), float(t[2 + 2 * n])]
    assert list(d["Short"]) == [str(k) for k in c["lens"][1:]]
    for i, k in enumerate(d["Short"]):
        assert float(d["Short"][k]["NCE"]) == float(t[1 + 4 * n + 2 * (i + 1)]) and float(d["Short"][k]["Quan"]) == float(t[2 + 4 * n + 2 * (i + 1)])
    assert all(not v.requires_grad for v in (d["All loss"], d["Long"]["NCE"]["image"]))
    assert (got["p_short"][:, :4] == (1, 0, 0, 1)).all()                         # logits 160 apart: exact 0 / 1 out of the pair softmax


def test_saturated_short_codes_from_the_transforms_into_the_objective():
    """probabilities exactly 0 and 1 out of the pair softmax (logits 160 apart), on and off target, through loss and backward"""
    name = "b65_c80"
    c = TC.build(name)
    m = _model(c)
    first = c["lens"][0]                                                         # pair 0 of the first short length comes out (1, 0)
    assert set(c["bits"][1:, first].tolist()) == {0, 1} and set(c["bits"][1:, first + 1].tolist()) == {0, 1}
    leaves = {mod: torch.tensor(c[mod + "_long"]).cuda().requires_grad_(True) for mod in ("img", "txt")}
    shorts = {mod: m._short_train(leaves[mod]) for mod in leaves}
    assert all((shorts[mod][str(c["lens"][1])][:, :4] == torch.tensor([1.0, 0.0, 0.0, 1.0]).cuda()).all() for mod in shorts)
    loss, d = m.object_function(leaves["img"], leaves["txt"], shorts["img"], shorts["txt"], labels=c["labels"], ties=_ties(c))
    (loss * c["up"]).backward()
    ref, r32 = TC.composed(name, torch.float64), TC.composed(name, torch.float32)
    n = len(c["lens"])
    known = [0, 1, 2, 1 + 2 * n, 2 + 2 * n] + [i + 4 * n + 2 * s for s in range(1, n) for i in (1, 2)]      # what loss_dict names
    flat = [d["All loss"], d["Long"]["NCE"]["image"], d["Long"]["Quan"]["image"], d["Long"]["NCE"]["text"], d["Long"]["Quan"]["text"]] + \
        [d["Short"][k][t] for k in d["Short"] for t in ("NCE", "Quan")]
    got = TC.expand(name, {"d_long_img": leaves["img"].grad.cpu().numpy(), "d_long_txt": leaves["txt"].grad.cpu().numpy()})
    got.update({TC.term_key(i): np.array([float(v)]) for i, v in zip(known, flat)})
    TC.compare(name + " composed", got, ref, {k: TC.rel_err(r32[k], ref[k]) for k in ref})
    assert set(got) == {"d_long_img", "d_long_txt", "ord_long_img", "ord_long_txt"} | {TC.term_key(i) for i in known}
    assert ref[TC.term_key(1 + 4 * n + 2)][0] > 100 * 0.25 / c["lens"][1]           # off-target saturated pairs: the -100 clamp is in the mean
    # the way through the transforms is a visible share of the ordinary entries of d long
    direct = TC.loss_grad(c["img_long"], TC.short_forward(c["img_long"], c["T"]), c["bits"], c["lens"], c["quan_alpha"], c["low_rate"], c["up"])[0]
    assert TC.rel_err(TC.expand(name, {"d_long_img": direct.numpy()})["ord_long_img"], ref["ord_long_img"]) > 1e-3


def test_short_backward_accumulates_into_g_long():
    """xmh_twdh_short_backward with accumulate != 0: g_long += g_z . T_cat^T (the product's residual operand is its own output)"""
    from xmh import _lib
    from xmh._lib import check, current_stream, lib, ptr
    name = "b65_c80"
    c = TC.build(name)
    const = _model(c)._constants(torch.device("cuda", 0))
    B, L2, S2 = c["B"], 2 * c["lens"][0], c["T"].shape[1]
    long = torch.tensor(c["img_long"]).cuda()
    p = torch.empty(B, S2, dtype=torch.float32, device="cuda")
    check(lib.xmh_twdh_short_forward(ptr(long), ptr(const["trans_t"]), B, L2, S2, ptr(p), current_stream()), "xmh_twdh_short_forward")
    g = torch.tensor(c["g_short"]).cuda()
    before = torch.tensor(np.random.default_rng(7).standard_normal((B, L2)).astype(np.float32)).cuda()
    outs = []
    for accumulate in (0, 1):
        gl = before.clone()
        ws = _lib.workspace(B * S2 * 4, gl.device)
        check(lib.xmh_twdh_short_backward(ptr(g), ptr(p), ptr(const["trans"]), B, L2, S2, ptr(gl), accumulate, ptr(ws), ws.numel(), current_stream()),
              "xmh_twdh_short_backward")
        outs.append(gl)
    ref = TC.reference(name, torch.float64)
    want = before.double().cpu().numpy() + ref["g_long"]
    e, e0 = TC.rel_err(outs[1].cpu().numpy(), want), TC.rel_err(outs[0].cpu().numpy(), ref["g_long"])
    yard = max(TC.pool()["g_long"], TC.e_ref(name)["g_long"])
    print("accumulate: e %.3e, written: e %.3e, yardstick %.3e, ratios %.2f %.2f" % (e, e0, yard, e / yard, e0 / yard))
    assert e <= TC.TOL_FACTOR * yard and e0 <= TC.TOL_FACTOR * yard
    assert torch.equal(outs[1], outs[0] + before)                                # one rounding of the sum, in the product's epilogue


def test_soft_argmax_hash_loss_is_differentiable():
    c = TC.build("b65_c80")
    m = _model(c)
    code = torch.tensor(c["img_long"]).cuda().requires_grad_(True)
    q = m.soft_argmax_hash_loss(code)
    (q * 1.7).backward()
    p64 = torch.tensor(c["img_long"]).double()
    want, want_g = float(1 - ((2 * p64 - 1) ** 2).mean()), (1.7 * -4 * (2 * p64 - 1) / p64.numel()).numpy()
    g32 = (1.7 * -4 * (2 * p64.float() - 1) / p64.numel()).numpy()
    e, e_ref = TC.rel_err(code.grad.cpu().numpy(), want_g), TC.rel_err(g32, want_g)
    print("soft_argmax_hash_loss: value %.9f / %.9f, gradient e %.3e e_ref %.3e" % (float(q.detach()), want, e, e_ref))
    assert float(q) == pytest.approx(want, rel=4 * 2.0 ** -23) and e <= TC.TOL_FACTOR * max(e_ref, 2.0 ** -24)
    with torch.no_grad():
        assert not m.soft_argmax_hash_loss(code).requires_grad


def test_two_evaluations_agree_to_the_bit():
    a, _, ta = _run("b130_c80")
    b, _, tb = _run("b130_c80")
    assert torch.equal(ta, tb)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_a_nan_probability_passes_through():
    from xmh.models.twdh import _Objective
    c = TC.build("b65_c80")
    m = _model(c)
    p = {k: torch.tensor(c[k]).cuda() for k in ("img_long", "img_short", "txt_long", "txt_short")}
    p["img_long"][7, 10:12] = float("nan")
    leaves = {k: v.requires_grad_(True) for k, v in p.items()}
    targets = m.hash_targets(c["labels"], torch.device("cuda", 0), _ties(c))
    keys = list(m.trans)
    xs = [leaves["img_long"], leaves["txt_long"]] + [_views(c, leaves["img_short"])[k] for k in keys] + [_views(c, leaves["txt_short"])[k] for k in keys]
    out = _Objective.apply(m, targets, len(keys), *xs)
    out[0].backward()
    torch.cuda.synchronize()
    n = len(c["lens"])
    t = out.detach().cpu().numpy()
    nan = np.isnan(t)
    assert nan[0] and nan[1] and nan[2] and nan[1 + 4 * n] and nan[2 + 4 * n] and nan.sum() == 5, t      # the image's long terms, their means, the total
    g = leaves["img_long"].grad.cpu().numpy()
    assert np.isnan(g[7, 10:12]).all() and np.isnan(g).sum() == 2
    for k in ("img_short", "txt_long", "txt_short"):
        assert np.isfinite(leaves[k].grad.cpu().numpy()).all(), k


def test_what_the_python_layer_refuses_on_the_device():
    c = TC.build("b3_c33")
    m = _model(c)
    li, lt = torch.tensor(c["img_long"]).cuda(), torch.tensor(c["txt_long"]).cuda()
    si, st = _views(c, torch.tensor(c["img_short"]).cuda()), _views(c, torch.tensor(c["txt_short"]).cuda())
    with pytest.raises(ValueError, match="label rows"):
        m.object_function(li, lt, si, st, labels=c["labels"][:2])
    with pytest.raises(ValueError, match="hash centres of 33 classes"):
        m.object_function(li, lt, si, st, labels=np.ones((3, 34), np.int64))
    with pytest.raises(ValueError, match="short codes"):
        m.object_function(li, lt, {"4": si["4"]}, st, labels=c["labels"])
    with pytest.raises(ValueError, match="is expected"):
        m.object_function(li[:, :-2], lt, si, st, labels=c["labels"])
    # without labels every sample is its own class (reference :186-190), and the draw comes from the CPU's global generator
    torch.manual_seed(11)
    a, _ = m.object_function(li, lt, si, st)
    torch.manual_seed(11)
    want = m.draw_ties()
    b, _ = m.object_function(li, lt, si, st, labels=np.eye(3, dtype=np.int64), ties=want)
    assert float(a) == float(b)
    q = m.soft_argmax_hash_loss(li)
    assert float(q) == pytest.approx(float(1 - ((2 * torch.tensor(c["img_long"]).double() - 1) ** 2).mean()), rel=1e-6)
