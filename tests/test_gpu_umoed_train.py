"""GPU: UMoED's decoder head in train mode and its backward (xmh_head_umoed_train_forward / xmh_head_umoed_backward,
csrc/xmh_umoed_grad.hip) through xmh.models.umoed against the float64 restatement of tests/umoed_train_cases.py and against
the reference's recorded numbers (tests/golden/umoed_train.npz).

Rule (umoed_cases.compare): embeds, the gradient of the tokens, of the learned rows, of all 19 parameters of every layer and of the
classifier within TOL_FACTOR = 4 times max(e_ref, pool): e = max|got - f64| / max|f64|, e_ref the float32 restatement's (for the golden
case the reference's own) e on the same inputs, pool the largest e_ref of that kind of tensor over the cases and settings.  Every ratio is
printed before the first assertion.  Cases (umoed_train_cases.TRAIN_CASES), each without dropout and with p = 0.3 masks drawn from the
case's seed: edge (B 3, T 7, M 5, one head, F 24, 2 x 2 slots, one layer), tiles (M 70, T 50, two heads, 3 x 5 slots, V 16, two layers),
rows (B 37, T 33, M 8, 2 x 3 slots, two layers: 296 and 111 reduction rows, weight gradients cut into 5, 13 and 2 chunks).

Bit-level: without a mask the train forward is the eval head's; two identical calls agree, forward and backward; a second backward with
``accumulate`` doubles every parameter gradient exactly (s + s is exact) and leaves d_tokens as written; gradients that are not asked for
are not formed and do not move the others by a bit.

Measured on an MI355X, worst e / yardstick (the bound is 4), without dropout / with p = 0.3: edge 1.06 / 0.92, tiles 0.82 / 0.96, rows 0.81 / 1.36;
against the reference's recorded numbers 0.70 / 1.62; with zeroed mask sections 1.02."""
import ctypes as C

import numpy as np
import pytest
import torch

import umoed_cases as UC
import umoed_train_cases as TC

pytestmark = pytest.mark.gpu


def _layer(c, **over):
    """UMoEDHashLayer with fusion in train mode, its one TokenHash loaded strictly from the case's drawn parameters"""
    from xmh.models.umoed import UMoEDHashLayer
    kw = dict(visual_tokens=c["T"], txt_tokens=0, img_feature_size=c["E"], txt_feature_size=c["E"], outputDim=c["V"], setDim=c["M"],
              dropout=TC.P_DROP, decoder_heads=c["heads"], decoder_layers=c["layers"], num_experts=c["n"], slots_per_expert=c["p"], MoE=True,
              fusion=True, hidden_dim=c["d"], hash_func_=c["hash_func"], merge_func_=UC.MERGE_OF[c["hash_func"]], dim_feedforward=c["F"])
    kw.update(over)
    layer = UMoEDHashLayer(**kw)
    layer.hash_module.load_state_dict({k: torch.tensor(v) for k, v in c["P"].items()}, strict=True)
    return layer.cuda().train()


def _keep(c, masks):
    return None if masks is None else torch.tensor(TC.flat_keep(masks)).cuda()


def _run(c, masks, layer=None, tokens_grad=True):
    """one train forward and backward of sum(embeds * G) -> ({"embeds", "g_tokens", "g_<name>"} float64 numpy, code, layer)"""
    layer = _layer(c) if layer is None else layer
    mod = layer.hash_module
    for q in mod.parameters():
        q.grad = None
    x = torch.tensor(c["x"]).cuda().requires_grad_(tokens_grad)
    embeds, code = layer.encode_img_train(x, keep=_keep(c, masks))
    assert tuple(embeds.shape) == (c["B"], c["M"], c["V"]) and embeds.requires_grad and not code.requires_grad
    (embeds * torch.tensor(c["G"]).cuda()).sum().backward()
    torch.cuda.synchronize()
    got = {"embeds": embeds.detach().cpu().double().numpy()}
    if tokens_grad:
        got["g_tokens"] = x.grad.cpu().double().numpy()
    for k, q in mod.named_parameters():
        if q.grad is not None:
            got["g_" + k] = q.grad.cpu().double().numpy()
    return got, code.detach(), layer


@pytest.mark.parametrize("which", TC.SETTINGS)
@pytest.mark.parametrize("name", list(TC.TRAIN_CASES))
def test_forward_and_every_gradient_against_float64_and_two_calls_to_the_bit(name, which):
    c = TC.case(name)
    masks, _ = TC.setting(c, which)
    got, code, layer = _run(c, masks)
    r64 = TC.reference(name, which)
    assert set(got) == set(r64) and len(got) == 3 + 19 * c["layers"] + 2
    worst = UC.compare("%s %s" % (name, which), got, r64, TC.own_errors(name, which), TC.pool_for(got))
    print(name, which, "worst ratio %.2f" % worst)
    again, code2, _ = _run(c, masks, layer)
    assert all(np.array_equal(got[k], again[k]) for k in got) and torch.equal(code, code2)       # one fixed summation order
    if masks is None:                                                                            # the eval head, to the bit
        x = torch.tensor(c["x"]).cuda()
        layer.eval()
        with torch.no_grad():
            e_eval, code_eval = layer.encode_img(x)
            e_ng, code_ng = layer.encode_img_train(x, keep=None)                                 # no record kept: the same forward
        layer.train()
        assert np.array_equal(e_eval.cpu().double().numpy(), got["embeds"]) and torch.equal(code_eval, code)
        assert torch.equal(e_ng, e_eval) and torch.equal(code_ng, code) and not e_ng.requires_grad
        assert np.array_equal(code.cpu().double().numpy(), UC.head(c["x"], c["P"], c, torch.float64)["code"])


@pytest.mark.parametrize("which", TC.SETTINGS)
def test_golden_case_against_the_reference(which):
    """the unmodified reference's recorded float64 numbers (masks replayed for p = 0.3); the yardstick is its own float32 deviation"""
    G = np.load(TC.GOLDEN)
    c = TC.case("golden")
    assert int(G["train__seed"]) == c["seed"]
    masks, _ = TC.setting(c, which)
    got, _, _ = _run(c, masks)
    vec, where = TC.golden_vector(got)
    g64, g32 = G["train__%s__f64" % which], G["train__%s__f32" % which].astype(np.float64)
    assert vec.shape == g64.shape
    pick = lambda v: {k: v[sl] for k, sl in where.items()}                                       # noqa: E731
    own = {k: UC.rel_err(g32[sl], g64[sl]) for k, sl in where.items()}
    worst = UC.compare("golden %s (reference)" % which, pick(vec), pick(g64), own, TC.pool_for(where))
    print("golden", which, "worst ratio against the reference %.2f" % worst)


def _c_backward(mod, x, keep, saved, up, grads, accumulate):
    from xmh import _lib
    from xmh._lib import check, current_stream, lib, ptr, workspace
    head, alive = mod._desc()
    B, T = x.shape[0], x.shape[1]
    wsb = C.c_size_t(0)
    lib.xmh_head_umoed_train_bytes(B, T, C.byref(head), C.byref(wsb))
    ws = workspace(wsb.value, x.device)
    at = lambda t: None if t is None else t.data_ptr()                                           # noqa: E731
    n = len(_lib.UmoedLayerGrads.NAMES)
    gp = grads["params"]
    layers = (_lib.UmoedLayerGrads * head.n_layers)(*[_lib.UmoedLayerGrads(*[at(t) for t in gp[1 + n * i:1 + n * (i + 1)]]) for i in range(head.n_layers)])
    g = _lib.UmoedHeadGrads(layers, at(gp[0]), at(gp[-2]), at(gp[-1]), at(grads["tokens"]))
    check(lib.xmh_head_umoed_backward(C.byref(head), ptr(x), ptr(keep), float(mod.dropout_p), ptr(up), B, T, ptr(saved), saved.numel(), C.byref(g),
                                      accumulate, ptr(ws), ws.numel(), current_stream()), "xmh_head_umoed_backward")
    torch.cuda.synchronize()


def test_accumulate_doubles_exactly_and_null_gradients_are_not_formed():
    c = TC.case("rows")                                                                          # split reductions: k_reduce_parts adds too
    layer = _layer(c)
    mod = layer.hash_module
    keep = _keep(c, c["masks"])
    x = torch.tensor(c["x"]).cuda()
    up = torch.tensor(c["G"]).cuda()
    with torch.no_grad():
        embeds, code, xk, saved = mod._run_train(x, keep)
    params = mod.head_params()
    full = {"params": [torch.full_like(q, float("nan")) for q in params], "tokens": torch.full_like(x, float("nan"))}
    _c_backward(mod, xk, keep, saved, up, full, 0)                                               # written over the NaNs
    once = [t.clone() for t in full["params"]], full["tokens"].clone()
    assert all(bool(torch.isfinite(t).all()) for t in once[0]) and bool(torch.isfinite(once[1]).all())
    _c_backward(mod, xk, keep, saved, up, full, 1)
    for q, a, b in zip(params, once[0], full["params"]):
        assert torch.equal(b, a + a), tuple(q.shape)                                             # s + s is exact in fp32
    assert torch.equal(full["tokens"], once[1])                                                  # d_tokens is written, never added to
    # only the classifier's weight and layer 1's phi asked for: the same bits, and nothing else is touched
    names = [k for k, _ in mod.named_parameters()]
    order = {id(q): i for i, q in enumerate(params)}
    idx = {k: order[id(q)] for k, q in mod.named_parameters()}
    some = {"params": [None] * len(params), "tokens": None}
    for k in ("classifier.weight", "decoder.layers.1.moe.phi"):
        some["params"][idx[k]] = torch.full_like(params[idx[k]], float("nan"))
    _c_backward(mod, xk, keep, saved, up, some, 0)
    for k in ("classifier.weight", "decoder.layers.1.moe.phi"):
        assert torch.equal(some["params"][idx[k]], once[0][idx[k]]), k
    assert len(names) == len(params) == 1 + 19 * c["layers"] + 2
    # through autograd: frozen parameters and tokens get no gradient, the others the same bits
    got_all, _, _ = _run(c, c["masks"], layer)
    frozen = ("decoder.layers.0.self_attn.in_proj_weight", "decoder.layers.1.moe.experts.weight", "decoder_learned_parameters", "classifier.bias")
    for k, q in mod.named_parameters():
        q.requires_grad_(k not in frozen)
    got, _, _ = _run(c, c["masks"], layer, tokens_grad=False)
    assert "g_tokens" not in got and not any("g_" + k in got for k in frozen) and len(got) == len(got_all) - 1 - len(frozen)
    assert all(np.array_equal(got[k], got_all[k]) for k in got)
    assert np.array_equal(got_all["g_tokens"], once[1].cpu().double().numpy())


def test_masks_that_zero_a_probability_row_and_a_whole_sublayer_output():
    c = TC.case("tiles")
    masks = [[m.copy() for m in layer] for layer in c["masks"]]
    masks[0][0][1, 1, 3, :] = 0                                                                  # drop1: a whole row of self-attention probabilities
    masks[1][2][0, 0, 69, :] = 0                                                                 # drop3: a whole row of cross-attention probabilities
    masks[1][5][:] = 0                                                                           # drop6 of layer 1: its Soft-MoE output is dropped
    r64, r32 = (TC.head_train(c["x"], c["P"], c, dt, c["G"], masks, TC.P_DROP) for dt in (torch.float64, torch.float32))
    got, _, _ = _run(c, masks)
    assert all(np.isfinite(v).all() for v in got.values())
    dead = ("moe.phi", "moe.experts.weight", "moe.experts.bias", "linear.weight", "linear.bias")
    for k in dead:                                                                               # exact zeros, in float64 and on the GPU
        assert not r64["g_decoder.layers.1." + k].any() and not got["g_decoder.layers.1." + k].any(), k
        assert got["g_decoder.layers.0." + k].any()
    worst = UC.compare("tiles, zeroed sections", got, r64, {k: UC.rel_err(r32[k], r64[k]) for k in r64}, TC.pool_for(got))
    print("zeroed sections: worst ratio %.2f" % worst)


def test_drawn_masks_follow_the_generator_and_the_refusals_are_named():
    from xmh._lib import XmhError
    c = TC.case("edge")
    layer = _layer(c)
    mod = layer.hash_module
    x = torch.tensor(c["x"]).cuda()
    outs = []
    for _ in range(2):
        mod.generator = torch.Generator(device="cuda").manual_seed(11)
        keep = mod.draw_keep_mask(c["B"], c["T"], x.device)
        mod.generator = torch.Generator(device="cuda").manual_seed(11)
        with torch.no_grad():
            outs.append((keep, layer.encode_img_train(x)[0]))
    assert outs[0][0].dtype == torch.uint8 and outs[0][0].is_cuda and outs[0][0].numel() == TC.flat_keep(c["masks"]).size
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]) and 0.6 < float(outs[0][0].float().mean()) < 0.8
    with torch.no_grad():
        assert torch.equal(layer.encode_img_train(x, keep=outs[0][0])[0], outs[0][1])            # the drawn mask, replayed
        assert not torch.equal(layer.encode_img_train(x, keep=None)[0], outs[0][1])
        assert torch.equal(layer.encode_txt_train(x, keep=None)[0], layer.encode_img_train(x, keep=None)[0])
    # the pinned refusals, in train mode and with a graph asked for
    with pytest.raises(NotImplementedError, match="backward of the decoder head"):
        layer.encode_img(x)
    with pytest.raises(NotImplementedError, match="backward of the decoder head"):
        layer.eval().encode_txt(x)
    layer.train()
    # the new ones
    with pytest.raises(ValueError, match="keep mask of 5 "):
        layer.encode_img_train(x, keep=torch.ones(5, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        layer.encode_img_train(x.cpu(), keep=None)
    mod.decoder.layers[0].norm1.eps = 1e-6
    with pytest.raises(XmhError, match="ln_eps"):
        layer.encode_img_train(x, keep=None)
    mod.decoder.layers[0].norm1.eps = 1e-5
    mod.first_layer = torch.nn.Linear(c["E"], c["d"]).cuda()
    with pytest.raises(NotImplementedError, match="first_layer"):
        layer.encode_img_train(x, keep=None)
    plain = dict(UC.head_case("plain"))
    from xmh.models.umoed import UMoEDTokenHash
    m = UMoEDTokenHash(outputDim=plain["V"], embedDim=plain["d"], setDim=plain["M"], decoder_heads=plain["heads"], decoder_layers=1, hash_func="tanh",
                       merge_func="mean", MoE=False, hidden_dim=plain["d"]).cuda()
    with pytest.raises(NotImplementedError, match="MoE: False"):
        m.forward_train(torch.zeros(2, 5, plain["d"]).cuda())
