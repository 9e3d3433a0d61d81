"""GPU: DIMCH's token-set head (xmh_head_dimch, xmh_head_dimch_train_forward, xmh_head_dimch_backward) against the float64
restatement of tests/dimch_cases.py:head.

Rule: per tensor e = max|got - f64| / max|f64| <= TOL_FACTOR = 4 times max(e_ref, pool), e_ref the float32 restatement's e on the same
inputs and pool the largest e_ref of that tensor over HEAD_CASES.  Every ratio is printed before the first assertion.  The inputs are
drawn so that no relu pre-activation lies within 64 eps of zero relative to the largest (dimch_cases.head_case), where a float32
evaluation may take the relu's other side.  Shapes: every T in {5, 50, 32}, E in {64, 512}, M in {1, 3, 8, 64}, K in {6, 16, 128},
B in {1, 2, 37}, with and without a keep mask, tanh and the pair softmax.

Measured on an MI355X, worst e / yardstick per case over the eleven tensors (the bound is 4): 0.86 (B = 1, M = 1), 0.60, 0.65
(B = 37, softmax), 1.01 (T = 50, E = 512, M = 8), 1.42 (g_x at T = 32, E = 512, M = 64, K = 128), 0.58; gradients through one output
alone 1.15 (g_b2 through hash); inference 0.77; a drawn mask 0.75; frozen parameters 0.34; the golden head case 0.76 (hash) against the
reference's recorded deviation."""
import numpy as np
import pytest
import torch

import dimch_cases as DC

pytestmark = pytest.mark.gpu


def _module(c, P=None):
    from xmh.models.dimch import DIMCHTokenHash
    m = DIMCHTokenHash(inputDim=c["T"], outputDim=c["K"], embedDim=c["E"], setDim=c["M"], dropout=c["p"], hash_func=c["hash_func"])
    P = c["P"] if P is None else P
    with torch.no_grad():
        for p, k in zip(m.head_params(), DC.HEAD_PARAMS):
            p.copy_(torch.tensor(P[k]))
    return m.cuda()


def _train(c, through="both", keep="case"):
    m = _module(c).train()
    x = torch.tensor(c["x"]).cuda().requires_grad_(True)
    keep = c["keep"] if keep == "case" else keep
    embeds, code = m(x, keep=None if keep is None else torch.tensor(keep))
    assert embeds.requires_grad and code.requires_grad and tuple(embeds.shape) == (c["B"], c["M"], c["K"]) and tuple(code.shape) == (c["B"], c["K"])
    tot = 0
    if through != "hash":
        tot = tot + (embeds * torch.tensor(c["g_embeds"]).cuda()).sum()
    if through != "embeds":
        tot = tot + (code * torch.tensor(c["g_hash"]).cuda()).sum()
    tot.backward()
    got = {"embeds": embeds, "hash": code, "g_x": x.grad}
    got.update({"g_" + k: p.grad for p, k in zip(m.head_params(), DC.HEAD_PARAMS)})
    return {k: v.detach().cpu().double().numpy() for k, v in got.items()}, m


@pytest.mark.parametrize("name", list(DC.HEAD_CASES))
def test_train_forward_and_backward_against_float64(name):
    c = DC.head_case(name)
    got, _ = _train(c)
    worst = DC.head_compare(name, got, DC.head_reference(name), DC.head_reference(name, torch.float32))
    print(name, "worst ratio %.2f" % worst)
    again, _ = _train(c)
    assert all(np.array_equal(got[k], again[k]) for k in got)                        # one fixed summation order: two calls agree to the bit


@pytest.mark.parametrize("name", ["b2_t5_e64_m3_k6_keep", "b37_t32_e64_m8_k6_keep"])
@pytest.mark.parametrize("through", ["embeds", "hash"])
def test_gradients_enter_through_one_output(name, through):
    c = DC.head_case(name)
    got, _ = _train(c, through)
    DC.head_compare("%s via %s" % (name, through), got, DC.head_reference(name, torch.float64, through), DC.head_reference(name, torch.float32, through))


@pytest.mark.parametrize("name", list(DC.HEAD_CASES))
def test_inference_against_float64_and_train_without_dropout_to_the_bit(name):
    c = DC.head_case(name)
    m = _module(c).eval()
    x = torch.tensor(c["x"]).cuda()
    embeds, code = m(x)
    assert not embeds.requires_grad and not code.requires_grad
    args = (c["x"], c["P"], None, 0.0, c["hash_func"])
    got = {"embeds": embeds.cpu().double().numpy(), "hash": code.cpu().double().numpy()}
    DC.head_compare(name + " eval", got, DC.head(*args, torch.float64), DC.head(*args, torch.float32))
    m.train()
    m.hash_layer[2].p = 0.0                                                          # p = 0: no mask is drawn
    assert m.draw_keep_mask(c["B"], x.device) is None
    te, tc = m(x.clone().requires_grad_(True))
    assert torch.equal(te.detach(), embeds) and torch.equal(tc.detach(), code)
    with torch.no_grad():
        ne, nc = m(x)                                                                # the train path with nothing kept
    assert torch.equal(ne, embeds) and torch.equal(nc, code)


def test_drawn_mask_is_seeded_and_applied():
    c = DC.head_case("b2_t50_e512_m8_k16_keep")
    m = _module(c).train()
    x = torch.tensor(c["x"]).cuda()
    outs = []
    for _ in range(2):
        m.generator = torch.Generator(device="cuda").manual_seed(77)
        with torch.no_grad():
            outs.append(m(x))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    m.generator = torch.Generator(device="cuda").manual_seed(77)
    keep = m.draw_keep_mask(c["B"], x.device)
    assert keep.dtype == torch.uint8 and tuple(keep.shape) == (c["B"] * c["M"], c["E"] // 2) and 0.6 < float(keep.float().mean()) < 0.8
    with torch.no_grad():
        replay = m(x, keep=keep.cpu())
    assert torch.equal(replay[0], outs[0][0])
    args = (c["x"], c["P"], keep.cpu().numpy(), c["p"], c["hash_func"])
    DC.head_compare("drawn mask", {"embeds": replay[0].cpu().double().numpy()}, DC.head(*args, torch.float64), DC.head(*args, torch.float32))


def test_frozen_parameters_get_no_gradient():
    c = DC.head_case("b2_t5_e64_m3_k6_keep")
    m = _module(c).train()
    m.token_layer.weight.requires_grad_(False)
    m.hash_layer[0].bias.requires_grad_(False)
    embeds, code = m(torch.tensor(c["x"]).cuda(), keep=torch.tensor(c["keep"]))
    ((embeds * torch.tensor(c["g_embeds"]).cuda()).sum() + (code * torch.tensor(c["g_hash"]).cuda()).sum()).backward()
    assert m.token_layer.weight.grad is None and m.hash_layer[0].bias.grad is None
    ref = DC.head_reference("b2_t5_e64_m3_k6_keep")
    got = {"g_" + k: p.grad.cpu().double().numpy() for p, k in zip(m.head_params(), DC.HEAD_PARAMS) if p.grad is not None}
    assert set(got) == {"g_conv_b", "g_w1", "g_w2", "g_b2"}
    DC.head_compare("frozen", got, ref, DC.head_reference("b2_t5_e64_m3_k6_keep", torch.float32))


def test_golden_head_case():
    """the reference's own recorded numbers (T = 5, E = 64, M = 3, K = 6, eval mode for the forward; the same numbers through the train
    path without a mask for the gradients), within 4 times its recorded float32-against-float64 deviation"""
    G = np.load(DC.GOLDEN)
    g = {k.split("__", 1)[1]: G[k] for k in G.files if k.startswith("head__")}
    dev = float(G["deviation__head"])
    c = dict(B=4, T=5, E=64, M=3, K=6, p=0.0, hash_func="tanh", P={k: g[k] for k in DC.HEAD_PARAMS}, keep=None, x=g["x"], g_embeds=g["g_embeds"],
             g_hash=g["g_hash"])
    got, m = _train(c)
    m.eval()
    e, h = m(torch.tensor(g["x"]).cuda())
    assert np.array_equal(e.cpu().double().numpy(), got["embeds"]) and np.array_equal(h.cpu().double().numpy(), got["hash"])
    rows = [(k, DC.rel_err(v, g["f64_" + k])) for k, v in got.items()]
    for k, err in rows:
        print("golden head %-9s e %.3e  deviation %.3e  ratio %.2f" % (k, err, dev, err / dev))
    assert all(err <= DC.TOL_FACTOR * dev for _, err in rows), rows


def test_shape_errors():
    c = DC.head_case("b2_t5_e64_m3_k6_keep")
    m = _module(c).eval()
    with pytest.raises(ValueError, match="tokens"):
        m(torch.zeros(2, 64, 5).cuda())                                              # [B, E, T]: tokens are always taken as [B, T, E]
