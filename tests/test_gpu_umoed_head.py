"""GPU: UMoED's soft-MoE decoder head (xmh_head_umoed, csrc/xmh_umoed.hip) through xmh.models.umoed against the float64
restatement of tests/umoed_cases.py:head and against the reference's recorded numbers (tests/golden/umoed.npz).

Rule: embeds within TOL_FACTOR = 4 times max(e_ref, pool): e = max|got - f64| / max|f64|, e_ref the float32 restatement's (for the golden
cases also the reference's own) e on the same inputs, pool the largest e_ref over HEAD_CASES.  The linear-subspace code is compared on
EVERY row: the inputs are drawn so that in float64 every row's two largest logits are at least 1e-3 of its largest |logit| apart.  Every
ratio is printed before the first assertion.  Cases (umoed_cases.HEAD_CASES): the golden shape; 3 x 5 slots with M = 64, T = 50, V = 16;
six layers at B = 37, F = 96; a slice of the workload (d = 512, 8 heads, 8 x 8 slots, F = 2048); the fusion call (5 + 4 tokens); the
plain decoder behind a first layer (E 192 -> 128) with tanh of the mean.

Measured on an MI355X, worst e / yardstick per case (the bound is 4): 0.49 (golden), 0.40 (3 x 5 slots), 0.89 (six layers), 0.49 (workload
slice), 0.46 (fusion), 1.05 (plain; its tanh code 0.84); against the reference's recorded numbers 0.44, 0.41 and 0.94.  No code bit differed."""
import numpy as np
import pytest
import torch

import umoed_cases as UC

pytestmark = pytest.mark.gpu


def _layer(c):
    """UMoEDHashLayer with fusion, its one TokenHash loaded strictly from the case's drawn parameters"""
    from xmh.models.umoed import UMoEDHashLayer
    layer = UMoEDHashLayer(visual_tokens=c.get("T_img", c["T"]), txt_tokens=c["T"] - c.get("T_img", c["T"]), img_feature_size=c["E"],
                           txt_feature_size=c["E"], outputDim=c["V"], setDim=c["M"], decoder_heads=c["heads"], decoder_layers=c["layers"],
                           num_experts=max(c["n"], 1), slots_per_expert=max(c["p"], 1), MoE=c["moe"], fusion=True, hidden_dim=c["d"],
                           hash_func_=c["hash_func"], merge_func_=UC.MERGE_OF[c["hash_func"]], dim_feedforward=c["F"])
    layer.hash_module.load_state_dict({k: torch.tensor(v) for k, v in c["P"].items()}, strict=True)
    return layer.cuda().eval().requires_grad_(False)


def _run(c, layer=None):
    layer = _layer(c) if layer is None else layer
    x = torch.tensor(c["x"]).cuda()
    with torch.no_grad():
        if "T_img" in c:
            embeds, code = layer.encode_imgAndtxt(x[:, :c["T_img"]], x[:, c["T_img"]:])
        else:
            embeds, code = layer.encode_img(x)
    torch.cuda.synchronize()
    assert tuple(embeds.shape) == (c["B"], c["M"], c["V"]) and embeds.dtype == torch.float32
    return {"embeds": embeds.cpu().double().numpy(), "code": code.cpu().double().numpy()}, layer


def _check(what, c, got, ref64, own):
    """embeds by the rule; the code bit for bit on every row (linear_subspace) or by the rule (tanh of the mean)"""
    if c["hash_func"] == "linear_subspace":
        worst = UC.compare(what, {"embeds": got["embeds"]}, ref64, own, UC.head_pool())
        assert got["code"].shape == ref64["code"].shape == (c["B"], c["M"] * int(np.log2(c["V"])))
        assert set(np.unique(got["code"])) <= {-1.0, 1.0}
        wrong = np.argwhere(got["code"] != ref64["code"])
        assert wrong.size == 0, (what, "code bits differ at", wrong[:8].tolist())
    else:
        worst = UC.compare(what, got, ref64, own, UC.head_pool())
    return worst


@pytest.mark.parametrize("name", list(UC.HEAD_CASES))
def test_head_against_float64_and_two_calls_to_the_bit(name):
    c = UC.head_case(name)
    got, layer = _run(c)
    r64, r32 = UC.head_reference(name), UC.head_reference(name, torch.float32)
    worst = _check(name, c, got, r64, {k: UC.rel_err(r32[k], r64[k]) for k in r64})
    print(name, "gap %.2e" % c["gap"], "worst ratio %.2f" % worst)
    again, _ = _run(c, layer)
    assert all(np.array_equal(got[k], again[k]) for k in got)                        # one fixed summation order


@pytest.mark.parametrize("name", list(UC.GOLDEN_HEAD_CASES))
def test_golden_cases_against_the_reference(name):
    """the reference's own recorded float64 numbers; the yardstick is its own float32-against-float64 deviation (or the largest recorded)"""
    G = np.load(UC.GOLDEN)
    c = UC.head_case(name)
    assert int(G["head__%s__seed" % name]) == c["seed"]
    g64 = {k: G["head__%s__f64_%s" % (name, k)] for k in ("embeds", "code")}
    g32 = {k: G["head__%s__f32_%s" % (name, k)] for k in ("embeds", "code")}
    got, _ = _run(c)
    own = {k: max(float(G["deviation__" + k]), UC.rel_err(g32[k], g64[k])) for k in g64}
    worst = _check(name + " (reference)", c, got, g64, own)
    print(name, "worst ratio against the reference %.2f" % worst)


def test_split_layer_runs_the_image_head_for_text_and_refuses_a_graph():
    """fusion: False keeps the reference's routing: encode_txt runs img_token_hash; and the head says that it has no backward"""
    from xmh.models.umoed import UMoEDHashLayer
    c = UC.head_case("golden")
    kw = dict(img_feature_size=c["E"], outputDim=c["V"], setDim=c["M"], decoder_heads=c["heads"], decoder_layers=c["layers"], num_experts=c["n"],
              slots_per_expert=c["p"], MoE=True, fusion=False, hidden_dim=c["d"], hash_func_="linear_subspace", merge_func_="concatenate")
    layer = UMoEDHashLayer(**kw)
    layer.img_token_hash.load_state_dict({k: torch.tensor(v) for k, v in c["P"].items()}, strict=True)
    layer = layer.cuda().eval()
    x = torch.tensor(c["x"]).cuda()
    with pytest.raises(NotImplementedError, match="backward of the decoder head"):
        layer.encode_img(x)
    with torch.no_grad():
        e_i, h_i = layer.encode_img(x)
        e_t, h_t = layer.encode_txt(x)
        with pytest.raises(AttributeError):
            layer.encode_imgAndtxt(x, x)
    assert torch.equal(e_i, e_t) and torch.equal(h_i, h_t)
    assert np.array_equal(h_i.cpu().double().numpy(), UC.head_reference("golden")["code"])
