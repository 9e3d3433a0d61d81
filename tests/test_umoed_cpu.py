"""UMoED without a GPU: the float64 restatements of tests/umoed_cases.py against the numbers the unmodified reference
recorded in tests/golden/umoed.npz (tools/make_golden_umoed.py) -- 1e-12 relative in float64, within the recorded
float32-against-float64 deviation in float32; the guards the GPU tests rely on; the module's state dict against the reference's record;
the bit order of the linear-subspace code; the registry, the configuration defaults, the C entry points' argument errors and bounds, and
what is refused with the key named."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import umoed_cases as UC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = "synthetic:1814:vision_layers=1,transformer_layers=1,vision_width=128,transformer_width=128,embed_dim=64,image_resolution=64"
NEW = ("xmh_head_umoed_bytes", "xmh_head_umoed", "xmh_umoed_loss_ws_bytes", "xmh_umoed_loss", "xmh_umoed_loss_grad")
# configs/UMoED/config.yaml of the reference, the model block
CONFIG_YAML = {"arch": "UMoED", "setDim": 64, "dropout": 0.3, "extreme": True, "extreme_T": 0.3, "triplet": True, "distance_mode": "cosine",
               "MoE": True, "fusion": True, "num_experts": 8, "slots_per_expert": 8, "hash_func": "linear_subspace", "merge_func": "concatenate",
               "decoder_heads": 8, "decoder_layers": 6, "hidden_dim": 512,
               "distance": {"mode": "pairwise", "denominator": 2.0, "temperature": 16.0, "temperature_txt_scale": 1.0},
               "chamfer": {"unif_alpha": 0.8, "token_triplet_margin": 0.1}, "hash_pars": {"triplet_alpha": 1, "triplet_margin": 0.3}}


# ---- the restatements against the reference's recorded numbers ------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(UC.GOLDEN_HEAD_CASES))
def test_head_restatement_reproduces_the_reference(name):
    G = np.load(UC.GOLDEN)
    c = UC.head_case(name)
    assert int(G["head__%s__seed" % name]) == c["seed"]                              # the same draw as the generator's
    r64, r32 = UC.head_reference(name), UC.head_reference(name, torch.float32)
    for k in ("embeds", "code"):
        g64, g32 = G["head__%s__f64_%s" % (name, k)], G["head__%s__f32_%s" % (name, k)]
        e64, e32 = UC.rel_err(r64[k], g64), UC.rel_err(r32[k], g64)
        dev = max(float(G["deviation__" + k]), UC.rel_err(g32, g64))
        print(name, k, "f64 %.2e" % e64, "f32 %.2e" % e32, "recorded deviation %.2e" % dev)
        assert r64[k].shape == g64.shape and e64 <= 1e-12, (name, k, e64)
        if k == "code" and c["hash_func"] == "linear_subspace":
            assert np.array_equal(r32[k], g64) and np.array_equal(g32, g64)
        else:
            assert 0 < dev < 1e-5 and e32 <= UC.TOL_FACTOR * dev, (name, k, e32, dev)
    # a decoder that attends to the tokens in place of the learned rows in its self-attention block is far outside
    swapped = dict(c["P"])
    k0, k1 = "decoder.layers.0.self_attn.in_proj_weight", "decoder.layers.0.multihead_attn.in_proj_weight"
    swapped[k0], swapped[k1] = c["P"][k1], c["P"][k0]
    assert UC.rel_err(UC.head(c["x"], swapped, c, torch.float64)["embeds"], G["head__%s__f64_embeds" % name]) > 1e-3


@pytest.mark.parametrize("name", list(UC.GOLDEN_LOSS_CASES))
def test_objective_restatement_reproduces_the_reference(name):
    G = np.load(UC.GOLDEN)
    c = dict(UC.draw_loss(**UC.GOLDEN_LOSS_CASES[name]), up=1.0)
    assert int(G["loss__%s__seed" % name]) == c["seed"]
    r64, r32 = UC.objective(c, torch.float64), UC.objective(c, torch.float32)
    for k in UC.TERMS + UC.GRADS:
        g64, g32 = G["loss__%s__f64_%s" % (name, k)], G["loss__%s__f32_%s" % (name, k)]
        dev = max(float(G["deviation__" + UC.kind_of(k)]), UC.rel_err(g32, g64))
        assert r64[k].shape == g64.shape and UC.rel_err(r64[k], g64) <= 1e-12, (name, k, UC.rel_err(r64[k], g64))
        assert UC.rel_err(r32[k], g64) <= UC.TOL_FACTOR * dev, (name, k, UC.rel_err(r32[k], g64), dev)
    assert r64["T_i2t"][0] > 0 and r64["T_t2i"][0] > 0
    wrong = UC.objective(c, torch.float64, token_triplet_margin=UC.consts(c)["token_triplet_margin"] * 1.5)
    assert UC.rel_err(wrong["loss"], G["loss__%s__f64_loss" % name]) > 1e-3           # a wrong margin is far outside


# ---- the guards the GPU tests rely on -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(UC.HEAD_CASES))
def test_head_cases_are_guarded(name):
    c = UC.head_case(name)
    r = UC.head_reference(name)
    bits = int(np.log2(c["V"]))
    print(name, "seed", c["seed"], "gap", c["gap"])
    assert r["embeds"].shape == (c["B"], c["M"], c["V"]) and np.isfinite(r["embeds"]).all()
    if c["hash_func"] == "linear_subspace":
        assert UC.head_gap(r["embeds"]) == c["gap"] >= UC.HEAD_GAP                   # every row: no bit is left out of the comparison
        assert r["code"].shape == (c["B"], c["M"] * bits) and set(np.unique(r["code"])) <= {-1.0, 1.0}
        if c["V"] == 2:
            assert np.array_equal(r["code"] > 0, r["embeds"][..., 1] > r["embeds"][..., 0])
    else:
        assert r["code"].shape == (c["B"], c["V"]) and np.abs(r["code"]).max() < 1


def test_head_cases_cover_the_table():
    H = UC.HEAD_CASES
    assert [(c["B"], c["T"], c["d"], c["heads"], c["M"], c["layers"], c["n"], c["p"], c["F"], c["V"]) for c in H.values()] == [
        (2, 5, 128, 2, 3, 2, 2, 2, 2048, 2), (1, 50, 128, 2, 64, 1, 3, 5, 2048, 16), (37, 32, 128, 2, 8, 6, 8, 8, 96, 2),
        (2, 50, 512, 8, 64, 2, 8, 8, 2048, 2), (2, 9, 128, 2, 3, 2, 2, 2, 2048, 2), (2, 5, 128, 2, 3, 2, 0, 0, 2048, 16)]
    assert H["plain"]["E"] == 192 and not H["plain"]["moe"] and H["plain"]["hash_func"] == "tanh" and H["fusion"]["T_img"] == 5


@pytest.mark.parametrize("name", list(UC.LOSS_CASES))
def test_loss_cases_are_guarded_and_live(name):
    c = UC.loss_case(name)
    probe = UC.guards(c)
    print(name, "seed", c["seed"], probe)
    assert UC.guarded(probe) and probe["clamp"] >= 1e-5 and probe.get("hinge", 1.0) >= 1e-5
    r = UC.loss_reference(name)
    assert all(np.isfinite(v).all() for v in r.values())
    if c["C"] > 1:
        assert r["T_i2t"][0] > 0 and r["T_t2i"][0] > 0 and (c["labels"] @ c["labels"].T == 0).any()      # some pairs share no class
    else:
        assert r["T_i2t"][0] == 0 and "hinge" not in probe
    assert (r["U_img"][0] == 0) == (c["M"] == 1)
    if c["same_set"]:
        x = torch.nn.functional.normalize(torch.tensor(c["e_img"], dtype=torch.float64), dim=-1)
        D = (1 - torch.einsum("btl,ktl->btk", x, x).clamp(min=0)).mean(1)
        assert abs(float(D[UC.SAME_ROW, UC.SAME_ROW])) < 1e-15 and np.array_equal(c["e_img"][UC.SAME_ROW, 0], c["e_img"][UC.SAME_ROW, 1])


def test_a_row_without_a_label_gives_nan():
    c = dict(UC.loss_case("b7_m5_v2_extreme"))
    c["labels"] = c["labels"].copy()
    c["labels"][0] = 0
    r = UC.objective(c, torch.float64)
    assert np.isnan(r["loss"][0]) and np.isnan(r["T_i2t"][0]) and np.isfinite(r["U_img"][0])


# ---- the bit order of the linear-subspace code ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [2, 4, 16])
def test_linear_subspace_bit_order(V):
    from xmh.models.umoed import linear_subspace_code
    bits = int(np.log2(V))
    logits = torch.full((1, V, V), -1.0)
    logits[0, torch.arange(V), torch.arange(V)] = 1.0            # row m has its maximum at index m
    want = np.array([[1.0 if (m >> (bits - 1 - j)) & 1 else -1.0 for j in range(bits)] for m in range(V)]).reshape(1, V * bits)
    assert np.array_equal(UC.linear_subspace_bits(logits.double()).numpy(), want)
    assert np.array_equal(linear_subspace_code(logits).numpy(), want)
    if V == 4:
        assert want.tolist() == [[-1, -1, -1, 1, 1, -1, 1, 1]]                       # 0 -> 00, 1 -> 01, 2 -> 10, 3 -> 11, most significant first
    tie = torch.zeros(1, 1, V)
    assert np.array_equal(linear_subspace_code(tie).numpy(), -np.ones((1, bits)))    # a tie goes to the first index


# ---- the module tree ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", list(UC.STATE_CONFIGS))
def test_state_dict_is_the_reference_s_and_loads_strictly(cfg):
    from xmh.models.umoed import UMoEDHashLayer
    G = np.load(UC.GOLDEN)
    rec = sorted(k for k in G.files if k.startswith("state__%s__" % cfg))
    want = [(k.split("__", 3)[3], tuple(int(n) for n in G[k])) for k in rec]
    layer = UMoEDHashLayer(**UC.STATE_CONFIGS[cfg])
    assert [(k, tuple(v.shape)) for k, v in layer.state_dict().items()] == want      # names, shapes and the reference's order
    first = "hash_module." if cfg == "moe_fusion" else "img_token_hash."
    assert want[0][0] == first + "decoder_learned_parameters"
    if cfg == "moe_fusion":
        names = dict(want)
        assert names["hash_module.decoder.layers.1.moe.phi"] == (2048, 8, 8) and names["hash_module.decoder.layers.0.moe.experts.weight"] == (8, 2048, 512)
        assert names["hash_module.decoder.layers.0.multihead_attn.out_proj.bias"] == (512,) and names["hash_module.classifier.weight"] == (2, 512)
    else:
        assert dict(want)["txt_token_hash.first_layer.weight"] == (256, 512)
    g = torch.Generator().manual_seed(1)
    sd = {k: torch.randn(shape, generator=g) for k, shape in want}
    assert layer.load_state_dict(sd, strict=True).missing_keys == []
    key = want[-1][0]
    assert torch.equal(layer.state_dict()[key], sd[key])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        with torch.no_grad():
            layer.eval().encode_img(torch.zeros(2, 50, 512))


def test_initial_weights_come_from_a_private_generator():
    from xmh.models.umoed import UMoEDTokenHash
    kw = dict(outputDim=2, embedDim=128, setDim=4, decoder_heads=2, decoder_layers=2, num_experts=2, slots_per_expert=2, MoE=True, hidden_dim=128,
              dim_feedforward=64)
    a = UMoEDTokenHash(seed=3, **kw)
    torch.manual_seed(5)
    b = UMoEDTokenHash(seed=3, **kw)
    assert all(torch.equal(p, q) for p, q in zip(a.state_dict().values(), b.state_dict().values()))
    assert not torch.equal(a.classifier.weight, UMoEDTokenHash(seed=4, **kw).classifier.weight)
    y0, y1 = a.decoder.layers
    assert torch.equal(y0.moe.phi, y1.moe.phi)                                       # the reference deep-copies one layer
    assert float(y0.self_attn.in_proj_bias.abs().max()) == 0 and float(y0.norm1.weight.min()) == 1
    assert float(y0.moe.phi.abs().max()) <= 0.5 and float(y0.moe.experts.weight.abs().max()) <= (64 * 128) ** -0.5
    assert float(y0.self_attn.in_proj_weight.abs().max()) <= (6.0 / (128 + 384)) ** 0.5
    assert a.code_width == 4 and UMoEDTokenHash(**dict(kw, outputDim=16)).code_width == 16


def test_registry_resolves_umoed():
    import xmh.models  # noqa: F401
    import xmh.runners  # noqa: F401
    from xmh.common.register import registry
    from xmh.models.umoed import UMoED
    from xmh.runners.methods import UMoEDTrainer
    assert registry.get_model_class("UMoED") is UMoED and registry.get_runner_class("UMoEDTrainer") is UMoEDTrainer


def test_model_and_objective_read_the_configuration():
    from xmh.models.umoed import UMoED, UMoEDObjective
    get = lambda c: types.SimpleNamespace(get=lambda k, d=None: c.get(k, d))         # noqa: E731
    k = UMoEDObjective.from_config(CONFIG_YAML).consts
    assert (k.extreme, round(k.extreme_T, 6), round(k.token_triplet_margin, 6), k.triplet_alpha, round(k.unif_alpha, 6)) == (1, 0.3, 0.1, 1.0, 0.8)
    d = UMoEDObjective.from_config({"distance": {"mode": "pairwise"}}).consts         # the reference's defaults
    assert (d.extreme, round(d.extreme_T, 6), round(d.token_triplet_margin, 6), d.triplet_alpha, round(d.unif_alpha, 6)) == (1, 0.01, 0.2, 1.0, 0.01)
    small = dict(CONFIG_YAML, clip_path=SMALL, setDim=4, decoder_heads=1, decoder_layers=1, num_experts=2, slots_per_expert=2, hidden_dim=64)
    m = UMoED.from_config(get(small), output_dim=4, txt_token_size=32)
    th = m.hash.hash_module
    assert (m.hash_func, m.output_dim, m.visual_token_size, m.txt_token_size, m.extreme, m.extreme_T) == ("linear_subspace", 4, 5, 32, True, 0.3)
    assert tuple(th.decoder_learned_parameters.shape) == (4, 64) and tuple(th.classifier.weight.shape) == (2, 64) and th.MoE
    assert tuple(th.decoder.layers[0].moe.phi.shape) == (2048, 2, 2) and m.objective.consts.extreme == 1
    assert all(key.split(".")[0] in ("backbone", "hash") for key in m.state_dict())
    # the reference's from_config defaults: softmax + mean (output_dim doubles), extreme True, 3 experts, no MoE, fusion
    dflt = UMoED.from_config(get({"clip_path": SMALL, "setDim": 4, "decoder_heads": 1, "decoder_layers": 1, "hidden_dim": 64}), output_dim=4)
    assert (dflt.hash_func, dflt.output_dim, dflt.extreme, dflt.extreme_T, dflt.hash.fusion, dflt.hash.hash_module.MoE) == ("softmax", 8, True, 0.01, True, False)
    assert tuple(dflt.hash.hash_module.classifier.weight.shape) == (4, 64) and dflt.hash.hash_module.num_experts == 3
    assert dflt.objective is None                                                    # distance.mode defaults to chamfer: said when asked for
    z = torch.zeros(2, 4, 4)
    with pytest.raises(NotImplementedError, match="distance.mode 'chamfer'"):
        dflt.object_function(z, None, z, None)
    assert UMoED(None, outputDim=4, clipPath=SMALL, setDim=4, decoder_heads=1, decoder_layers=1, hidden_dim=64, hash_func="tanh").extreme is False
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.objective(z, z, torch.ones(2, 3))


def test_what_is_not_built_is_refused_with_the_key_named():
    from xmh.models.umoed import UMoEDHashLayer, UMoEDObjective, UMoEDTokenHash
    with pytest.raises(NotImplementedError, match="distance.mode 'smooth_chamfer'"):
        UMoEDObjective(mode="smooth_chamfer")
    with pytest.raises(NotImplementedError, match="distance_mode 'euclidean'"):
        UMoEDObjective(mode="pairwise", distance_mode="euclidean")
    with pytest.raises(NotImplementedError, match="triplet False"):
        UMoEDObjective(mode="pairwise", triplet=False)
    with pytest.raises(NotImplementedError, match="hidden_dim 256 != embed_dim 512"):
        UMoEDTokenHash(MoE=True, hidden_dim=256, embedDim=512)
    for pair in (("linear_subspace", "mean"), ("tanh", "concatenate"), ("softmax", "concatenate")):
        with pytest.raises(NotImplementedError, match="hash_func '%s' with merge_func '%s'" % pair):
            UMoEDHashLayer(hash_func_=pair[0], merge_func_=pair[1], decoder_layers=1, img_feature_size=64, hidden_dim=64, decoder_heads=1, dim_feedforward=8)
    with pytest.raises(ValueError, match="Unsupported hash func"):
        UMoEDHashLayer(hash_func_="sign")
    with pytest.raises(ValueError, match="Unsupported merge func"):
        UMoEDHashLayer(hash_func_="tanh", merge_func_="bitwise")


# ---- the C entry points ---------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_prototyped():
    from xmh import _lib
    header = open(os.path.join(ROOT, "include", "xmh.h")).read()
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header) and hasattr(so, name) and name in _lib.PROTOTYPES, name


def test_structs_match_the_header():
    from xmh import _lib
    header = open(os.path.join(ROOT, "include", "xmh.h")).read()
    for struct, cls in (("xmh_umoed_layer", _lib.UmoedLayer), ("xmh_umoed_head", _lib.UmoedHead), ("xmh_umoed_consts", _lib.UmoedConsts)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = []
        for decl in body.split(";"):
            words = decl.strip().split(None, 1 + decl.strip().startswith("const"))
            if words:
                names += [n.strip(" *\n") for n in words[-1].split(",")]
        assert names == [n for n, _ in cls._fields_], (struct, names)
    assert ctypes.sizeof(_lib.UmoedConsts) == 20 and ctypes.sizeof(_lib.UmoedLayer) == 21 * ctypes.sizeof(ctypes.c_void_p)


def _head(layers=None, n_layers=1, E=128, d=128, heads=2, F=2048, M=3, V=2, n=2, p=2, moe=1, hash_func=0, merge=0, first=None, q=256, lin2=None):
    from xmh import _lib
    if layers is None:
        layers = (_lib.UmoedLayer * n_layers)()
        for y in layers:
            for k in _lib.UmoedLayer.NAMES:
                setattr(y, k, 256)
            if moe:
                y.lin2_w = y.lin2_b = None
            else:
                y.phi = y.exp_w = y.exp_b = None
                y.lin2_w = y.lin2_b = lin2 if lin2 is not None else 256
    return _lib.UmoedHead(layers, n_layers, first, first, q, 256, 256, E, d, heads, F, M, V, n, p, moe, hash_func, merge, 1e-5), layers


def test_head_argument_errors_and_bounds_without_a_gpu():
    from xmh import _lib
    L = _lib.lib
    one, big = ctypes.c_void_p(256), 1 << 30                                         # never dereferenced: every call fails before a launch
    nb = lambda B=2, T=5, **kw: L.xmh_head_umoed_bytes(B, T, ctypes.byref(_head(**kw)[0]))          # noqa: E731

    def run(B=2, T=5, x=one, e=one, c=one, ws=one, nbytes=big, **kw):
        h, keep = _head(**kw)
        return L.xmh_head_umoed(ctypes.byref(h), x, B, T, e, c, ws, nbytes, None)

    need = nb()
    assert need >= 4 * 2 * 3 * (2048 + 7 * 128) and nb(B=100, T=50, E=512, d=512, heads=8, M=64, n=8, p=8, n_layers=6) > 0
    assert nb(B=256, T=128, M=128, n=16, p=16, V=256, F=4096, d=1024, heads=16, E=2048, first=256) > 0                    # every bound at once
    assert L.xmh_head_umoed_bytes(2, 5, None) == 0 and nb(B=0) == 0 and nb(T=0) == 0 and nb(M=0) == 0
    outside = [dict(d=128, heads=4), dict(M=129), dict(T=129), dict(E=2049, first=256), dict(d=1088, heads=17, E=1088), dict(F=4097),
               dict(n=16, p=17), dict(V=512), dict(V=3), dict(B=257, M=128), dict(B=65536, M=1, T=1)]
    for kw in outside:
        assert nb(**kw) == 0, kw
        assert run(**kw) == -95, (kw, L.xmh_last_error())
    assert run(d=128, heads=4) == -95 and b"head dim" in L.xmh_last_error()
    assert run(M=129) == -95 and b"M <= 128" in L.xmh_last_error()
    assert run(n=16, p=17) == -95 and b"S <= 256" in L.xmh_last_error()
    assert run(V=3) == -95 and b"power of two" in L.xmh_last_error()
    assert nb(V=3, moe=0, hash_func=1, merge=1) > 0 and nb(V=3, moe=0, hash_func=2, merge=1) == 0      # the pair softmax needs an even V
    for kw in (dict(x=None), dict(e=None), dict(c=None), dict(ws=None), dict(q=None), dict(B=0), dict(F=0), dict(hash_func=3), dict(hash_func=0, merge=1),
               dict(hash_func=1, merge=0), dict(E=192), dict(moe=0, lin2=0), dict(ws=ctypes.c_void_p(260))):
        assert run(**kw) == -22, (kw, L.xmh_last_error())
    assert b"xmh_head_umoed" in L.xmh_last_error()
    h, keep = _head()
    keep[0].phi = None
    assert L.xmh_head_umoed(ctypes.byref(h), one, 2, 5, one, one, one, big, None) == -22 and b"layer 0" in L.xmh_last_error()
    assert run(nbytes=need - 1) == -12 and b"workspace" in L.xmh_last_error()


def test_loss_argument_errors_and_bounds_without_a_gpu():
    from xmh import _lib
    L = _lib.lib
    one, big = ctypes.c_void_p(256), 1 << 30
    ws = L.xmh_umoed_loss_ws_bytes
    assert ws(512, 128, 256, 127) > 0 and ws(1, 1, 1, 1) > 0 and 0 < ws(100, 64, 2, 24) < 1 << 20
    assert ws(513, 8, 2, 5) == 0 and ws(20, 129, 2, 5) == 0 and ws(20, 8, 257, 5) == 0 and ws(20, 8, 2, 128) == 0
    assert ws(0, 8, 2, 5) == 0 and ws(20, 0, 2, 5) == 0 and ws(20, 8, 0, 5) == 0 and ws(20, 8, 2, 0) == 0
    good = _lib.UmoedConsts(1, 0.3, 0.1, 1.0, 0.8)
    need = ws(4, 3, 2, 5)

    def loss(B=4, M=3, V=2, C=5, e=one, lab=one, cst=good, wsp=one, nbytes=big, out=one):
        return L.xmh_umoed_loss(e, one, B, M, V, C, lab, ctypes.byref(cst) if cst is not None else None, wsp, nbytes, out, None)

    def grad(B=4, M=3, V=2, C=5, e=one, lab=one, cst=good, wsp=one, nbytes=big, outs=(one, one)):
        return L.xmh_umoed_loss_grad(e, one, B, M, V, C, lab, ctypes.byref(cst) if cst is not None else None, None, *outs, 0, wsp, nbytes, None)

    for fn, who in ((loss, b"xmh_umoed_loss"), (grad, b"xmh_umoed_loss_grad")):
        assert fn(e=None) == -22 and who in L.xmh_last_error()
        assert fn(B=0) == -22 and fn(M=0) == -22 and fn(V=0) == -22 and fn(C=0) == -22
        assert fn(B=513) == -95 and b"B <= 512" in L.xmh_last_error()
        assert fn(M=129) == -95 and fn(V=257) == -95 and fn(C=128) == -95
        assert fn(lab=None) == -22 and fn(cst=None) == -22 and fn(wsp=None) == -22
        assert fn(cst=_lib.UmoedConsts(1, 0.0, 0.1, 1.0, 0.8)) == -22 and b"extreme_T" in L.xmh_last_error()
        assert fn(nbytes=need - 1) == -12 and b"workspace" in L.xmh_last_error()
        assert fn(wsp=ctypes.c_void_p(260)) == -22
    assert loss(out=None) == -22
    assert grad(outs=(None, None)) == 0                                              # nothing asked for
