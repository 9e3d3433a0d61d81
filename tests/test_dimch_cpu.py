"""No GPU: the float64 restatement of DIMCH's objective (tests/dimch_cases.py) against the golden of the reference's own
DIMCH.object_function in float64 and float32 (tests/golden/dimch.npz, tools/make_golden_dimch.py); the guards of the case pool; the
designed clamp case and the row without a label; the new C symbols, their argument errors and workspace bounds; the constants of the
Python layer; the head's restatement against the golden head case, its state dict against the golden keys and shapes, the registry and
the model's ``from_config``.

Tolerance against the golden: the float64 numbers are the same expression evaluated twice (the restatement uses a max-subtracted
log-sum-exp and never forms the [N, N, N] tensor), so 1e-12 relative -- every scalar relative to itself, every gradient relative to
its largest entry.  The reference's float32 numbers lie within its own recorded float32-against-float64 deviation of that tensor
kind; 4 times that is allowed.  A margin of the wrong sign or a weight 1 % off is far outside either."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import dimch_cases as DC
from conftest import ROOT

NEW = ("xmh_dimch_loss_ws_bytes", "xmh_dimch_loss", "xmh_dimch_loss_grad", "xmh_head_dimch_bytes", "xmh_head_dimch",
       "xmh_head_dimch_train_forward", "xmh_head_dimch_backward")
SMALL = "synthetic:1814:vision_layers=1,transformer_layers=1,vision_width=128,transformer_width=128,embed_dim=64,image_resolution=64"
# the model block of the reference's configs/DIMCH/config.yaml, copied
CONFIG_YAML = {"arch": "DIMCH", "model_type": "base", "clip_path": "./ViT-B-32.pt", "setDim": 8, "dropout": 0.3, "hash_func": "tanh",
               "merge_func": "mean",
               "distance": {"mode": "smooth_chamfer", "denominator": 2.0, "temperature": 16.0, "temperature_txt_scale": 1.0},
               "chamfer": {"margin": 0.2, "mmd_gamma": 0.5, "semi_hard_triplet": False, "max_violation": True, "mmd_alpha": 1, "unif_alpha": 0.3,
                           "token_triplet_margin": 0.3},
               "hash_pars": {"triplet_alpha": 50, "infonce_alpha": 0.1, "quan_alpha": 1.0, "hash_triplet_alpha": 50, "triplet_margin": 0.3}}


def _golden(name):
    G = np.load(DC.GOLDEN)
    g = {k.split("__", 1)[1]: G[k] for k in G.files if k.startswith(name + "__")}
    c = dict(DC.GOLDEN_CASES[name], **{k: g[k] for k in DC.INPUTS}, labels=g["labels"].astype(np.int64), up=1.0)
    return g, c, {kind: float(G["deviation__" + kind]) for kind in DC.KINDS}


@pytest.mark.parametrize("name", list(DC.GOLDEN_CASES))
def test_restatement_reproduces_the_reference(name):
    g, c, dev = _golden(name)
    k = DC.consts(c)
    assert str(g["mode"]) == k["mode"] and str(g["hash_func"]) == k["hash_func"] and g["e_img"].shape == (c["B"], c["M"], c["K"])
    assert all(float(g[f]) == float(k[f]) for f in DC.CONST_KEYS if f not in ("mode", "hash_func"))
    assert c["B"] * c["M"] <= 576
    r = DC.objective(c, torch.float64)
    e64 = {key: DC.rel_err(r[key], g["f64_" + key]) for key in DC.TERMS + DC.GRADS}
    e32 = {key: DC.rel_err(r[key], g["f32_" + key]) for key in DC.TERMS + DC.GRADS}
    print(name, "f64:", " ".join("%s %.1e" % kv for kv in e64.items()))
    print(name, "f32:", " ".join("%s %.1e" % kv for kv in e32.items()))
    assert all(v <= 1e-12 for v in e64.values()), e64
    assert all(v <= DC.TOL_FACTOR * dev[DC.kind_of(key)] for key, v in e32.items()), (e32, dev)
    # what the bounds are there for: a margin of the wrong sign, or a weight 1 % off, is far outside them
    wrong = {"margin": DC.objective(c, torch.float64, token_triplet_margin=-k["token_triplet_margin"]),
             "weight": DC.objective(c, torch.float64, triplet_alpha=1.01 * k["triplet_alpha"])}
    for what, w in wrong.items():
        for key in ("loss", "g_e_img", "g_e_txt"):
            e = DC.rel_err(w[key], g["f32_" + key])
            print(name, "wrong", what, key, "%.2e" % e)
            assert e > 100 * DC.TOL_FACTOR * dev[DC.kind_of(key)], (what, key, e)


def test_recorded_deviation_is_a_yardstick():
    G = np.load(DC.GOLDEN)
    dev = {kind: float(G["deviation__" + kind]) for kind in DC.KINDS}
    print(dev)
    assert all(0 < v < 1e-3 for v in dev.values()), dev
    pool = DC.pool()
    print(pool)
    assert set(pool) == set(DC.KINDS) and all(0 < v < 1e-3 for v in pool.values()), pool


@pytest.mark.parametrize("name", list(DC.CASES))
def test_case_pool_is_guarded(name):
    """in float64 no masked hinge argument and no 1 - s is nearer than 1e-5 to zero, no top-2 gap behind a maximum below 1e-4"""
    c = DC.build(name)
    p = DC.guards(c)
    print(name, "seed", c["seed"], p)
    assert DC.guarded(p)
    assert "one_minus_s" in p and (c["C"] == 1 or "hinge" in p)
    assert ("gap" in p) == (DC.consts(c)["mode"] in ("chamfer", "max") and c["M"] > 1)
    assert c["labels"].sum(1).min() >= 1
    r = DC.reference(name)
    assert all(np.isfinite(v).all() for v in r.values())
    assert (r["unif"][0] == 0) == (c["M"] == 1)


def test_designed_clamp_case():
    """sample CLAMP_ROW's text tokens are its image tokens: s > 1 there, clamp(1 - s, 0) is active and its gradient is zero there"""
    c = DC.build("b7_m5_k6_clamp")
    r = DC.CLAMP_ROW
    assert np.array_equal(c["e_img"][r], c["e_txt"][r])
    x = torch.nn.functional.normalize(torch.tensor(c["e_img"], dtype=torch.float64).reshape(-1, c["K"]), dim=-1)
    y = torch.nn.functional.normalize(torch.tensor(c["e_txt"], dtype=torch.float64).reshape(-1, c["K"]), dim=-1)
    s = DC.set_similarity(x, y, c["M"], DC.consts(c))
    assert float(1 - s[r, r]) < -1e-5
    off = s.clone()
    off[r, r] = 0
    assert float((1 - off).min()) > 1e-5                                             # nowhere else
    # the clamp's zero gradient: the loss does not move with s[r][r], so the triplet terms give the same value with it pushed further
    lab = torch.tensor(c["labels"], dtype=torch.float64)
    m = DC.consts(c)["token_triplet_margin"]
    far = s.clone()
    far[r, r] += 0.5
    assert float(DC.triplet_term(torch.clamp(1 - s, 0), lab, m)) == float(DC.triplet_term(torch.clamp(1 - far, 0), lab, m))
    ref = DC.reference("b7_m5_k6_clamp")
    assert np.isfinite(ref["g_e_img"]).all() and np.abs(ref["g_e_img"][r]).max() > 0


def test_a_row_without_a_label_gives_nan():
    c = dict(DC.build("b7_m5_k6_smooth"))
    c["labels"] = c["labels"].copy()
    c["labels"][0] = 0
    for dtype in (torch.float64, torch.float32):
        r = DC.objective(c, dtype)
        assert all(np.isnan(r[k][0]) for k in ("loss", "T_i2t", "T_t2i", "Th_i2t", "Th_t2i"))
        assert all(np.isfinite(r[k][0]) for k in ("mmd", "unif", "Q_img", "Q_txt"))


def test_new_symbols_are_declared_exported_and_prototyped():
    from xmh import _lib
    header = open(os.path.join(ROOT, "include", "xmh.h")).read()
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header) and hasattr(so, name) and name in _lib.PROTOTYPES, name


def test_consts_struct_matches_the_header():
    """the ctypes structure has the header's fields in the header's order"""
    from xmh.models.dimch import DimchConsts
    header = open(os.path.join(ROOT, "include", "xmh.h")).read()
    body = re.search(r"typedef struct xmh_dimch_consts \{(.*?)\} xmh_dimch_consts;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            kind, rest = decl.split(None, 1)
            names += [(n.strip(), kind) for n in rest.split(",")]
    assert names == [(n, "int" if t is ctypes.c_int else "float") for n, t in DimchConsts._fields_]
    assert ctypes.sizeof(DimchConsts) == 4 * len(names)


def test_argument_errors_and_workspace_bounds_without_a_gpu():
    from xmh import _lib
    from xmh.models.dimch import DimchConsts
    L = _lib.lib
    one = ctypes.c_void_p(256)                                                       # never dereferenced: every call fails before a launch
    big = 1 << 30
    ws = L.xmh_dimch_loss_ws_bytes
    assert 0 < ws(128, 64, 64, 80) <= 32 << 20                                       # no N x N buffer: that alone would be 256 MiB
    assert ws(512, 64, 256, 127) > 0 and ws(1, 1, 1, 1) > 0
    assert ws(513, 8, 16, 80) == 0 and ws(20, 65, 16, 80) == 0 and ws(20, 8, 257, 80) == 0 and ws(20, 8, 16, 128) == 0
    assert ws(0, 8, 16, 80) == 0 and ws(20, 0, 16, 80) == 0 and ws(20, 8, 0, 80) == 0 and ws(20, 8, 16, 0) == 0
    # O(N K + B^2): doubling M doubles the N K part and leaves the rest
    assert ws(64, 64, 64, 80) - ws(64, 32, 64, 80) <= 2 * (ws(64, 32, 64, 80) - ws(64, 16, 64, 80)) + 4096
    need = ws(4, 3, 16, 5)
    good = DimchConsts(0, 0, 2.0, 16.0, 1.0, 0.3, 0.3, 0.5, 50.0, 1.0, 0.3, 50.0, 1.0)

    def loss(B=4, M=3, K=16, Kh=16, C=5, e=one, lab=one, cst=good, wsp=one, nbytes=big, out=one):
        return L.xmh_dimch_loss(e, one, one, one, B, M, K, Kh, C, lab, ctypes.byref(cst) if cst is not None else None, wsp, nbytes, out, None)

    def grad(B=4, M=3, K=16, Kh=16, C=5, e=one, lab=one, cst=good, wsp=one, nbytes=big, outs=(one,) * 4):
        return L.xmh_dimch_loss_grad(e, one, one, one, B, M, K, Kh, C, lab, ctypes.byref(cst) if cst is not None else None, None, *outs, 0, wsp,
                                     nbytes, None)

    for fn, who in ((loss, b"xmh_dimch_loss"), (grad, b"xmh_dimch_loss_grad")):
        assert fn(e=None) == -22 and who in L.xmh_last_error()
        assert fn(B=0) == -22 and fn(M=0) == -22 and fn(K=0) == -22 and fn(Kh=0) == -22 and fn(C=0) == -22
        assert fn(B=513) == -95 and fn(M=65) == -95 and fn(K=257) == -95 and fn(Kh=257) == -95 and fn(C=128) == -95
        assert fn(lab=None) == -22 and fn(cst=None) == -22 and fn(wsp=None) == -22
        assert fn(cst=DimchConsts(4, 0, 2.0, 16.0, 1.0, 0.3, 0.3, 0.5, 50.0, 1.0, 0.3, 50.0, 1.0)) == -22 and b"mode" in L.xmh_last_error()
        assert fn(cst=DimchConsts(0, 2, 2.0, 16.0, 1.0, 0.3, 0.3, 0.5, 50.0, 1.0, 0.3, 50.0, 1.0)) == -22
        assert fn(cst=DimchConsts(0, 0, 2.0, 0.0, 1.0, 0.3, 0.3, 0.5, 50.0, 1.0, 0.3, 50.0, 1.0)) == -22             # temperature 0
        assert fn(nbytes=need - 1) == -12 and b"workspace" in L.xmh_last_error()
        assert fn(wsp=ctypes.c_void_p(260)) == -22
    assert loss(out=None) == -22
    assert grad(outs=(None,) * 4) == 0                                               # nothing asked for


def test_python_layer_reads_the_configuration():
    from xmh.models.dimch import DIMCHObjective, mode_index
    obj = DIMCHObjective.from_config(CONFIG_YAML)
    k = obj.consts
    assert (k.mode, k.hash_func) == (0, 0) and obj.mode == "smooth_chamfer" and obj.hash_func == "tanh"
    got = {f: getattr(k, f) for f in DC.CONST_KEYS if f not in ("mode", "hash_func")}
    assert got == {f: np.float32(DC.CONFIG[f]) for f in got}, got                    # dimch_cases.CONFIG is the same configuration
    d = DIMCHObjective.from_config({}).consts                                        # the reference's defaults (DIMCH.py:44-63, :94)
    assert (d.mode, d.hash_func) == (1, 1)
    assert [round(getattr(d, f), 6) for f in ("denominator", "temperature", "temperature_txt_scale", "token_triplet_margin", "triplet_margin",
                                              "mmd_gamma", "triplet_alpha", "mmd_alpha", "unif_alpha", "hash_triplet_alpha", "quan_alpha")] \
        == [2.0, 16.0, 1.0, 0.2, 0.3, 0.5, 1.0, 0.01, 0.01, 0.5, 0.001]
    assert [mode_index(m) for m in DC.MODES] == [0, 1, 2, 3]
    with pytest.raises(ValueError):
        mode_index("median")
    with pytest.raises(ValueError):
        DIMCHObjective(hash_func="sign")
    z = torch.zeros(2, 3, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        obj(z, torch.zeros(2, 4), z, torch.zeros(2, 4), torch.ones(2, 5))


# ---- head, model, runner -----------------------------------------------------------------------------------------------------------
def test_head_restatement_reproduces_the_reference():
    """the golden head case (T = 5, E = 64, M = 3, K = 6, eval mode, B = 4): float64 to 1e-12, float32 within 4 times the recorded
    float32-against-float64 deviation of the head"""
    G = np.load(DC.GOLDEN)
    g = {k.split("__", 1)[1]: G[k] for k in G.files if k.startswith("head__")}
    dev = float(G["deviation__head"])
    assert 0 < dev < 1e-5 and g["x"].shape == (4, 5, 64) and g["conv_w"].shape == (3, 5, 3) and g["w2"].shape == (6, 32)
    r = DC.head(g["x"], {k: g[k] for k in DC.HEAD_PARAMS}, None, 0.0, "tanh", torch.float64, g["g_embeds"], g["g_hash"])
    e64 = {k: DC.rel_err(v, g["f64_" + k]) for k, v in r.items()}
    e32 = {k: DC.rel_err(v, g["f32_" + k]) for k, v in r.items()}
    print("f64:", e64)
    print("f32:", e32)
    assert set(r) == {"embeds", "hash", "g_x"} | {"g_" + k for k in DC.HEAD_PARAMS}
    assert all(v <= 1e-12 for v in e64.values()), e64
    assert all(v <= DC.TOL_FACTOR * dev for v in e32.values()), (e32, dev)
    # a convolution that runs the other way (taps reversed) is far outside
    flipped = dict({k: g[k] for k in DC.HEAD_PARAMS}, conv_w=g["conv_w"][:, :, ::-1].copy())
    assert DC.rel_err(DC.head(g["x"], flipped, None, 0.0, "tanh", torch.float64)["embeds"], g["f64_embeds"]) > 1e-3


@pytest.mark.parametrize("name", list(DC.HEAD_CASES))
def test_head_case_pool_is_guarded(name):
    c = DC.head_case(name)
    print(name, "seed", c["seed"], "relu guard", c["relu"])
    assert c["relu"] >= DC.HEAD_GUARD and (c["keep"] is None) == (c["p"] == 0)
    r = DC.head_reference(name)
    assert r["embeds"].shape == (c["B"], c["M"], c["K"]) and r["hash"].shape == (c["B"], c["K"]) and r["g_x"].shape == c["x"].shape
    assert all(np.isfinite(v).all() and np.abs(v).max() > 0 for v in r.values())
    if c["hash_func"] == "softmax":
        assert np.allclose(r["hash"].reshape(c["B"], -1, 2).sum(-1), 1.0)


def test_head_cases_cover_the_shapes():
    vals = {k: {c[k] for c in DC.HEAD_CASES.values()} for k in ("T", "E", "M", "K", "B")}
    assert vals == {"T": {5, 50, 32}, "E": {64, 512}, "M": {1, 3, 8, 64}, "K": {6, 16, 128}, "B": {1, 2, 37}}


def test_registry_resolves_dimch():
    import xmh.models  # noqa: F401
    import xmh.runners  # noqa: F401
    from xmh.common.register import registry
    from xmh.models.dimch import DIMCH
    from xmh.runners.methods import DIMCHTrainer
    assert registry.get_model_class("DIMCH") is DIMCH and registry.get_runner_class("DIMCHTrainer") is DIMCHTrainer


def test_head_state_dict_is_the_reference_s_and_loads_strictly():
    from xmh.models.dimch import DIMCHHashLayer
    G = np.load(DC.GOLDEN)
    want = {k.split("__", 1)[1]: tuple(int(n) for n in G[k]) for k in G.files if k.startswith("state__")}
    assert len(want) == 12
    head = DIMCHHashLayer(50, 32, 512, 16, setDim=8)
    assert {k: tuple(v.shape) for k, v in head.state_dict().items()} == want
    assert list(head.state_dict()) == list(want)                                     # the reference's order too
    g = torch.Generator().manual_seed(1)
    sd = {k: torch.randn(shape, generator=g) for k, shape in want.items()}
    assert head.load_state_dict(sd, strict=True).missing_keys == []
    assert torch.equal(head.txt_token_hash.hash_layer[3].weight, sd["txt_token_hash.hash_layer.3.weight"])
    # weights_init_kaiming: zero biases, the linear layers uniform within sqrt(6 / fan_out), the convolution normal with std sqrt(2 / fan_in)
    fresh = DIMCHHashLayer(50, 32, 512, 16, setDim=8).img_token_hash
    assert all(float(b.detach().abs().max()) == 0 for b in (fresh.token_layer.bias, fresh.hash_layer[0].bias, fresh.hash_layer[3].bias))
    assert float(fresh.hash_layer[0].weight.detach().abs().max()) <= (6.0 / 256) ** 0.5
    assert 0.8 < float(fresh.token_layer.weight.detach().std()) / (2.0 / 150) ** 0.5 < 1.2
    torch.manual_seed(5)                                                             # the values come from the head's own seeded generator
    assert torch.equal(fresh.token_layer.weight, DIMCHHashLayer(50, 32, 512, 16, setDim=8).img_token_hash.token_layer.weight)
    assert not torch.equal(fresh.token_layer.weight, DIMCHHashLayer(50, 32, 512, 16, setDim=8, seed=3).img_token_hash.token_layer.weight)
    with pytest.raises(NotImplementedError):
        DIMCHHashLayer(add_global=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        head.eval().encode_img(torch.zeros(2, 50, 512))


def test_head_struct_matches_the_header():
    from xmh import _lib
    header = open(os.path.join(ROOT, "include", "xmh.h")).read()
    for struct, cls in (("xmh_dimch_head", _lib.DimchHead), ("xmh_dimch_head_grads", _lib.DimchHeadGrads)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n.strip(" *") for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1 + decl.strip().startswith("const"))[-1].split(",")]
        assert names == [n for n, _ in cls._fields_], (struct, names)


def test_head_argument_errors_without_a_gpu():
    from xmh import _lib
    L = _lib.lib
    one = ctypes.c_void_p(256)                                                       # never dereferenced: every call fails before a launch
    wsb = ctypes.c_size_t(0)
    nb = L.xmh_head_dimch_bytes
    saved = nb(20, 50, 512, 256, 8, 16, ctypes.byref(wsb))
    assert saved >= 4 * (20 * 8 * (512 + 256) + 20 * 16) and wsb.value >= 4 * 20 * 8 * (512 + 256 + 16)
    assert nb(512, 50, 512, 256, 64, 256, None) > 0 and nb(1, 1, 1, 1, 1, 1, None) > 0
    assert nb(513, 50, 512, 256, 64, 16, None) == 0 and nb(2, 257, 512, 256, 8, 16, None) == 0 and nb(2, 50, 4096, 256, 8, 16, None) == 0
    assert nb(2, 50, 512, 256, 8, 257, ctypes.byref(wsb)) == 0 and wsb.value == 0 and nb(0, 50, 512, 256, 8, 16, None) == 0

    def desc(T=5, E=64, H=32, M=3, K=6, hf=0, w=256):
        return _lib.DimchHead(w, 256, 256, 256, 256, 256, T, E, H, M, K, hf)

    big = 1 << 30
    fwd = lambda d=None, x=one, B=4, e=one, h=one, buf=one, n=big: L.xmh_head_dimch(ctypes.byref(d or desc()), x, B, e, h, buf, n, None)   # noqa: E731
    trn = lambda d=None, x=one, B=4, e=one, h=one, buf=one, n=big, p=0.3: L.xmh_head_dimch_train_forward(   # noqa: E731
        ctypes.byref(d or desc()), x, one, p, B, e, h, buf, n, None)
    grads = _lib.DimchHeadGrads(*([256] * 7))
    bwd = lambda d=None, x=one, B=4, buf=one, n=big, p=0.3, g=grads, ws=one: L.xmh_head_dimch_backward(   # noqa: E731
        ctypes.byref(d or desc()), x, 1, p, one, one, B, buf, n, ctypes.byref(g) if g is not None else None, 0, ws, big, None)
    need = nb(4, 5, 64, 32, 3, 6, None)
    for fn, who in ((fwd, b"xmh_head_dimch"), (trn, b"xmh_head_dimch_train_forward"), (bwd, b"xmh_head_dimch_backward")):
        assert fn(x=None) == -22 and who in L.xmh_last_error()
        assert fn(d=desc(w=None)) == -22 and fn(B=0) == -22 and fn(d=desc(T=0)) == -22 and fn(d=desc(hf=2)) == -22
        assert fn(d=desc(K=7, hf=1)) == -22 and b"odd" in L.xmh_last_error()
        assert fn(d=desc(M=65), B=512) == -95 and fn(d=desc(T=257)) == -95 and fn(d=desc(K=257)) == -95 and fn(d=desc(E=2049)) == -95
        assert fn(buf=None) == -22 and fn(n=need - 1) == -22 and fn(buf=ctypes.c_void_p(260)) == -22
    assert fwd(e=None) == -22 and trn(h=None) == -22 and trn(p=1.0) == -22 and bwd(p=-0.1) == -22 and bwd(g=None) == -22 and bwd(ws=None) == -22
    assert bwd(g=_lib.DimchHeadGrads()) == 0                                         # nothing asked for


def test_model_reads_the_configuration():
    import types
    from xmh.models.dimch import DIMCH
    get = lambda c: types.SimpleNamespace(get=lambda k, d=None: c.get(k, d))         # noqa: E731
    m = DIMCH.from_config(get(dict(CONFIG_YAML, clip_path=SMALL)), output_dim=16, txt_token_size=32)
    k = m.objective.consts
    assert (m.hash_func, m.output_dim, m.visual_token_size, m.txt_token_size, k.mode, k.hash_func) == ("tanh", 16, 5, 32, 0, 0)
    assert {f: getattr(k, f) for f in DC.CONST_KEYS if f not in ("mode", "hash_func")} == \
        {f: np.float32(DC.CONFIG[f]) for f in DC.CONST_KEYS if f not in ("mode", "hash_func")}
    th, tt = m.hash.img_token_hash, m.hash.txt_token_hash
    assert tuple(th.token_layer.weight.shape) == (8, 5, 3) and tuple(tt.token_layer.weight.shape) == (8, 32, 3)
    assert tuple(th.hash_layer[0].weight.shape) == (32, 64) and tuple(th.hash_layer[3].weight.shape) == (16, 32) and th.dropout_p == 0.3
    assert all(key.split(".")[0] in ("backbone", "hash") for key in m.state_dict())
    # the reference's defaults, and the doubling of output_dim for the pair softmax (DIMCH.py:92-98)
    d = DIMCH.from_config(get({"clip_path": SMALL}), output_dim=16)
    assert (d.hash_func, d.output_dim, d.objective.consts.hash_func, d.objective.consts.mode) == ("softmax", 32, 1, 1)
    assert tuple(d.hash.img_token_hash.hash_layer[3].weight.shape) == (32, 32) and tuple(d.hash.img_token_hash.token_layer.weight.shape) == (64, 5, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.eval().encode_text(torch.zeros(2, 32, dtype=torch.long))
