"""UMoED's train-mode decoder head without a GPU: the float64 restatement of tests/umoed_train_cases.py against what the
unmodified reference recorded in tests/golden/umoed_train.npz (tools/make_golden_umoed_train.py: no dropout, and p = 0.3 with replayed
masks) -- 1e-12 relative in float64, within four times the reference's largest recorded float32-against-float64 deviation in float32; the restatement
without masks against umoed_cases.head, exactly; the ReLU guard of the fixed seeds; the row counts the GPU cases were chosen for; the C
entry points' sizes, bounds and argument errors, which come back before any launch; the bindings against the header; the refusals."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import umoed_cases as UC
import umoed_train_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("xmh_head_umoed_train_bytes", "xmh_umoed_keep_bytes", "xmh_head_umoed_train_forward", "xmh_head_umoed_backward")


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", TC.SETTINGS)
def test_restatement_reproduces_the_reference(which):
    G = np.load(TC.GOLDEN)
    c = TC.case("golden")
    assert int(G["train__seed"]) == c["seed"]
    r64, r32 = TC.reference("golden", which), TC.reference("golden", which, torch.float32)
    mine64, where = TC.golden_vector(r64)
    mine32, _ = TC.golden_vector(r32)
    g64, g32 = G["train__%s__f64" % which], G["train__%s__f32" % which].astype(np.float64)
    assert mine64.shape == g64.shape == g32.shape
    assert len(where) == 3 + 19 * c["layers"] + 2 + 0 and "g_decoder.layers.1.moe.experts.weight" in where      # embeds, tokens, queries; classifier
    worst = 0.0
    pool = max(UC.rel_err(g32[sl], g64[sl]) for sl in where.values())                # the reference's largest float32 deviation over the tensors
    for key, sl in where.items():
        e64, e32 = UC.rel_err(mine64[sl], g64[sl]), UC.rel_err(mine32[sl], g64[sl])
        worst = max(worst, e64)
        assert e64 <= 1e-12, (which, key, e64)
        assert 0 < pool < 1e-5 and e32 <= UC.TOL_FACTOR * pool, (which, key, e32, pool)
    print(which, "worst float64 deviation from the reference %.2e over %d tensors" % (worst, len(where)))
    # the other setting's masks are far outside: the replay is what is compared
    other = TC.reference("golden", TC.SETTINGS[1 - TC.SETTINGS.index(which)])
    assert UC.rel_err(TC.golden_vector(other)[0][where["embeds"]], g64[where["embeds"]]) > 1e-3


@pytest.mark.parametrize("name", ["edge", "rows"])
def test_without_masks_the_restatement_is_the_inference_head_s(name):
    c = TC.case(name)
    ones = [[np.ones(s, np.uint8) for s in TC.keep_shapes(c)] for _ in range(c["layers"])]
    for dtype in (torch.float64, torch.float32):
        want = UC.head(c["x"], c["P"], c, dtype)["embeds"]
        assert np.array_equal(TC.head_train(c["x"], c["P"], c, dtype, c["G"])["embeds"], want)
        assert np.array_equal(TC.head_train(c["x"], c["P"], c, dtype, c["G"], ones, 0.0)["embeds"], want)
    dropped = TC.reference(name, "p03")["embeds"]
    assert UC.rel_err(dropped, TC.reference(name, "p0")["embeds"]) > 1e-2             # the masks act


@pytest.mark.parametrize("name", list(TC.TRAIN_CASES) + ["golden"])
def test_the_fixed_seeds_pass_the_relu_guard(name):
    c = TC.case(name)
    gap = TC.case_gap(c)
    print(name, "seed", c["seed"], "smallest |pre| / max|pre| %.2e" % gap)
    assert gap >= TC.RELU_GAP
    r = TC.reference(name, "p03")
    assert all(np.isfinite(v).all() and np.abs(v).max() > 0 for v in r.values())
    assert set(r) == {"embeds", "g_tokens"} | {"g_" + k for k in UC.head_shapes(c)}
    keep = TC.flat_keep(c["masks"])
    assert keep.dtype == np.uint8 and keep.size == c["layers"] * sum(int(np.prod(s)) for s in TC.keep_shapes(c)) and 0.6 < keep.mean() < 0.8


def test_the_seeds_are_the_first_guarded_ones():
    base = {"edge": 7401, "tiles": 7402, "rows": 7403}
    for name, spec in TC.TRAIN_CASES.items():
        seed = TC.find_seed(dict(spec, seed=base[name]))
        assert seed == spec["seed"] and (seed - base[name]) // 1000 <= TC.MAX_REDRAWS, (name, seed)


def _tn_split(M, N, K):
    """xmh::grad::tn_split (csrc/xmh_grad_kernels.hip), restated: how many chunks the row reduction of dW [N, K] over M rows is cut into"""
    cdiv = lambda a, b: -(-a // b)                                                   # noqa: E731
    s = max(1, min(cdiv(512, cdiv(N, 64) * cdiv(K, 64)), cdiv(M, 64), 16))
    return cdiv(M, cdiv(cdiv(M, s), 32) * 32)


def test_the_cases_reach_what_they_were_chosen_for():
    e, t, r = (TC.TRAIN_CASES[k] for k in ("edge", "tiles", "rows"))
    assert (e["B"], e["T"], e["M"], e["d"], e["heads"], e["F"], e["n"], e["p"], e["V"], e["layers"]) == (3, 7, 5, 64, 1, 24, 2, 2, 2, 1)
    assert (t["B"], t["T"], t["M"], t["d"], t["heads"], t["F"], t["n"], t["p"], t["V"], t["layers"]) == (2, 50, 70, 128, 2, 96, 3, 5, 16, 2)
    assert (r["B"], r["T"], r["M"], r["d"], r["heads"], r["F"], r["n"], r["p"], r["V"], r["layers"]) == (37, 33, 8, 64, 1, 40, 2, 3, 4, 2)
    assert t["M"] > 64 and r["B"] * r["M"] == 296 and r["B"] * r["p"] == 111
    # rows: the out-projections' [64, 64] gradients over 296 rows, the in-projection's [192, 64] and the tokens' side [128, 64] over 1221 rows,
    # and an expert's [40, 64] over 111 rows are all cut; edge: nothing is
    assert _tn_split(296, 64, 64) == 5 and _tn_split(296, 192, 64) == 5 and _tn_split(37 * 33, 128, 64) == 13 and _tn_split(111, 40, 64) == 2
    assert _tn_split(15, 64, 64) == 1 and _tn_split(6, 24, 64) == 1


# ---- the C entry points -------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_prototyped():
    from xmh import _lib
    header = open(os.path.join(ROOT, "include", "xmh.h")).read()
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header) and hasattr(so, name) and name in _lib.PROTOTYPES, name
        decl = re.search(r"^(?:size_t|int) %s\((.*?)\);" % name, header, re.S | re.M).group(1)
        assert len(decl.split(",")) == len(_lib.PROTOTYPES[name][1]), name            # one ctypes argument per declared parameter


def test_grad_structs_match_the_header():
    from xmh import _lib
    header = open(os.path.join(ROOT, "include", "xmh.h")).read()
    for struct, cls in (("xmh_umoed_layer_grads", _lib.UmoedLayerGrads), ("xmh_umoed_head_grads", _lib.UmoedHeadGrads)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = []
        for decl in body.split(";"):
            words = decl.strip().split(None, 1 + decl.strip().startswith("const"))
            if words:
                names += [n.strip(" *\n") for n in words[-1].split(",")]
        assert names == [n for n, _ in cls._fields_], (struct, names)
    assert _lib.UmoedLayerGrads.NAMES == _lib.UmoedLayer.NAMES[:19] and "lin2_w" not in _lib.UmoedLayerGrads.NAMES
    assert ctypes.sizeof(_lib.UmoedLayerGrads) == 19 * ctypes.sizeof(ctypes.c_void_p) and ctypes.sizeof(_lib.UmoedHeadGrads) == 5 * ctypes.sizeof(ctypes.c_void_p)


def _head(n_layers=1, E=128, d=128, heads=2, F=96, M=3, V=2, n=2, p=2, moe=1, first=None, eps=1e-5, q=256):
    from xmh import _lib
    layers = (_lib.UmoedLayer * n_layers)()
    for y in layers:
        for k in _lib.UmoedLayer.NAMES:
            setattr(y, k, 256)
        if moe:
            y.lin2_w = y.lin2_b = None
        else:
            y.phi = y.exp_w = y.exp_b = None
    return _lib.UmoedHead(layers, n_layers, first, first, q, 256, 256, E, d, heads, F, M, V, n, p, moe, 0, 0, eps), layers


def test_sizes_follow_the_documented_layout_and_are_zero_outside_the_bounds():
    from xmh import _lib
    L = _lib.lib

    def sizes(B=2, T=5, **kw):
        h, alive = _head(**kw)
        ws = ctypes.c_size_t(123)
        rec = L.xmh_head_umoed_train_bytes(B, T, ctypes.byref(h), ctypes.byref(ws))
        return rec, ws.value, L.xmh_umoed_keep_bytes(B, T, ctypes.byref(h))

    rec, ws, keep = sizes()
    B, T, H, M, d, F = 2, 5, 2, 3, 128, 96
    per_layer = B * H * M * M + B * M * d + B * H * M * T + B * M * d + B * M * F + B * M * d
    assert keep == per_layer and sizes(n_layers=3)[2] == 3 * per_layer
    # the record: the repeated queries, then per layer 12 row buffers of d (qkv counts three), kv, h, D and Cw, Xs, Ys -- in 256-byte pieces
    floats = B * M * d + (12 * B * M * d + 2 * B * T * d + B * M * F + 2 * B * M * 4 + B * 4 * F + B * 4 * d)
    assert 4 * floats <= rec <= 4 * floats + 17 * 256 and rec % 256 == 0 and ws > 0 and ws % 256 == 0
    assert sizes(n_layers=2)[0] - rec == rec - ((4 * B * M * d + 255) // 256) * 256                       # a layer more is a layer's bytes more
    r, w, k = sizes(B=100, T=50, E=512, d=512, heads=8, F=2048, M=64, n=8, p=8, n_layers=6)              # the configuration's shape
    assert 1.7e9 < r < 1.9e9 and 2.5e8 < w < 3.5e8 and k == 6 * (100 * 8 * 64 * (64 + 50) + 100 * 64 * (3 * 512 + 2048))
    assert sizes(B=256, T=128, M=128, n=16, p=16, V=256, F=4096, d=1024, heads=16, E=1024)[0] > 0          # every bound at once
    assert L.xmh_head_umoed_train_bytes(2, 5, None, None) == 0 and L.xmh_umoed_keep_bytes(2, 5, None) == 0
    h, alive = _head()
    assert L.xmh_head_umoed_train_bytes(2, 5, ctypes.byref(h), None) == rec                               # the workspace size is optional
    outside = [dict(moe=0), dict(first=256, E=192), dict(eps=1e-6), dict(B=0), dict(T=0), dict(M=129), dict(T=129), dict(d=128, heads=4),
               dict(F=4097), dict(n=16, p=17), dict(V=3), dict(B=257, M=128), dict(d=1088, heads=17, E=1088)]
    for kw in outside:
        assert sizes(**kw) == (0, 0, 0), kw


def test_argument_errors_come_back_before_any_launch():
    from xmh import _lib
    L = _lib.lib
    one, big = ctypes.c_void_p(256), 1 << 40                                         # never dereferenced: every call fails before a launch
    no_grads = _lib.UmoedHeadGrads(None, None, None, None, None)

    def fwd(B=2, T=5, x=one, keep=None, drop=0.3, e=one, c=one, rec=one, rec_bytes=big, ws=one, ws_bytes=big, **kw):
        h, alive = _head(**kw)
        return L.xmh_head_umoed_train_forward(ctypes.byref(h), x, keep, drop, B, T, e, c, rec, rec_bytes, ws, ws_bytes, None)

    def bwd(B=2, T=5, x=one, keep=None, drop=0.3, up=one, rec=one, rec_bytes=big, grads=no_grads, ws=one, ws_bytes=big, **kw):
        h, alive = _head(**kw)
        return L.xmh_head_umoed_backward(ctypes.byref(h), x, keep, drop, up, B, T, rec, rec_bytes, ctypes.byref(grads) if grads is not None else None, 0,
                                         ws, ws_bytes, None)

    h, alive = _head()
    wsb = ctypes.c_size_t(0)
    need = L.xmh_head_umoed_train_bytes(2, 5, ctypes.byref(h), ctypes.byref(wsb))
    for fn, who in ((fwd, b"xmh_head_umoed_train_forward"), (bwd, b"xmh_head_umoed_backward")):
        assert fn(moe=0) == -95 and b"plain decoder" in L.xmh_last_error() and who in L.xmh_last_error()
        assert fn(first=256, E=192) == -95 and b"first layer" in L.xmh_last_error()
        assert fn(eps=1e-6) == -95 and b"ln_eps" in L.xmh_last_error() and b"1e-5" in L.xmh_last_error()
        assert fn(M=129) == -95 and b"M <= 128" in L.xmh_last_error()
        assert fn(d=128, heads=4) == -95 and b"head dim" in L.xmh_last_error()
        assert fn(n=16, p=17) == -95 and b"S <= 256" in L.xmh_last_error()
        assert fn(F=4097) == -95 and fn(V=3) == -95 and fn(B=257, M=128) == -95
        for kw in (dict(x=None), dict(rec=None), dict(ws=None), dict(q=None), dict(B=0), dict(F=0), dict(keep=one, drop=1.0), dict(keep=one, drop=-0.1),
                   dict(rec=ctypes.c_void_p(260)), dict(ws=ctypes.c_void_p(260))):
            assert fn(**kw) == -22, (kw, L.xmh_last_error())
        assert fn(rec_bytes=need - 1) == -12 and b"xmh_head_umoed_train_bytes" in L.xmh_last_error()
        assert fn(ws_bytes=wsb.value - 1) == -12 and b"workspace" in L.xmh_last_error()
    assert fwd(e=None) == -22 and fwd(c=None) == -22 and bwd(up=None) == -22 and bwd(grads=None) == -22
    h, alive = _head()
    alive[0].phi = None
    assert L.xmh_head_umoed_train_forward(ctypes.byref(h), one, None, 0.0, 2, 5, one, one, one, big, one, big, None) == -22 and b"layer 0" in L.xmh_last_error()


# ---- the module ----------------------------------------------------------------------------------------------------------------------------
def _module(**over):
    from xmh.models.umoed import UMoEDTokenHash
    kw = dict(outputDim=2, embedDim=64, setDim=3, decoder_heads=1, decoder_layers=2, num_experts=2, slots_per_expert=2, MoE=True, hidden_dim=64,
              dim_feedforward=24, hash_func="linear_subspace", merge_func="concatenate")
    kw.update(over)
    return UMoEDTokenHash(**kw)


def test_keep_masks_are_drawn_as_bytes_from_the_module_s_generator():
    m = _module()
    assert m.dropout_p == 0.3 and m.generator is None
    want = 2 * (4 * 1 * 3 * 3 + 4 * 3 * 64 + 4 * 1 * 3 * 7 + 4 * 3 * 64 + 4 * 3 * 24 + 4 * 3 * 64)
    assert sum(m.keep_sections(4, 7)) * 2 == want
    m.generator = torch.Generator().manual_seed(5)
    a = m.draw_keep_mask(4, 7, "cpu")
    m.generator = torch.Generator().manual_seed(5)
    b = m.draw_keep_mask(4, 7, "cpu")
    assert a.dtype == torch.uint8 and a.numel() == want and torch.equal(a, b) and set(a.unique().tolist()) == {0, 1}
    assert 0.65 < float(a.float().mean()) < 0.75                                      # Bernoulli(1 - p)
    assert _module(dropout=0.0).draw_keep_mask(4, 7, "cpu") is None
    with pytest.raises(ValueError, match="nothing would be kept"):
        _module(dropout=1.0).draw_keep_mask(4, 7, "cpu")
    assert len(m.head_params()) == 1 + 19 * 2 + 2 and m.head_params()[0] is m.decoder_learned_parameters


def test_what_has_no_train_mode_is_refused_with_the_key_named():
    x = torch.zeros(2, 5, 64)
    with pytest.raises(NotImplementedError, match="MoE: False"):
        _module(MoE=False).forward_train(x)
    with pytest.raises(NotImplementedError, match="MoE: False"):
        _module(MoE=False).draw_keep_mask(2, 5, "cpu")
    with pytest.raises(NotImplementedError, match="first_layer"):
        _first_layer_module().forward_train(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _module().forward_train(x, keep=None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        with torch.no_grad():
            _module().forward_train(x)
    # the pinned entry points keep refusing, and say where training lives
    with pytest.raises(NotImplementedError, match="backward of the decoder head"):
        _module()(x)
    with pytest.raises(NotImplementedError, match="forward_train"):
        _module()(x)


def _first_layer_module():
    """a Soft-MoE head cannot have a first layer (the constructor refuses the pair), so one is attached to show the refusal's text"""
    m = _module()
    m.first_layer = torch.nn.Linear(96, 64)
    return m
