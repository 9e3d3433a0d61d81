"""No GPU: the golden file of MITH's training head against the cases and the restatement of tests/mith_head_grad_cases.py (the inputs
regenerate, the restatement's fp32 run reproduces every stored tensor and its fp64 run stays within the stored e_ref), the new C entry
points (declared, exported, prototyped; argument errors reported without a GPU), and the Python layer's refusals: CPU tensors,
dropout, and the three calls that still have no training path."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import mith_head_grad_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("xmh_mith_train_saved_bytes", "xmh_mith_train_ws_bytes", "xmh_mith_train_forward", "xmh_mith_train_backward")


@pytest.mark.parametrize("case", list(MC.CASES))
def test_golden_regenerates_and_the_restatement_reproduces_it(case):
    G = MC.golden()
    D, heads, layers, R, K, top_k, L, B, mod, mk = MC.CASES[case]
    sd, cls, tok, mask, ups = MC.case_inputs(case)
    assert int(G[case + "__seed"]) == MC.case_seed(case)
    assert MC.inputs_checksum(sd, cls, tok, mask, ups) == float(G[case + "__checksum"])
    r32 = MC.run_restatement(sd, cls, tok, mask, ups, heads, top_k, torch.float32)
    r64 = MC.run_restatement(sd, cls, tok, mask, ups, heads, top_k, torch.float64)
    assert np.array_equal(r32.pop("keep"), r64["keep"])                          # the seeds leave no selection tie between the two
    stored = {k.split("__", 1)[1] for k in G if k.startswith(case + "__") and "__eref_" not in k} - {"seed", "checksum"}
    assert stored == set(r32) and len(stored) == 4 + 2 + 6 * R + 1 + 12 * layers + 4
    for k, v in r32.items():
        assert np.array_equal(MC.thin(v), G["%s__%s" % (case, k)]), k            # to the bit
        e_ref = float(G["%s__eref_%s" % (case, k)])
        assert e_ref < 2e-6, (k, e_ref)                                          # the reference's fp32 run is a float32 computation of this head
        assert MC.rel_err(v, r64[k]) <= e_ref * (1 + 1e-9) + 1e-300, k
    keep = r64["keep"]                                                           # [L, B, K]
    assert (case in MC.EMPTY_CONCEPT_CASES) <= bool((~keep.any(axis=0)).any())
    if mask is not None:
        assert not keep.transpose(1, 0, 2)[mask].any() and not r64["g_tokens"].transpose(1, 0, 2)[mask].any()
    if mk == "pad_all":
        assert mask[1].all() and not r64["g_tokens"][:, 1].any()
    assert top_k <= K


def test_restatement_under_a_given_keep_set_and_the_margins():
    case = "k20_top8_l50_r1_txt_allmasked"
    D, heads, layers, R, K, top_k, L, B, mod, mk = MC.CASES[case]
    sd, cls, tok, mask, ups = MC.case_inputs(case)
    s = []
    own = MC.run_restatement(sd, cls, tok, mask, ups, heads, top_k, torch.float64, scores_out=s)
    given = MC.run_restatement(sd, cls, tok, mask, ups, heads, top_k, torch.float64, keep=own["keep"])
    assert all(np.array_equal(own[k], given[k]) for k in own)
    keep, margin = MC.selection(s[0], mask, top_k)
    assert np.array_equal(keep.numpy(), own["keep"]) and keep.sum(-1).max() <= top_k
    m = margin.numpy()
    assert np.isinf(m.transpose(1, 0, 2)[mask]).all() and (m[np.isfinite(m)] > 0).all()
    flipped = own["keep"].copy()
    flipped[0, 0] = ~flipped[0, 0]
    other = MC.run_restatement(sd, cls, tok, mask, ups, heads, top_k, torch.float64, keep=flipped)
    assert not np.array_equal(other["tokens_hash"][0], own["tokens_hash"][0]) and np.array_equal(other["tokens_hash"][1:], own["tokens_hash"][1:])


def test_lta_parent_entries_are_stored():
    G = MC.golden()
    assert G["lta_parent__thin"].dtype == np.float32 and G["lta_parent__thin"].size == 40 * 16 * 512 // MC.THIN
    assert float(G["lta_parent__crc"]) == int(G["lta_parent__crc"]) and os.path.getsize(MC.GOLDEN) < (1 << 20)


def test_new_symbols_are_declared_exported_and_prototyped():
    from xmh import _lib
    header = open(os.path.join(ROOT, "include", "xmh.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.PROTOTYPES and getattr(_lib.lib, name).argtypes == _lib.PROTOTYPES[name][1]
    for struct in ("xmh_mith_train", "xmh_mith_mlp_grads", "xmh_mith_grads"):
        assert "} %s;" % struct in header
    assert ctypes.sizeof(_lib.MithTrain) == ctypes.sizeof(_lib.MithHead) + ctypes.sizeof(_lib.Linear)
    assert ctypes.sizeof(_lib.MithGrads) == 9 * 8 and ctypes.sizeof(_lib.MithMlpGrads) == 6 * 8


def _desc(D=64, K=8, R=1, layers=1, heads=1, top_k=4, eps=1e-5):
    """a descriptor whose pointers are never dereferenced: every check below fails before a launch"""
    from xmh import _lib
    one = 256
    lin = lambda n, k, bias=one: _lib.Linear(one, None, None, bias, n, k)      # noqa: E731
    mlps = (_lib.MithMlp * max(R, 1))(*[_lib.MithMlp(one, one, eps, lin(4 * D, D), lin(D, 4 * D)) for _ in range(R)])
    blocks = (_lib.ClipBlock * max(layers, 1))(*[_lib.ClipBlock(one, one, one, one, lin(3 * D, D), lin(D, D), lin(4 * D, D), lin(D, 4 * D))
                                                 for _ in range(layers)])
    head = _lib.MithHead(D, K, top_k, R, layers, heads, mlps, lin(K, D, None), one, blocks, one, one)
    return _lib.MithTrain(head, lin(D, D)), (mlps, blocks)


def test_argument_errors_are_reported_without_a_gpu():
    from xmh import _lib
    L_ = _lib.lib
    one = ctypes.c_void_p(256)
    big = 1 << 40

    def fwd(d, B=2, L=5, cls=one, out=one, saved=one, sbytes=big, ws=one, wbytes=big):
        return L_.xmh_mith_train_forward(ctypes.byref(d[0]) if d else None, cls, one, None, B, L, one, out, one, one, saved, sbytes, ws, wbytes, None)

    def bwd(d, B=2, L=5, cls=one, saved=one, sbytes=big, grads=True, ws=one, wbytes=big, R=1, layers=1):
        mg, bg = (_lib.MithMlpGrads * max(R, 1))(), (_lib.ClipBlockGrads * max(layers, 1))()
        g = _lib.MithGrads(mg, None, bg, None, None, None, None, one, one)
        return L_.xmh_mith_train_backward(ctypes.byref(d[0]) if d else None, cls, B, L, one, one, one, one, saved, sbytes,
                                          ctypes.byref(g) if grads else None, 0, ws, wbytes, None)
    ok = _desc()
    for fn, name in ((fwd, b"xmh_mith_train_forward"), (bwd, b"xmh_mith_train_backward")):
        assert fn(None) == -22 and name in L_.xmh_last_error()                   # null pointers
        assert fn(ok, cls=None) == -22 and fn(ok, ws=None) == -22 and fn(ok, B=-1) == -22
        assert fn(ok, B=0) == 0
        assert fn(_desc(K=129, top_k=8)) == -95 and b"> 128" in L_.xmh_last_error()      # beyond the block stack's limits
        assert fn(_desc(D=66, heads=1)) == -95 and fn(_desc(D=1088, heads=17)) == -95 and fn(_desc(D=128, heads=1)) == -95
        assert fn(_desc(R=5)) == -95 and fn(_desc(eps=1e-6)) == -95
        assert fn(_desc(top_k=9)) == -22 and fn(_desc(top_k=0)) == -22 and fn(ok, L=0) == -22      # misfitting
        assert fn(ok, sbytes=16) == -12 and b"saved" in L_.xmh_last_error()      # short buffers
        assert fn(ok, wbytes=16) == -12 and b"workspace" in L_.xmh_last_error()
    assert fwd(ok, out=None) == -22 and bwd(ok, saved=None) == -22 and bwd(ok, grads=False) == -22
    assert fwd(ok, saved=None, sbytes=0, wbytes=16) == -12                       # a forward without a record still needs its workspace
    # the size helpers answer for the limits, and agree with what the entry points ask for
    saved, ws = L_.xmh_mith_train_saved_bytes(2, 5, 64, 8, 1, 1), L_.xmh_mith_train_ws_bytes(2, 5, 64, 8, 1)
    assert saved % 256 == 0 and ws % 256 == 0 and saved >= 16 * 2 * 8 * 64 * 4 and ws > 0
    assert fwd(ok, sbytes=saved - 1) == -12 and fwd(ok, wbytes=ws - 1) == -12 and bwd(ok, sbytes=saved - 1) == -12 and bwd(ok, wbytes=ws - 1) == -12
    assert L_.xmh_mith_train_saved_bytes(2, 5, 64, 129, 1, 1) == 0 and L_.xmh_mith_train_ws_bytes(2, 5, 66, 8, 1) == 0
    assert L_.xmh_mith_train_ws_bytes(0, 5, 64, 8, 1) == 0 and L_.xmh_mith_train_saved_bytes(2, 5, 1088, 8, 1, 1) == 0
    last = (0, 0)
    for B in (1, 2, 3, 64, 128):
        cur = (L_.xmh_mith_train_saved_bytes(B, 49, 512, 64, 2, 2), L_.xmh_mith_train_ws_bytes(B, 49, 512, 64, 2))
        assert cur[0] > last[0] and cur[1] > last[1]
        last = cur


def test_python_layer_refuses_what_it_cannot_run():
    import xmh.runners  # noqa: F401
    from xmh.models.clip import CLIP
    from xmh.models.mith import MITH, MITHHashLayer
    from xmh.runners.methods import MITHTrainer
    h = MITHHashLayer(64, 8, 0.0, 1, "gelu", 4, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        h.encode_img_train(torch.zeros(2, 64), torch.zeros(5, 2, 64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        h.encode_txt_train(torch.zeros(2, 64), torch.zeros(5, 2, 64), torch.zeros(2, 5, dtype=torch.bool))
    d = MITHHashLayer(64, 8, 0.1, 1, "gelu", 4, 1)
    with pytest.raises(NotImplementedError, match="dropout"):
        d.encode_img_train(torch.zeros(2, 64), torch.zeros(5, 2, 64))
    with pytest.raises(NotImplementedError, match="dropout"):
        d.encode_txt_train(torch.zeros(2, 64), torch.zeros(5, 2, 64), None)
    assert d.state_dict().keys() == h.state_dict().keys() and callable(MITH.forward_train_heads)
    # the scope boundary: these three still have no training path, and say what is missing
    with pytest.raises(NotImplementedError, match="MITH") as e:
        MITH.forward_train(types.SimpleNamespace(), None, None)
    assert "token outputs" in str(e.value) and "no backward" not in str(e.value)
    with pytest.raises(NotImplementedError, match="MITH's head") as e:
        MITHTrainer.train_epoch(types.SimpleNamespace(), 0)
    assert "forward_train_heads" in str(e.value)
    p = CLIP(16, 8, 1, 64, 4, 8, 16, 64, 1, 1, return_patches=True)
    with pytest.raises(NotImplementedError, match="MITH") as e:
        p.encode_image_train(torch.zeros(1, 3, 8, 8))
    assert "not built" not in str(e.value)
    with pytest.raises(NotImplementedError, match="MITH") as e:
        p.encode_text_train(torch.zeros(1, 8, dtype=torch.int64))
    assert "not built" not in str(e.value)


def test_head_params_follow_the_tables():
    from xmh.models import clip_train as CT
    from xmh.models import mith as M
    h = M.MITHHashLayer(64, 8, 0.0, 2, "gelu", 4, 2)
    for gcl, lct, proj in ((h.gcl_i, h.lct_i, h.img_concept_proj), (h.gcl_t, h.lct_t, h.txt_concept_proj)):
        params = M.head_params(gcl, lct, proj)
        assert len(params) == 6 * 2 + 1 + 12 * 2 + 2 * 8 + 2
        pm, concept, pb, hw, hb, pw, pbias = M._split(params, 2, 2, 8)
        assert pm[6] is gcl.mlp.lns[1].weight and pm[4] is gcl.mlp.mlps[0][3].weight and concept is gcl.common_concept_embedding.weight
        assert pb == CT.block_params(lct.transformer) and hw[3] is lct.hashing.fc_list[3].weight and hb[7] is lct.hashing.fc_list[7].bias
        assert pw is proj.weight and pbias is proj.bias
        assert {id(p) for p in params} == {id(p) for p in list(gcl.parameters()) + list(lct.parameters()) + list(proj.parameters())}
    assert len(M.head_params(M.MITHHashLayer(64, 8, 0.0, 1, "gelu", 4, 0).gcl_i, h.lct_i, h.img_concept_proj)) == 1 + 24 + 16 + 2
    assert [f for f, _ in M.MLP] == list(MC.MLP_FIELDS)
    buf = torch.arange(200000, dtype=torch.float32)
    A = M.saved_attention(buf, (2, 5, 64, 8, 1, 1))                              # behind the block record, the MLP's four pieces and two [B, K]
    assert A.shape == (2, 8, 5) and int(A[0, 0, 0]) == 16 * 2 * 8 * 64 + (2 * 128 + 2 * 512) + 2 * 64
