"""No GPU: the golden file of the two CLIP towers trained through their token outputs (tools/make_golden_tower_tokens.py: the
reference's own fp32 outputs and gradients) against the float64 restatement of tests/tower_tokens_cases.py, the binding of the new C
entry points and their argument checks, and what of the Python layer can be seen without a device."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import tower_tokens_cases as TT


@pytest.mark.parametrize("case", list(TT.CASES))
def test_restatement_reproduces_the_golden_within_its_own_error(case):
    G = TT.golden()
    tower = TT.tower_of(case)
    sd, x, ups, kpm = TT.case_inputs(case)
    assert int(G[case + "__seed"]) == TT.case_seed(case)
    assert TT.inputs_checksum(sd, x, ups, kpm) == float(G[case + "__checksum"])
    r64 = TT.run_restatement(tower, sd, x, ups, kpm, torch.float64)
    assert sorted(r64) == sorted(TT.tensor_names(tower, TT.count_layers(tower, sd)))
    for k in r64:
        stored, eref = G["%s__%s" % (case, k)], float(G["%s__eref_%s" % (case, k)])
        assert stored.dtype == np.float32 and r64[k].dtype == np.float64 and np.isfinite(r64[k]).all()
        assert 0.0 < eref < 1e-5, (k, eref)                          # an fp32 computation of this tower
        # e_ref is the largest deviation over the WHOLE tensor, so the stored (thinned) elements lie within it
        assert np.abs(stored.astype(np.float64) - TT.thin(r64[k])).max() <= eref * np.abs(r64[k]).max() * (1 + 1e-12), k      # (the product rounds)
    if tower == "txt":
        vocab, L = sd["token_embedding.weight"].shape[0], x.shape[1]
        absent = np.setdiff1d(np.arange(vocab), np.unique(x))
        assert not r64["g_tok"][absent].any() and not r64["g_pos"][L:].any()


def test_cases_are_the_ones_the_back_end_can_go_wrong_at():
    rows = {name: ((s[0] // s[1]) ** 2 + 1) * s[5] for name, s in TT.IMG_CASES.items()}
    rows.update({name: s[5] * s[6] for name, s in TT.TXT_CASES.items()})
    assert sorted(rows.values()) == [1, 5, 10, 21, 51, 165, 250, 2050, 4160]
    assert rows["img_r8_p4_d64_b1"] % 4 and rows["txt_v97_c64_d64_l64_b65"] > 64 * 64 and TT.IMG_CASES["img_r64_p32_d64_b2"][4] % 32
    sd, ids, ups, kpm = TT.case_inputs("txt_v11_c40_d64_b5_kpm")
    eos = ids.argmax(1)
    assert 0 in eos and ids.shape[1] - 1 in eos and kpm is not None and ups[1].shape == (33, 5, 32) and ups[0].shape == (5, 32)
    for a, b in zip(TT.case_inputs("img_r28_p4_d64_b5")[2], TT.case_inputs("img_r28_p4_d64_b5")[2]):
        assert np.array_equal(a, b)                                  # seeded


def test_every_kind_has_a_pool_and_the_file_holds_small_arrays_only():
    import tower_grad_cases as TG
    for tower in ("img", "txt"):
        for kind in TT.KINDS[tower]:
            assert 1e-8 < TT.pool_eref(tower, kind) < 1e-5, (tower, kind)
    assert os.path.getsize(TT.GOLDEN) <= os.path.getsize(TG.GOLDEN)
    with np.load(TT.GOLDEN, allow_pickle=False) as z:
        assert all(z[k].dtype in (np.float32, np.float64, np.int64) for k in z.files)
        assert all(z[c + "__bit_equal"] in (0, 1) for c in TT.CASES)


NEW = (("xmh_vit_train_forward_tokens", 10), ("xmh_vit_backward_tokens", 12), ("xmh_text_train_forward_tokens", 13),
       ("xmh_text_backward_tokens", 15), ("xmh_vit_train_tokens_saved_bytes", 4), ("xmh_vit_train_tokens_ws_bytes", 5),
       ("xmh_text_train_tokens_saved_bytes", 4), ("xmh_text_train_tokens_ws_bytes", 4))


def test_symbols_are_declared_and_bound():
    from xmh import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "xmh.h")).read()
    for name, n_args in NEW:
        assert name in _lib.PROTOTYPES and getattr(_lib.lib, name).argtypes == _lib.PROTOTYPES[name][1]
        decl = header.split(name + "(", 1)[1].split(");", 1)[0]
        assert decl.count(",") + 1 == n_args == len(_lib.PROTOTYPES[name][1]), name


def test_sizes():
    from xmh._lib import lib
    vs, vw = lib.xmh_vit_train_tokens_saved_bytes, lib.xmh_vit_train_tokens_ws_bytes
    ts, tw = lib.xmh_text_train_tokens_saved_bytes, lib.xmh_text_train_tokens_ws_bytes
    zeros = [vs(0, 50, 768, 12), vw(4, 50, 768, 0, 512), ts(4, 0, 512, 12), tw(4, 32, 512, 0), vs(4, 129, 768, 1), tw(4, 129, 512, 512),
             vs(4, 50, 1028, 1), ts(4, 32, 510, 1), vw(2, 129, 64, 48, 16), ts(2, 8, 66, 1), vw(4, 1, 64, 48, 16), vs(1 << 21, 2, 64, 1)]
    assert zeros == [0] * len(zeros)                                 # outside the limits, as the B-row size functions answer
    for B in (1, 2, 41, 128):
        M = B * 50
        n = vs(B, 50, 768, 12)                                       # the record, the rows in front of ln_pre and ALL rows in front of ln_post
        assert n % 256 == 0 and n >= lib.xmh_clip_saved_bytes(B, 50, 768, 12) + 2 * M * 768 * 4
        assert n - lib.xmh_vit_train_saved_bytes(B, 50, 768, 12) >= (M - B) * 768 * 4 - 256
        assert ts(B, 32, 512, 12) >= lib.xmh_clip_saved_bytes(B, 32, 512, 12) + B * 32 * 512 * 4
        # against the B-row workspace: LN(rows) and its gradient over M rows instead of B, the M projected rows, no [B, D] row buffer
        assert vw(B, 50, 768, 3072, 512) - lib.xmh_vit_train_ws_bytes(B, 50, 768, 3072, 512) >= (2 * (M - B) * 768 - B * 768 + M * 512) * 4 - 1024
        assert tw(B, 32, 512, 512) - lib.xmh_text_train_ws_bytes(B, 32, 512, 512) >= (2 * (B * 32 - B) * 512 - B * 512 + B * 32 * 512) * 4 - 1024


def test_argument_errors_without_a_gpu():
    from xmh import _lib
    L = _lib.lib
    one = ctypes.c_void_p(256)                                      # never dereferenced: every check below fails before a launch
    big = 1 << 40
    blocks = (_lib.ClipBlock * 1)()
    lin = lambda n, k: _lib.Linear(256, None, None, None, n, k)     # noqa: E731

    def vit(width=128, heads=2, res=32, patch=8, out=16):
        return _lib.VitWeights(res, patch, width, heads, 1, out, lin(width, 3 * patch * patch), 256, 256, 256, 256, 256, 256, lin(out, width), blocks)

    def fwd(w, image=one, B=2, y=one, tok=one, saved=one, sbytes=big, ws=one, wbytes=big):
        return L.xmh_vit_train_forward_tokens(ctypes.byref(w), image, B, y, tok, saved, sbytes, ws, wbytes, None)
    assert fwd(vit(), image=None) == -22 and b"xmh_vit_train_forward_tokens" in L.xmh_last_error()
    assert fwd(vit(), y=None) == -22 and fwd(vit(), tok=None) == -22 and fwd(vit(), saved=None) == -22 and fwd(vit(), B=-1) == -22
    assert fwd(vit(res=30)) == -22 and fwd(vit(heads=1)) == -95 and fwd(vit(res=96)) == -95
    assert fwd(vit(), sbytes=L.xmh_vit_train_tokens_saved_bytes(2, 17, 128, 1) - 1) == -12 and b"saved" in L.xmh_last_error()
    assert fwd(vit(), sbytes=L.xmh_vit_train_saved_bytes(2, 17, 128, 1)) == -12          # the B-row record is too small
    assert fwd(vit(), wbytes=L.xmh_vit_train_tokens_ws_bytes(2, 17, 128, 192, 16) - 1) == -12 and b"workspace" in L.xmh_last_error()
    assert fwd(vit(), B=0, image=None) == 0
    grads = _lib.VitGrads(*([256] * 8), (_lib.ClipBlockGrads * 1)())

    def bwd(w, gc=one, gt=one, gr=grads, saved=one, sbytes=big, wbytes=big):
        return L.xmh_vit_backward_tokens(ctypes.byref(w), one, 2, saved, sbytes, gc, gt, ctypes.byref(gr) if gr is not None else None, 0, one, wbytes, None)
    assert bwd(vit(), gc=None, gt=None) == -22 and b"xmh_vit_backward_tokens" in L.xmh_last_error()
    assert bwd(vit(), gr=None) == -22 and bwd(vit(), saved=None) == -22 and bwd(vit(), sbytes=16) == -12 and bwd(vit(), wbytes=16) == -12

    def text(width=128, heads=2, vocab=50, context=8, out=16):
        return _lib.TextWeights(vocab, context, width, heads, 1, out, 256, 256, 256, 256, lin(out, width), blocks)

    def tfwd(w, Lq=8, ids=one, y=one, tok=one, eos=one, sbytes=big, wbytes=big):
        return L.xmh_text_train_forward_tokens(ctypes.byref(w), ids, None, 2, Lq, y, tok, eos, one, sbytes, one, wbytes, None)
    assert tfwd(text(), ids=None) == -22 and tfwd(text(), y=None) == -22 and tfwd(text(), tok=None) == -22 and tfwd(text(), eos=None) == -22
    assert tfwd(text(), Lq=9) == -22 and b"positional" in L.xmh_last_error() and tfwd(text(heads=4)) == -95
    assert tfwd(text(), sbytes=16) == -12 and tfwd(text(), wbytes=16) == -12
    tg = _lib.TextGrads(*([256] * 5), (_lib.ClipBlockGrads * 1)())
    tb = lambda w, Lq=8, eos=one, ge=one, gt=one, sbytes=big: L.xmh_text_backward_tokens(ctypes.byref(w), one, None, eos, 2, Lq, one, sbytes, ge, gt,      # noqa: E731
                                                                                         ctypes.byref(tg), 0, one, big, None)
    assert tb(text(), eos=None) == -22 and tb(text(), ge=None, gt=None) == -22 and tb(text(), Lq=9) == -22 and tb(text(), sbytes=16) == -12


def test_python_layer_without_a_gpu():
    import xmh.runners  # noqa: F401
    from xmh.models import clip_train as CT
    from xmh.models.clip import CLIP
    from xmh.models.mith import MITH
    from xmh.runners import methods
    from xmh.runners.methods import MITHTrainer
    for rp in (False, True):                                        # the new methods do not look at return_patches
        m = CLIP(16, 8, 1, 64, 4, 8, 16, 64, 1, 1, return_patches=rp)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m.encode_image_train_tokens(torch.zeros(1, 3, 8, 8))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m.encode_text_train_tokens(torch.zeros(1, 8, dtype=torch.int64))
    for fn in (CT._VitTokensTrain, CT._TextTokensTrain):
        assert issubclass(fn, torch.autograd.Function)
    assert callable(MITH.forward_train_towers) and callable(MITH.forward_train_heads) and callable(MITHTrainer.train_epoch_towers)
    assert "train" in vars(MITHTrainer)                             # train() runs train_epoch_towers
    with pytest.raises(NotImplementedError, match="all-reduce"):
        MITHTrainer.train_epoch_towers(types.SimpleNamespace(distributed=True), 0)
    with pytest.raises(NotImplementedError, match="train_epoch_towers"):
        MITHTrainer.train_epoch(types.SimpleNamespace(), 0)
    with pytest.raises(NotImplementedError, match="forward_train_towers"):
        MITH.forward_train(types.SimpleNamespace(), None, None)
    p = CLIP(16, 8, 1, 64, 4, 8, 16, 64, 1, 1, return_patches=True)
    with pytest.raises(NotImplementedError, match="encode_image_train_tokens"):
        p.encode_image_train(torch.zeros(1, 3, 8, 8))
    with pytest.raises(NotImplementedError, match="encode_text_train_tokens"):
        p.encode_text_train(torch.zeros(1, 8, dtype=torch.int64))
    assert len(CT.VIT) == 8 and len(CT.TEXT) == 5 and len(CT.BLOCK) == 12      # no parameter-table entries were added
    import inspect
    assert "step" in inspect.signature(methods._train_epoch).parameters         # one loop, a per-batch hook
