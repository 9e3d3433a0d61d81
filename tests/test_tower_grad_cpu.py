"""No GPU: the golden file of the two CLIP towers' backward (tools/make_golden_tower_grad.py: the reference's own fp32 gradients) against
the restatement of tests/tower_grad_cases.py -- its fp32 run regenerates the stored tensors to the bit, its fp64 run the stored
e_ref -- the binding of the new C entry points, and what of the Python layer can be seen without a device."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import tower_grad_cases as TC


@pytest.mark.parametrize("case", list(TC.CASES))
def test_restatement_regenerates_the_golden(case):
    G = TC.golden()
    tower = TC.tower_of(case)
    sd, x, up, kpm = TC.case_inputs(case)
    assert int(G[case + "__seed"]) == TC.case_seed(case)
    assert TC.inputs_checksum(sd, x, up, kpm) == float(G[case + "__checksum"])
    r32 = TC.run_restatement(tower, sd, x, up, kpm, torch.float32)
    r64 = TC.run_restatement(tower, sd, x, up, kpm, torch.float64)
    per, _ = TC.erefs(r32, r64)
    assert sorted(r32) == sorted(TC.tensor_names(tower, TC.count_layers(tower, sd)))
    for k in r32:
        assert r32[k].dtype == np.float32 and r64[k].dtype == np.float64 and np.isfinite(r64[k]).all()
        assert np.array_equal(G["%s__%s" % (case, k)], TC.thin(r32[k])), k
        assert float(G["%s__eref_%s" % (case, k)]) == per[k], k
        assert 0.0 < per[k] < 1e-5, (k, per[k])                    # an fp32 computation of this tower


@pytest.mark.parametrize("case", list(TC.TXT_CASES))
def test_text_cases_hold_what_the_token_gradient_needs(case):
    vocab, context, D, layers, out_dim, L, B, kp = TC.TXT_CASES[case]
    sd, ids, up, kpm = TC.case_inputs(case)
    assert ids.shape == (B, L) and ids.dtype == np.int64 and ids.min() >= 0 and ids.max() == vocab - 1
    eos = ids.argmax(1)
    assert ((ids == vocab - 1).sum(1) == 1).all()                  # EOS once per caption
    assert L - 1 in eos and (B == 1 or 0 in eos)
    for b in range(B):
        assert not ids[b, eos[b] + 1:].any() and (ids[b, :eos[b]] > 0).all()      # padding behind, drawn ids before
    if kpm is not None:
        assert not kpm[:, 0].any() and kpm.any()                   # every query keeps a visible key
    r64 = TC.run_restatement("txt", sd, ids, up, kpm, torch.float64)
    absent = np.setdiff1d(np.arange(vocab), np.unique(ids))
    assert not r64["g_tok"][absent].any() and not r64["g_pos"][L:].any()
    if case == "txt_v11_c40_d64_b5_kpm":
        counts = np.bincount(ids.reshape(-1), minlength=vocab)
        assert (counts[:-1] > 1).all() and any(np.unique(row).size < np.count_nonzero(row) for row in ids)      # across and within rows
    if case == "txt_v64_c16_d64_b3":
        assert L < context


def test_every_kind_has_a_pool_and_the_file_holds_small_arrays_only():
    for tower in ("img", "txt"):
        for kind in TC.KINDS[tower]:
            assert 1e-8 < TC.pool_eref(tower, kind) < 1e-5, (tower, kind)
    assert os.path.getsize(TC.GOLDEN) < 1 << 20
    with np.load(TC.GOLDEN, allow_pickle=False) as z:
        assert all(z[k].dtype in (np.float32, np.float64, np.int64) for k in z.files)


def test_symbols_and_structs_are_bound():
    from xmh import _lib
    assert ctypes.sizeof(_lib.VitGrads) == 9 * ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(_lib.TextGrads) == 6 * ctypes.sizeof(ctypes.c_void_p)
    assert [n for n, _ in _lib.VitGrads._fields_][:8] == [k for k, _ in TC.IMG_OWN]
    assert [n for n, _ in _lib.TextGrads._fields_][:5] == ["proj"] + [k for k, _ in TC.TXT_OWN[1:]]
    for name in ("xmh_vit_train_forward", "xmh_vit_backward", "xmh_text_train_forward", "xmh_text_backward", "xmh_vit_train_saved_bytes",
                 "xmh_vit_train_ws_bytes", "xmh_text_train_saved_bytes", "xmh_text_train_ws_bytes"):
        assert name in _lib.PROTOTYPES and getattr(_lib.lib, name).argtypes == _lib.PROTOTYPES[name][1]
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "xmh.h")).read()
    for name, n_args in (("xmh_vit_train_forward", 9), ("xmh_vit_backward", 11), ("xmh_text_train_forward", 12), ("xmh_text_backward", 14),
                         ("xmh_vit_train_saved_bytes", 4), ("xmh_vit_train_ws_bytes", 5), ("xmh_text_train_saved_bytes", 4),
                         ("xmh_text_train_ws_bytes", 4)):
        decl = header.split(name + "(", 1)[1].split(");", 1)[0]
        assert decl.count(",") + 1 == n_args == len(_lib.PROTOTYPES[name][1]), name


def test_sizes():
    from xmh._lib import lib
    vs, vw = lib.xmh_vit_train_saved_bytes, lib.xmh_vit_train_ws_bytes
    ts, tw = lib.xmh_text_train_saved_bytes, lib.xmh_text_train_ws_bytes
    assert vs(0, 50, 768, 12) == 0 and vw(4, 50, 768, 0, 512) == 0 and ts(4, 0, 512, 12) == 0 and tw(4, 32, 512, 0) == 0
    assert vs(4, 129, 768, 1) == 0 and tw(4, 129, 512, 512) == 0 and vs(4, 50, 1028, 1) == 0 and ts(4, 32, 510, 1) == 0      # outside the limits
    last = 0
    for B in (1, 2, 41, 128):
        n = vs(B, 50, 768, 12)
        assert n % 256 == 0 and n >= lib.xmh_clip_saved_bytes(B, 50, 768, 12) + (B * 50 + B) * 768 * 4 and n >= last
        last = n
        assert ts(B, 32, 512, 12) >= lib.xmh_clip_saved_bytes(B, 32, 512, 12) + B * 512 * 4
        assert vw(B, 50, 768, 3072, 512) >= lib.xmh_clip_blocks_backward_ws_bytes(B, 50, 768) + B * 49 * 3072 * 4
        assert tw(B, 32, 512, 512) >= lib.xmh_clip_blocks_backward_ws_bytes(B, 32, 512)
    assert vs(2, 5, 64, 0) > 0                                       # a tower without blocks keeps its rows all the same


# (B, L, D) -> what the six size functions returned before the scratch sizing, the limit checks and the entry points' prologue were
# shared (recorded from that library): saved bytes for layers 0, 1, 12; workspaces for conv_k in (48, 3072) x out_dim in (16, 512)
RECORDED_SIZES = {
    (1, 5, 64): dict(vit_saved=(1536, 22016, 247296), text_saved=(256, 20736, 246016), clip_saved=(0, 20480, 245760),
                     vit_ws=(186624, 186624, 235008, 235008), text_ws=(183552, 183552), blocks_ws=104960),
    (2, 17, 128): dict(vit_saved=(18432, 296960, 3360768), text_saved=(1024, 279552, 3343360), clip_saved=(0, 278528, 3342336),
                       vit_ws=(510464, 510464, 897536, 897536), text_ws=(470528, 470528), blocks_ws=284416),
    (41, 50, 64): dict(vit_saved=(535296, 8932096, 101296896), text_saved=(10496, 8407296, 100772096), clip_saved=(0, 8396800, 100761600),
                       vit_ws=(7630848, 7630848, 40385792, 40385792), text_ws=(6009344, 6009344), blocks_ws=3607296),
    (128, 50, 768): dict(vit_saved=(20054016, 334626816, 3794927616), text_saved=(393216, 314966016, 3775266816),
                         clip_saved=(0, 314572800, 3774873600), vit_ws=(264172800, 264959232, 337777920, 340825344),
                         text_ws=(221779200, 224826624), blocks_ws=113741824),
    (128, 77, 512): dict(vit_saved=(20447232, 343408640, 3895984128), text_saved=(262144, 323223552, 3875799040),
                         clip_saved=(0, 322961408, 3875536896), vit_ws=(270167296, 270691584, 398847232, 398847232),
                         text_ws=(226684160, 228715776), blocks_ws=111306752),
}


def test_sizes_are_the_recorded_ones():
    from xmh._lib import lib
    for s, want in RECORDED_SIZES.items():
        got = dict(vit_saved=tuple(lib.xmh_vit_train_saved_bytes(*s, n) for n in (0, 1, 12)),
                   text_saved=tuple(lib.xmh_text_train_saved_bytes(*s, n) for n in (0, 1, 12)),
                   clip_saved=tuple(lib.xmh_clip_saved_bytes(*s, n) for n in (0, 1, 12)),
                   vit_ws=tuple(lib.xmh_vit_train_ws_bytes(*s, k, o) for k in (48, 3072) for o in (16, 512)),
                   text_ws=tuple(lib.xmh_text_train_ws_bytes(*s, o) for o in (16, 512)),
                   blocks_ws=lib.xmh_clip_blocks_backward_ws_bytes(*s))
        assert got == want, s
    vs, vw, ts, tw = lib.xmh_vit_train_saved_bytes, lib.xmh_vit_train_ws_bytes, lib.xmh_text_train_saved_bytes, lib.xmh_text_train_ws_bytes
    zeros = [vs(0, 50, 768, 12), vw(4, 50, 768, 0, 512), ts(4, 0, 512, 12), tw(4, 32, 512, 0), vs(4, 129, 768, 1), tw(4, 129, 512, 512),
             vs(4, 50, 1028, 1), ts(4, 32, 510, 1), vw(2, 129, 64, 48, 16), ts(2, 8, 66, 1), lib.xmh_clip_blocks_backward_ws_bytes(4, 129, 512),
             lib.xmh_clip_blocks_backward_ws_bytes(0, 32, 512), lib.xmh_clip_blocks_backward_ws_bytes(4, 32, 510)]
    assert zeros == [0] * len(zeros)


def test_tables_state_the_parameter_order_once():
    import block_grad_cases as BC
    from xmh import _lib
    from xmh.models import clip_train as CT
    from xmh.models.clip import CLIP
    fields = lambda struct: [n for n, _ in struct._fields_ if n != "blocks"]      # noqa: E731
    for table, struct in ((CT.BLOCK, _lib.ClipBlockGrads), (CT.VIT, _lib.VitGrads), (CT.TEXT, _lib.TextGrads)):
        assert [name for name, _ in table] == fields(struct)
    assert CT.BLOCK == BC.PARAMS                                    # the cases' names are the table's
    m = CLIP(16, 8, 1, 64, 4, 8, 16, 64, 1, 1)
    blk = m.transformer.resblocks[0]
    for module, table in ((blk, CT.BLOCK), (m.visual, CT.VIT), (m, CT.TEXT)):
        assert all(isinstance(module.get_parameter(path), torch.nn.Parameter) for _, path in table)
    img = CT.tower_params(m.visual, CT.VIT)
    txt = CT.tower_params(m, CT.TEXT)
    assert len(img) == len(CT.VIT) + len(CT.BLOCK) and len(txt) == len(CT.TEXT) + len(CT.BLOCK)
    assert [id(p) for p in CT.block_params(m.transformer)] == [id(blk.get_parameter(path)) for _, path in CT.BLOCK]
    assert [id(p) for p in m.transformer._train_params(blk)] == [id(p) for p in CT.block_params(m.transformer)]
    assert sorted(map(id, img)) == sorted(id(p) for p in m.visual.parameters())                   # each exactly once
    mine = set(map(id, img))
    assert sorted(map(id, txt)) == sorted(id(p) for p in m.parameters() if id(p) not in mine and p is not m.logit_scale)


def test_argument_errors_without_a_gpu():
    from xmh import _lib
    L = _lib.lib
    one = ctypes.c_void_p(256)                                      # never dereferenced: every check below fails before a launch
    big = 1 << 40
    blocks = (_lib.ClipBlock * 1)()
    lin = lambda n, k: _lib.Linear(256, None, None, None, n, k)     # noqa: E731

    def vit(width=128, heads=2, res=32, patch=8, out=16, conv=None, proj=None):
        return _lib.VitWeights(res, patch, width, heads, 1, out, conv or lin(width, 3 * patch * patch), 256, 256, 256, 256, 256, 256,
                               proj or lin(out, width), blocks)

    def fwd(w, image=one, B=2, y=one, saved=one, sbytes=big, ws=one, wbytes=big):
        return L.xmh_vit_train_forward(ctypes.byref(w), image, B, y, saved, sbytes, ws, wbytes, None)
    assert fwd(vit(), image=None) == -22 and b"xmh_vit_train_forward" in L.xmh_last_error()
    assert fwd(vit(), y=None) == -22 and fwd(vit(), saved=None) == -22 and fwd(vit(), ws=None) == -22 and fwd(vit(), B=-1) == -22
    assert fwd(vit(res=30)) == -22 and fwd(vit(heads=3)) == -22 and fwd(vit(conv=lin(128, 100))) == -22 and fwd(vit(proj=lin(16, 64))) == -22
    assert fwd(vit(heads=1)) == -95 and fwd(vit(width=1088, heads=17)) == -95 and fwd(vit(res=96)) == -95      # head dim, width, L = 145
    assert fwd(vit(res=36, patch=6)) == -95
    assert fwd(vit(), sbytes=L.xmh_vit_train_saved_bytes(2, 17, 128, 1) - 1) == -12 and b"saved" in L.xmh_last_error()
    assert fwd(vit(), sbytes=L.xmh_vit_train_saved_bytes(2, 17, 128, 1), wbytes=L.xmh_vit_train_ws_bytes(2, 17, 128, 192, 16) - 1) == -12
    assert fwd(vit(), B=0, image=None) == 0

    grads = _lib.VitGrads(*([256] * 8), (_lib.ClipBlockGrads * 1)())
    none = _lib.VitGrads(*([256] * 8), None)

    def bwd(w, g=one, gr=grads, saved=one, sbytes=big, ws=one, wbytes=big):
        return L.xmh_vit_backward(ctypes.byref(w), one, 2, saved, sbytes, g, ctypes.byref(gr) if gr is not None else None, 0, ws, wbytes, None)
    assert bwd(vit(), g=None) == -22 and bwd(vit(), gr=None) == -22 and bwd(vit(), gr=none) == -22 and bwd(vit(), saved=None) == -22
    assert bwd(vit(), sbytes=16) == -12 and bwd(vit(), wbytes=16) == -12 and bwd(vit(heads=1)) == -95

    def text(width=128, heads=2, vocab=50, context=8, out=16):
        return _lib.TextWeights(vocab, context, width, heads, 1, out, 256, 256, 256, 256, lin(out, width), blocks)

    def tfwd(w, Lq=8, ids=one, y=one, eos=one, sbytes=big, wbytes=big):
        return L.xmh_text_train_forward(ctypes.byref(w), ids, None, 2, Lq, y, eos, one, sbytes, one, wbytes, None)
    assert tfwd(text(), ids=None) == -22 and tfwd(text(), y=None) == -22 and tfwd(text(), eos=None) == -22
    assert tfwd(text(), Lq=9) == -22 and b"positional" in L.xmh_last_error() and tfwd(text(), Lq=0) == -22
    assert tfwd(text(heads=4)) == -95 and tfwd(text(context=200), Lq=129) == -95
    assert tfwd(text(), sbytes=16) == -12 and tfwd(text(), wbytes=16) == -12
    tg = _lib.TextGrads(*([256] * 5), (_lib.ClipBlockGrads * 1)())
    tb = lambda w, Lq=8, eos=one, g=one, sbytes=big: L.xmh_text_backward(ctypes.byref(w), one, None, eos, 2, Lq, one, sbytes, g,       # noqa: E731
                                                                        ctypes.byref(tg), 0, one, big, None)
    assert tb(text(), eos=None) == -22 and tb(text(), g=None) == -22 and tb(text(), Lq=9) == -22 and tb(text(), sbytes=16) == -12


def test_python_layer_without_a_gpu(tmp_path):
    import xmh.runners  # noqa: F401
    from xmh.models.base import BaseModel
    from xmh.models.clip import CLIP
    from xmh.models.mith import MITH
    from xmh.models.twdh import TwDH
    from xmh.runners.base import BaseTrainer
    from xmh.runners.methods import DCMHTTrainer, DSPHTrainer, MITHTrainer, TwDHTrainer
    m = CLIP(16, 8, 1, 64, 4, 8, 16, 64, 1, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.encode_image_train(torch.zeros(1, 3, 8, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.encode_text_train(torch.zeros(1, 8, dtype=torch.int64))
    with pytest.raises(NotImplementedError, match="MITH"):
        CLIP(16, 8, 1, 64, 4, 8, 16, 64, 1, 1, return_patches=True).encode_image_train(torch.zeros(1, 3, 8, 8))
    assert callable(BaseModel.forward_train)
    for cls, word in ((MITH, "MITH"), (TwDH, "TwDH")):
        assert cls.forward_train is not BaseModel.forward_train
        with pytest.raises(NotImplementedError, match=word):
            cls.forward_train(types.SimpleNamespace(), None, None)
    with pytest.raises(NotImplementedError, match="towers"):
        BaseTrainer.train_epoch(types.SimpleNamespace(), 0)
    for cls, word in ((MITHTrainer, "MITH's head"), (TwDHTrainer, "TwDH's head")):
        with pytest.raises(NotImplementedError, match=word):
            cls.train_epoch(types.SimpleNamespace(), 0)
    assert "train_epoch" in vars(DCMHTTrainer) and "train_epoch" in vars(DSPHTrainer) and "train_epoch" in vars(TwDHTrainer)
    assert DCMHTTrainer.train_epoch is not BaseTrainer.train_epoch
    with pytest.raises(NotImplementedError, match="all-reduce"):
        DCMHTTrainer.train_epoch(types.SimpleNamespace(distributed=True), 0)
