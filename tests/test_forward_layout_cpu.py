"""The host side of the encoder entry points (csrc/xmh_forward.hip, csrc/xmh_block_grad.hip) as far as the library answers without a
GPU: the workspace and record sizes of every carve, and the return code and xmh_last_error() text of every refusal that comes before
the first launch or stream use.  The values were recorded from the library before the block chain, the record layout and the text
towers' checks were each reduced to one statement: Python restates neither the workspace layout nor the C error texts, so a carve that
moved or a check that changed place shows up here.  No call below gets a device pointer; the host addresses it passes are compared
against null and never read."""
import ctypes

import pytest

PARITY, FAST, EXACT = 0, 1, 2

# (B, L, width, conv_k, out_dim) -> xmh_clip_workspace_bytes in parity, fast and exact mode
WORKSPACE = [
    ((2, 50, 768, 3072, 0), (4590080, 3066368, 4590080)),            # image tower, cls only
    ((2, 50, 768, 3072, 512), (4897280, 3373568, 4897280)),          # ... and every token
    ((100, 50, 768, 3072, 0), (229479424, 153293824, 229479424)),
    ((100, 50, 768, 3072, 512), (244839424, 168653824, 244839424)),
    ((2, 32, 512, 0, 0), (1319424, 926208, 1319424)),                # text tower, EOS only
    ((2, 32, 512, 0, 512), (1450496, 1057280, 1450496)),
    ((100, 32, 512, 0, 0), (65946624, 46285824, 65946624)),
    ((100, 32, 512, 0, 512), (72500224, 52839424, 72500224)),
    ((3, 5, 64, 0, 0), (40960, 29184, 40448)),                       # a 64-wide toy
    ((3, 5, 64, 48, 64), (50176, 38400, 49664)),
    ((0, 50, 768, 3072, 0), (0, 0, 0)),
    ((0, 32, 512, 0, 512), (0, 0, 0)),
    ((2, 0, 512, 0, 0), (0, 0, 0)),
    ((2, 32, 0, 0, 0), (0, 0, 0)),
]

# (B, L, width, layers) -> xmh_clip_saved_bytes
SAVED = [((2, 50, 768, 12), 12 * 16 * 2 * 50 * 768 * 4), ((3, 5, 64, 2), 2 * 16 * 3 * 5 * 64 * 4), ((100, 32, 512, 12), 12 * 16 * 100 * 32 * 512 * 4),
         ((0, 50, 768, 12), 0), ((2, 0, 768, 12), 0), ((2, 50, 0, 12), 0), ((2, 50, 768, 0), 0)]

# (B, L, width) -> xmh_clip_blocks_backward_ws_bytes
BACKWARD_WS = [((2, 50, 768), 16873216), ((3, 5, 64), 117760), ((100, 32, 512), 43042816),
               ((0, 50, 768), 0), ((2, 129, 768), 0), ((2, 50, 766), 0)]        # no batch; L > 128; width % 4

# (B, E) -> xmh_head_workspace_bytes in parity, fast and exact mode
HEAD_WS = [((2, 512), (28672, 26624, 24576)), ((100, 512), (1433600, 1331200, 1228800)), ((3, 64), (5632, 5120, 4608)),
           ((0, 512), (0, 0, 0)), ((2, 0), (0, 0, 0))]

# (B, L, width, k_bits) -> xmh_head_mith_workspace_bytes in parity, fast and exact mode
MITH_WS = [((2, 50, 512, 64), (3879936, 2581504, 3900416)), ((100, 32, 512, 128), (303308800, 208281600, 304332800)),
           ((3, 5, 64, 16), (147968, 101376, 151552)), ((0, 50, 512, 64), (0, 0, 0)), ((2, 50, 512, 0), (0, 0, 0))]


@pytest.fixture(scope="module")
def L():
    from xmh import _lib
    return _lib


def test_workspace_and_record_sizes(L):
    lib = L.lib
    for args, want in WORKSPACE:
        assert tuple(int(lib.xmh_clip_workspace_bytes(*args, p)) for p in (PARITY, FAST, EXACT)) == want, args
    for args, want in SAVED:
        assert int(lib.xmh_clip_saved_bytes(*args)) == want, args
    for args, want in BACKWARD_WS:
        assert int(lib.xmh_clip_blocks_backward_ws_bytes(*args)) == want, args
    for args, want in HEAD_WS:
        assert tuple(int(lib.xmh_head_workspace_bytes(*args, p)) for p in (PARITY, FAST, EXACT)) == want, args
    for args, want in MITH_WS:
        assert tuple(int(lib.xmh_head_mith_workspace_bytes(*args, p)) for p in (PARITY, FAST, EXACT)) == want, args


_host = ctypes.create_string_buffer(64)
H = ctypes.addressof(_host)                    # a non-null address: no call below gets far enough to read or write it
BIG = 1 << 30


def _fitting_block(L, D):
    """one block whose layer shapes fit width D and whose weight pointers are all null"""
    lin = L.Linear
    arr = (L.ClipBlock * 1)()
    arr[0] = L.ClipBlock(None, None, None, None, lin(None, None, None, None, 3 * D, D), lin(None, None, None, None, D, D),
                         lin(None, None, None, None, 4 * D, D), lin(None, None, None, None, D, 4 * D))
    return arr


def _vit(L, heads=12, shapes=True):
    w = L.VitWeights()
    w.resolution, w.patch, w.width, w.heads, w.layers, w.out_dim = 224, 32, 768, heads, 12, 512
    if shapes:
        w.conv1.n, w.conv1.k, w.proj.n, w.proj.k = 768, 3072, 512, 768
    return ctypes.byref(w)


def _text(L, heads=8):
    w = L.TextWeights()
    w.vocab, w.context, w.width, w.heads, w.layers, w.out_dim = 49408, 77, 512, heads, 12, 512
    w.proj.n, w.proj.k = 512, 512
    return ctypes.byref(w)


def _dcmht(L, bits2):
    h = L.DcmhtHead()
    h.v_proj.n = h.v_proj.k = h.out_proj.n = h.out_proj.k = h.fc2.k = 512
    h.fc2.n = bits2
    return ctypes.byref(h)


def _mith(L):
    h = L.MithHead()
    h.width, h.k_bits, h.top_k, h.res_layers, h.layers, h.heads = 512, 64, 4, 2, 2, 8
    h.concept.n, h.concept.k = 64, 512
    return ctypes.byref(h)


def _calls(L):
    """name -> the refused (or empty) call.  Signatures: include/xmh.h."""
    lib = L.lib
    blk0, fit = (L.ClipBlock * 1)(), _fitting_block(L, 64)
    grads = (L.ClipBlockGrads * 1)()
    fwd, sav, bwd = lib.xmh_clip_blocks_forward, lib.xmh_clip_blocks_forward_saved, lib.xmh_clip_blocks_backward
    vit, txt, pck, dev = lib.xmh_vit_b32_forward, lib.xmh_text_forward, lib.xmh_text_forward_packed, lib.xmh_text_forward_packed_dev
    dcmht, dsph, mith = lib.xmh_head_dcmht, lib.xmh_head_dsph, lib.xmh_head_mith
    lin = L.Linear
    return {
        "blocks precision": lambda: fwd(None, 1, 64, 1, None, 1, 4, 0, None, 7, None, 0, None),
        "blocks null": lambda: fwd(None, 1, 64, 1, None, 1, 4, 0, None, PARITY, None, 0, None),
        "blocks heads": lambda: fwd(blk0, 1, 64, 3, H, 1, 4, 0, None, PARITY, H, BIG, None),
        "blocks workspace parity": lambda: fwd(blk0, 1, 64, 1, H, 3, 5, 0, None, PARITY, H, 16, None),
        "blocks workspace fast": lambda: fwd(blk0, 1, 64, 1, H, 3, 5, 0, None, FAST, H, 16, None),
        "blocks workspace exact": lambda: fwd(blk0, 1, 64, 1, H, 3, 5, 0, None, EXACT, H, 16, None),
        "blocks shapes": lambda: fwd(blk0, 1, 64, 1, H, 3, 5, 0, None, PARITY, H, BIG, None),
        "blocks shapes exact": lambda: fwd(blk0, 1, 64, 1, H, 3, 5, 0, None, EXACT, H, BIG, None),
        "blocks fp32 weights": lambda: fwd(fit, 1, 64, 1, H, 3, 5, 0, None, EXACT, H, BIG, None),
        "blocks fp16 weights": lambda: fwd(fit, 1, 64, 1, H, 3, 5, 0, None, PARITY, H, BIG, None),
        "blocks fp16 weights fast": lambda: fwd(fit, 1, 64, 1, H, 3, 5, 0, None, FAST, H, BIG, None),
        "blocks no batch": lambda: fwd(None, 1, 64, 1, None, 0, 4, 0, None, PARITY, None, 0, None),
        "blocks no layers": lambda: fwd(blk0, 0, 64, 1, H, 3, 5, 0, None, PARITY, H, BIG, None),
        "saved precision": lambda: sav(None, 1, 64, 1, None, 1, 4, 0, None, 7, None, 0, None, 0, None),
        "saved null": lambda: sav(blk0, 1, 64, 1, H, 1, 4, 0, None, PARITY, H, BIG, None, BIG, None),
        "saved width": lambda: sav(blk0, 1, 66, 1, H, 1, 4, 0, None, PARITY, H, BIG, H, BIG, None),
        "saved record": lambda: sav(blk0, 2, 64, 1, H, 3, 5, 0, None, PARITY, H, BIG, H, 16, None),
        "saved workspace": lambda: sav(blk0, 2, 64, 1, H, 3, 5, 0, None, EXACT, H, 16, H, BIG, None),
        "saved no batch": lambda: sav(None, 1, 64, 1, None, 0, 4, 0, None, PARITY, None, 0, None, 0, None),
        "saved no layers": lambda: sav(blk0, 0, 64, 1, H, 3, 5, 0, None, PARITY, H, BIG, H, 0, None),
        "backward null saved": lambda: bwd(blk0, 1, 64, 1, 3, 5, 0, None, None, BIG, H, 1, grads, 0, H, BIG, None),
        "backward record": lambda: bwd(blk0, 2, 64, 1, 3, 5, 0, None, H, 16, H, 1, grads, 0, H, BIG, None),
        "backward workspace": lambda: bwd(blk0, 1, 64, 1, 3, 5, 0, None, H, BIG, H, 1, grads, 0, H, 16, None),
        "backward shapes": lambda: bwd(blk0, 1, 64, 1, 3, 5, 0, None, H, BIG, H, 1, grads, 0, H, BIG, None),
        "backward fp32 weights": lambda: bwd(fit, 1, 64, 1, 3, 5, 0, None, H, BIG, H, 1, grads, 0, H, BIG, None),
        "vit precision": lambda: vit(None, None, 2, 7, None, None, None, 0, None),
        "vit null": lambda: vit(None, None, 2, PARITY, None, None, None, 0, None),
        "vit no output": lambda: vit(_vit(L), H, 2, PARITY, None, None, H, BIG, None),
        "vit geometry": lambda: vit(_vit(L, heads=5), H, 2, PARITY, H, None, H, BIG, None),
        "vit shapes": lambda: vit(_vit(L, shapes=False), H, 2, PARITY, H, None, H, BIG, None),
        "vit workspace cls": lambda: vit(_vit(L), H, 2, PARITY, H, None, H, 16, None),
        "vit workspace tokens": lambda: vit(_vit(L), H, 2, FAST, H, H, H, 16, None),
        "vit no batch": lambda: vit(None, None, 0, PARITY, None, None, None, 0, None),
        "text precision": lambda: txt(None, None, None, 2, 32, 7, None, None, None, None, 0, None),
        "text null": lambda: txt(None, None, None, 2, 32, PARITY, None, None, None, None, 0, None),
        "text no output": lambda: txt(_text(L), H, None, 2, 32, PARITY, None, None, None, H, BIG, None),
        "text context": lambda: txt(_text(L), H, None, 2, 78, PARITY, H, None, None, H, BIG, None),
        "text no tokens": lambda: txt(_text(L), H, None, 2, 0, PARITY, H, None, None, H, BIG, None),
        "text shapes": lambda: txt(_text(L, heads=7), H, None, 2, 32, PARITY, H, None, None, H, BIG, None),
        "text workspace eos": lambda: txt(_text(L), H, None, 2, 32, EXACT, H, None, None, H, 16, None),
        "text workspace tokens": lambda: txt(_text(L), H, None, 2, 32, PARITY, H, H, None, H, 16, None),
        "text no batch": lambda: txt(None, None, None, 0, 32, PARITY, None, None, None, None, 0, None),
        "packed precision": lambda: pck(None, None, None, 0, 4, 32, 7, None, None, 0, None),
        "packed null": lambda: pck(None, None, None, 0, 4, 32, PARITY, None, None, 0, None),
        "packed context": lambda: pck(_text(L), H, H, 8, 4, 78, PARITY, H, H, BIG, None),
        "packed 64": lambda: pck(_text(L), H, H, 8, 4, 65, PARITY, H, H, BIG, None),
        "packed few rows": lambda: pck(_text(L), H, H, 3, 4, 32, PARITY, H, H, BIG, None),
        "packed many rows": lambda: pck(_text(L), H, H, 129, 4, 32, PARITY, H, H, BIG, None),
        "packed shapes": lambda: pck(_text(L, heads=0), H, H, 8, 4, 32, PARITY, H, H, BIG, None),
        "packed workspace": lambda: pck(_text(L), H, H, 8, 4, 32, FAST, H, H, 16, None),
        "packed no batch": lambda: pck(None, None, None, 0, 0, 32, PARITY, None, None, 0, None),
        "packed_dev precision": lambda: dev(None, None, None, 4, 32, 7, None, None, None, 0, None),
        "packed_dev exact": lambda: dev(_text(L), H, None, 4, 32, EXACT, H, None, H, BIG, None),
        "packed_dev null": lambda: dev(None, None, None, 4, 32, PARITY, None, None, None, 0, None),
        "packed_dev context": lambda: dev(_text(L), H, None, 4, 78, PARITY, H, None, H, BIG, None),
        "packed_dev 64": lambda: dev(_text(L), H, None, 4, 65, FAST, H, None, H, BIG, None),
        "packed_dev shapes": lambda: dev(_text(L, heads=7), H, None, 4, 32, PARITY, H, None, H, BIG, None),
        "packed_dev workspace eos": lambda: dev(_text(L), H, None, 4, 32, PARITY, H, None, H, 16, None),
        "packed_dev workspace tokens": lambda: dev(_text(L), H, H, 4, 32, FAST, H, H, H, 16, None),
        "packed_dev no batch": lambda: dev(None, None, None, 0, 32, PARITY, None, None, None, 0, None),
        "dcmht precision": lambda: dcmht(None, None, 2, 7, None, None, None, None, 0, None),
        "dcmht null": lambda: dcmht(None, None, 2, PARITY, None, None, None, None, 0, None),
        "dcmht shapes": lambda: dcmht(_dcmht(L, 33), H, 2, PARITY, H, None, None, H, BIG, None),
        "dcmht workspace": lambda: dcmht(_dcmht(L, 128), H, 2, PARITY, H, None, None, H, 16, None),
        "dcmht workspace exact": lambda: dcmht(_dcmht(L, 128), H, 2, EXACT, H, None, None, H, 16, None),
        "dsph precision": lambda: dsph(None, None, 2, 7, None, None, None, None, None, None, 0, None),
        "dsph null": lambda: dsph(None, None, 2, PARITY, None, None, None, None, None, None, 0, None),
        "dsph bits": lambda: dsph(ctypes.byref(lin(None, None, None, None, 1025, 512)), H, 2, PARITY, H, None, None, None, None, H, BIG, None),
        "dsph no workspace": lambda: dsph(ctypes.byref(lin(None, None, None, None, 64, 512)), H, 2, PARITY, None, H, None, None, None, None, 0, None),
        "dsph workspace": lambda: dsph(ctypes.byref(lin(None, None, None, None, 64, 512)), H, 2, FAST, H, None, None, None, None, H, 16, None),
        "mith precision": lambda: mith(None, None, None, None, 2, 50, 7, None, None, None, 0, None),
        "mith null": lambda: mith(None, None, None, None, 2, 50, PARITY, None, None, None, 0, None),
        "mith shapes": lambda: mith(ctypes.byref(L.MithHead()), H, H, None, 2, 50, PARITY, H, H, H, BIG, None),
        "mith workspace": lambda: mith(_mith(L), H, H, None, 2, 50, PARITY, H, H, H, 16, None),
        "mith workspace exact": lambda: mith(_mith(L), H, H, None, 2, 50, EXACT, H, H, H, 16, None),
    }


# name -> (return code, xmh_last_error() when the code is not 0)
REFUSALS = {
    'blocks precision': (-22, 'xmh forward: precision must be 0 (parity), 1 (fast) or 2 (exact), got 7'),
    'blocks null': (-22, 'xmh_clip_blocks_forward: bad arguments'),
    'blocks heads': (-22, 'xmh_clip_blocks_forward: bad arguments'),
    'blocks workspace parity': (-12, 'xmh_clip_blocks_forward: workspace of 16 bytes, 35072 needed'),
    'blocks workspace fast': (-12, 'xmh_clip_blocks_forward: workspace of 16 bytes, 23296 needed'),
    'blocks workspace exact': (-12, 'xmh_clip_blocks_forward: workspace of 16 bytes, 34560 needed'),
    'blocks shapes': (-22, 'xmh forward: block 0 has layer shapes that do not fit width 64'),
    'blocks shapes exact': (-22, 'xmh forward: block 0 has layer shapes that do not fit width 64'),
    'blocks fp32 weights': (-22, 'xmh forward: block 0 lacks fp32 weights (exact mode)'),
    'blocks fp16 weights': (-22, 'xmh forward: block 0 lacks fp16 weights (w_hi) for width 64'),
    'blocks fp16 weights fast': (-22, 'xmh forward: block 0 lacks fp16 weights (w_hi) for width 64'),
    'blocks no batch': (0, ''),
    'blocks no layers': (0, ''),
    'saved precision': (-22, 'xmh forward: precision must be 0 (parity), 1 (fast) or 2 (exact), got 7'),
    'saved null': (-22, 'xmh_clip_blocks_forward_saved: bad arguments'),
    'saved width': (-95, 'xmh_clip_blocks_forward_saved: width 66 is not a multiple of 4'),
    'saved record': (-12, 'xmh_clip_blocks_forward_saved: saved buffer of 16 bytes, 122880 needed'),
    'saved workspace': (-12, 'xmh_clip_blocks_forward_saved: workspace of 16 bytes, 34560 needed'),
    'saved no batch': (0, ''),
    'saved no layers': (0, ''),
    'backward null saved': (-22, 'xmh_clip_blocks_backward: null saved buffer'),
    'backward record': (-12, 'xmh_clip_blocks_backward: saved buffer of 16 bytes, 122880 needed'),
    'backward workspace': (-12, 'xmh_clip_blocks_backward: workspace of 16 bytes, 117760 needed'),
    'backward shapes': (-22, 'xmh_clip_blocks_backward: block 0 has layer shapes that do not fit width 64'),
    'backward fp32 weights': (-22, 'xmh_clip_blocks_backward: block 0 lacks fp32 weights'),
    'vit precision': (-22, 'xmh forward: precision must be 0 (parity), 1 (fast) or 2 (exact), got 7'),
    'vit null': (-22, 'xmh_vit_b32_forward: bad arguments'),
    'vit no output': (-22, 'xmh_vit_b32_forward: bad arguments'),
    'vit geometry': (-22, 'xmh_vit_b32_forward: resolution 224 / patch 32 / width 768 / heads 5 do not fit'),
    'vit shapes': (-22, 'xmh_vit_b32_forward: conv1 / proj shapes do not fit the tower'),
    'vit workspace cls': (-12, 'xmh_vit_b32_forward: workspace of 16 bytes, 4590080 needed'),
    'vit workspace tokens': (-12, 'xmh_vit_b32_forward: workspace of 16 bytes, 3373568 needed'),
    'vit no batch': (0, ''),
    'text precision': (-22, 'xmh forward: precision must be 0 (parity), 1 (fast) or 2 (exact), got 7'),
    'text null': (-22, 'xmh_text_forward: bad arguments'),
    'text no output': (-22, 'xmh_text_forward: bad arguments'),
    'text context': (-22, 'xmh_text_forward: 78 tokens, the positional embedding holds 77'),
    'text no tokens': (-22, 'xmh_text_forward: 0 tokens, the positional embedding holds 77'),
    'text shapes': (-22, 'xmh_text_forward: shapes do not fit the tower'),
    'text workspace eos': (-12, 'xmh_text_forward: workspace of 16 bytes, 1319424 needed'),
    'text workspace tokens': (-12, 'xmh_text_forward: workspace of 16 bytes, 1450496 needed'),
    'text no batch': (0, ''),
    'packed precision': (-22, 'xmh forward: precision must be 0 (parity), 1 (fast) or 2 (exact), got 7'),
    'packed null': (-22, 'xmh_text_forward_packed: bad arguments'),
    'packed context': (-22, 'xmh_text_forward_packed: 78 tokens (positional embedding 77, packed attention 64)'),
    'packed 64': (-22, 'xmh_text_forward_packed: 65 tokens (positional embedding 77, packed attention 64)'),
    'packed few rows': (-22, 'xmh_text_forward_packed: 3 rows for 4 captions of at most 32 tokens'),
    'packed many rows': (-22, 'xmh_text_forward_packed: 129 rows for 4 captions of at most 32 tokens'),
    'packed shapes': (-22, 'xmh_text_forward_packed: shapes do not fit the tower'),
    'packed workspace': (-12, 'xmh_text_forward_packed: workspace of 16 bytes, 1851904 needed'),
    'packed no batch': (0, ''),
    'packed_dev precision': (-22, 'xmh forward: precision must be 0 (parity), 1 (fast) or 2 (exact), got 7'),
    'packed_dev exact': (-95, 'xmh_text_forward_packed_dev: parity or fast mode only'),
    'packed_dev null': (-22, 'xmh_text_forward_packed_dev: bad arguments'),
    'packed_dev context': (-22, 'xmh_text_forward_packed_dev: 78 tokens (positional embedding 77, packed attention 64)'),
    'packed_dev 64': (-22, 'xmh_text_forward_packed_dev: 65 tokens (positional embedding 77, packed attention 64)'),
    'packed_dev shapes': (-22, 'xmh_text_forward_packed_dev: shapes do not fit the tower'),
    'packed_dev workspace eos': (-12, 'xmh_text_forward_packed_dev: workspace of 16 bytes, 2638336 needed'),
    'packed_dev workspace tokens': (-12, 'xmh_text_forward_packed_dev: workspace of 16 bytes, 2114048 needed'),
    'packed_dev no batch': (0, ''),
    'dcmht precision': (-22, 'xmh forward: precision must be 0 (parity), 1 (fast) or 2 (exact), got 7'),
    'dcmht null': (-22, 'xmh_head_dcmht: bad arguments'),
    'dcmht shapes': (-22, 'xmh_head_dcmht: layer shapes do not fit (E = 512, fc2 33 x 512)'),
    'dcmht workspace': (-12, 'xmh_head_dcmht: workspace of 16 bytes, 28672 needed'),
    'dcmht workspace exact': (-12, 'xmh_head_dcmht: workspace of 16 bytes, 24576 needed'),
    'dsph precision': (-22, 'xmh forward: precision must be 0 (parity), 1 (fast) or 2 (exact), got 7'),
    'dsph null': (-22, 'xmh_head_dsph: bad arguments'),
    'dsph bits': (-22, 'xmh_head_dsph: 1025 bits from 512 features exceed the workspace layout'),
    'dsph no workspace': (-22, 'xmh_head_dsph: workspace needed'),
    'dsph workspace': (-12, 'xmh_head_dsph: workspace of 16 bytes, 26624 needed'),
    'mith precision': (-22, 'xmh forward: precision must be 0 (parity), 1 (fast) or 2 (exact), got 7'),
    'mith null': (-22, 'xmh_head_mith: bad arguments'),
    'mith shapes': (-22, 'xmh_head_mith: head shapes do not fit (width 0, 0 bits, 0 heads)'),
    'mith workspace': (-12, 'xmh_head_mith: workspace of 16 bytes, 3879936 needed'),
    'mith workspace exact': (-12, 'xmh_head_mith: workspace of 16 bytes, 3900416 needed'),
}


def test_every_call_has_a_recorded_answer(L):
    assert sorted(_calls(L)) == sorted(REFUSALS)


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusal_before_the_first_launch(L, name):
    code, text = REFUSALS[name]
    rc = _calls(L)[name]()
    assert rc == code, (rc, L.lib.xmh_last_error())
    if code:
        assert L.lib.xmh_last_error().decode() == text
