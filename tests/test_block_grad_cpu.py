"""No GPU: the golden file of the CLIP block-stack backward (tools/make_golden_block_grad.py: the reference Transformer's own fp32
gradients) against the restatement of tests/block_grad_cases.py -- its fp32 run regenerates the stored tensors to the bit, its fp64
run the stored e_ref -- and the binding of the new C entry points."""
import ctypes

import numpy as np
import pytest
import torch

import block_grad_cases as BC


@pytest.mark.parametrize("case", list(BC.CASES))
def test_restatement_regenerates_the_golden(case):
    G = BC.golden()
    D, heads, layers, L, B, causal, kp = BC.CASES[case]
    sd, x, up, kpm = BC.case_inputs(case)
    assert int(G[case + "__seed"]) == BC.case_seed(case)
    assert BC.inputs_checksum(sd, x, up, kpm) == float(G[case + "__checksum"])
    if kpm is not None:                                           # every query keeps a visible key
        assert not kpm[:, 0].any() and kpm.any()
    r32 = BC.run_restatement(sd, x, up, heads, causal, kpm, torch.float32)
    r64 = BC.run_restatement(sd, x, up, heads, causal, kpm, torch.float64)
    per, _ = BC.erefs(r32, r64)
    assert len(r32) == 2 + 12 * layers
    for k in r32:
        assert r32[k].dtype == np.float32 and np.isfinite(r64[k]).all()
        assert np.array_equal(G["%s__%s" % (case, k)], BC.thin(r32[k])), k
        assert float(G["%s__eref_%s" % (case, k)]) == per[k], k
        assert per[k] < 2e-6, (k, per[k])                         # an fp32 computation of this stack


def test_every_kind_has_a_pool_and_the_file_is_small():
    import os
    for kind in BC.KINDS:
        assert 1e-8 < BC.pool_eref(kind) < 2e-6, kind
    assert os.path.getsize(BC.GOLDEN) < 1 << 20
    assert float(BC.golden()["d64_l1_b1__eref_g_l0_proj_b"]) == 0.0       # B = L = 1: the bias gradient is the upstream row itself


def test_symbols_and_struct_are_bound():
    from xmh import _lib
    assert ctypes.sizeof(_lib.ClipBlockGrads) == 12 * ctypes.sizeof(ctypes.c_void_p)
    assert [n for n, _ in _lib.ClipBlockGrads._fields_] == [k for k, _ in BC.PARAMS]
    for name in ("xmh_clip_blocks_backward", "xmh_clip_blocks_backward_ws_bytes"):
        assert name in _lib.PROTOTYPES and getattr(_lib.lib, name).argtypes == _lib.PROTOTYPES[name][1]
    from xmh.models.clip import Transformer
    assert callable(Transformer.run_train)


def test_workspace_bytes():
    from xmh._lib import lib
    f = lib.xmh_clip_blocks_backward_ws_bytes
    assert f(0, 50, 768) == 0 and f(4, 0, 768) == 0 and f(4, 50, 0) == 0 and f(-1, 50, 768) == 0
    last = 0
    for B in (1, 2, 41, 128):
        n = f(B, 50, 768)
        assert n % 256 == 0 and n >= 5 * B * 50 * 768 * 4 and n >= last
        last = n
    assert f(4, 129, 768) == 0 and f(4, 50, 770) == 0                 # outside the limits


def test_argument_errors_without_a_gpu():
    from xmh import _lib
    L = _lib.lib
    one = ctypes.c_void_p(256)                                      # never dereferenced: every check below fails before a launch
    blocks = (_lib.ClipBlock * 1)()
    grads = (_lib.ClipBlockGrads * 1)()
    big = 1 << 40

    def call(width=128, heads=2, B=2, Lq=7, saved=one, sbytes=big, dy=one, ws=one, wbytes=big, g=grads, blk=blocks):
        return L.xmh_clip_blocks_backward(blk, 1, width, heads, B, Lq, 0, None, saved, sbytes, dy, 1, g, 0, ws, wbytes, None)

    assert call(dy=None) == -22 and b"xmh_clip_blocks_backward" in L.xmh_last_error()
    assert call(saved=None) == -22 and call(ws=None) == -22 and call(g=None) == -22 and call(blk=None) == -22
    assert call(heads=3) == -22 and call(Lq=0) == -22
    assert call(width=128, heads=1) == -95 and call(width=96, heads=2) == -95 and call(Lq=129) == -95
    need = L.xmh_clip_saved_bytes(2, 7, 128, 1)
    assert call(sbytes=need - 1) == -12 and b"saved" in L.xmh_last_error()
    assert call(sbytes=need, wbytes=L.xmh_clip_blocks_backward_ws_bytes(2, 7, 128) - 1) == -12 and b"workspace" in L.xmh_last_error()
    assert call(B=0) == 0                                            # nothing to do
