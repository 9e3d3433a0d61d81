"""The argument checks of the four objectives' entry points (xmh_hyp, xmh_dnph, xmh_dimch, xmh_umoed; loss and gradient each): a
workspace one byte short, a workspace pointer off its 256-byte alignment and a shape one past the bound are each refused with the
entry's own status, before any HIP call -- so host buffers do, no GPU is needed -- and with the outputs left as they were."""
import ctypes as C

import numpy as np
import pytest

from xmh import _lib
from xmh._lib import lib
from xmh.models.dimch import DimchConsts

EINVAL, ENOMEM, ENOTSUP = -22, -12, -95
B, K, CLS = 2, 4, 3                                      # K is also M and V
FILL = 7.25


def _p(a):
    return C.c_void_p(a.ctypes.data)


DIMCH_CST = DimchConsts(1, 1, 2.0, 16.0, 1.0, 0.2, 0.3, 0.5, 1.0, 0.01, 0.01, 0.5, 0.001)
UMOED_CST = _lib.UmoedConsts(0, 0.01, 0.2, 1.0, 0.01)
LAB = np.ones((B, 1), dtype=np.uint32)
XS = np.full((B, K, K), 0.5, dtype=np.float32)
X = _p(XS)                                               # stands for every input: no check reads through it


# per objective: the short-workspace status, the shapes of the call and the bound of each, a function that packs
# the leading arguments of both entries from the shapes, the workspace sizing from the shapes, the out length, the gradient shapes
def _hyp(b, k, c):
    return (X, X, X, b, k, c, _p(LAB), 0.25, 0.8)


def _dnph(b, k, c, cp):
    return (X, X, X, X, X, b, k, c, cp, _p(LAB), 1.0, 0.1, None, None)


def _dimch(b, m, k, kh, c):
    return (X, X, X, X, b, m, k, kh, c, _p(LAB), C.byref(DIMCH_CST))


def _umoed(b, m, v, c):
    return (X, X, b, m, v, c, _p(LAB), C.byref(UMOED_CST))


OBJECTIVES = {
    "hyp": dict(short=EINVAL, shape=(B, K, CLS), bound=(4096, 4096, 1024), pack=_hyp, ws=lambda s: lib.xmh_hyp_loss_ws_bytes(*s), out=8,
                grads=((B, K), (B, K), (CLS, K))),
    "dnph": dict(short=ENOMEM, shape=(B, K, CLS, CLS), bound=(4096, 4096, 1024, 1024), pack=_dnph,
                 ws=lambda s: lib.xmh_dnph_loss_ws_bytes(*s), out=8, grads=((B, K), (B, K), (B, CLS), (B, CLS), (CLS, K))),
    "dimch": dict(short=ENOMEM, shape=(B, K, K, K, CLS), bound=(512, 64, 256, 256, 127), pack=_dimch,
                  ws=lambda s: lib.xmh_dimch_loss_ws_bytes(s[0], s[1], s[2], s[4]), out=12, grads=((B, K, K), (B, K, K), (B, K), (B, K))),
    "umoed": dict(short=ENOMEM, shape=(B, K, K, CLS), bound=(512, 128, 256, 127), pack=_umoed, ws=lambda s: lib.xmh_umoed_loss_ws_bytes(*s),
                  out=8, grads=((B, K, K), (B, K, K))),
}


def _call(name, entry, shape, ws_ptr, ws_bytes):
    """-> (status, the output buffers, all prefilled with FILL)"""
    o = OBJECTIVES[name]
    lead = o["pack"](*shape)
    if entry == "loss":
        outs = [np.full(o["out"], FILL, dtype=np.float64)]
        rc = getattr(lib, "xmh_%s_loss" % name)(*lead, ws_ptr, ws_bytes, _p(outs[0]), None)
    else:
        up = np.ones(1, dtype=np.float32)
        outs = [np.full(s, FILL, dtype=np.float32) for s in o["grads"]]
        rc = getattr(lib, "xmh_%s_loss_grad" % name)(*lead, _p(up), *[_p(g) for g in outs], 0, ws_ptr, ws_bytes, None)
    return rc, outs


def _aligned(nbytes):
    """a host buffer with nbytes + 256 usable bytes from a 256-byte aligned address -> (keep-alive, address)"""
    buf = np.zeros(nbytes + 512, dtype=np.uint8)
    return buf, (buf.ctypes.data + 255) & ~255


@pytest.mark.parametrize("entry", ["loss", "grad"])
@pytest.mark.parametrize("name", sorted(OBJECTIVES))
def test_rejections_keep_their_status_and_leave_the_outputs_alone(name, entry):
    o = OBJECTIVES[name]
    need = o["ws"](o["shape"])
    assert need > 0 and need % 256 == 0
    keep, base = _aligned(need)
    who = ("xmh_%s_loss" % name) + ("_grad" if entry == "grad" else "")

    def refused(rc, outs, status, text):
        msg = lib.xmh_last_error().decode()
        assert rc == status, (rc, msg)
        assert msg.startswith(who + ":") and text in msg, msg
        assert all((t == FILL).all() for t in outs)

    refused(*_call(name, entry, o["shape"], C.c_void_p(base), need - 1), o["short"], "workspace of %d bytes < %d (xmh_%s_loss_ws_bytes)"
            % (need - 1, need, name))
    refused(*_call(name, entry, o["shape"], C.c_void_p(base + 128), need), EINVAL, "workspace not 256-byte aligned")
    for i, top in enumerate(o["bound"]):                 # each bounded extent in turn, one past its bound
        shape = tuple(top + 1 if j == i else s for j, s in enumerate(o["shape"]))
        if name == "dnph" and i == 2:                    # Cp >= C is asked before the bounds are
            shape = shape[:3] + (top + 1,)
        assert o["ws"](shape) == 0 or name == "dimch" and i == 3          # Kh does not enter DIMCH's workspace
        refused(*_call(name, entry, shape, C.c_void_p(base), need), ENOTSUP, "outside")
    assert keep is not None
