"""CPU: MITH's training objective -- a float64 restatement of the reference expression (models/MITH/MITH.py:116-232) against goldens
written by the reference itself (oracle/make_golden_mith_loss.py), the model-side contract (one buffer under four names, weights,
state_dict, the errors raised before any launch) and the argument checks of xmh_mith_loss / xmh_mith_loss_grad, which run before
any HIP call."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle.fixtures import aligned_host as _host, grads_close
from oracle.losses import MITH_CASES as CASES, MITH_INPUTS as INPUTS, MITH_WEIGHTS as WEIGHTS, load_mith as load, mith_oracle

SYNTH_CLIP = "synthetic:1814:vision_layers=1,transformer_layers=1"


@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_the_reference(name):
    N, B, K, D, w, buf0, steps = load(name)
    buf = buf0.copy()
    for st in steps:
        buf[st["indexs"]] = st["inputs"][5]                              # the step's write: tokens_hash_t's rows stay
        assert np.array_equal(buf, st["buf"])
        terms, grads = mith_oracle(st["inputs"], buf, st["label_sim"], w)
        assert np.allclose(terms, st["terms"], rtol=2e-5, atol=1e-6), (name, terms, st["terms"])
        for k, got, ref in zip(INPUTS, grads, st["grads"]):
            assert grads_close(got, ref), (name, k, np.abs(got - ref).max(), np.abs(ref).max())


def test_goldens_cover_what_their_names_say():
    _, _, K, _, _, _, steps = load("clamp")
    st = steps[0]
    Y = st["buf"]
    dots = np.concatenate([Y @ st["inputs"][i].T for i in (2, 3, 4, 5)], axis=1)
    assert K == 128 and (dots == 64).any() and (dots == -64).any() and (np.abs(dots) > 64).any()
    _, _, _, _, w, _, steps = load("sign0")
    c_i, c_t, t_i, t_t = (torch.as_tensor(steps[0]["inputs"][i]) for i in (2, 3, 4, 5))
    lam = w["hyper_lambda"]
    assert (torch.sign((c_i * lam + t_i * (1 - lam)) + (c_t * lam + t_t * (1 - lam))) == 0).any()
    S = load("float_sim")[6][0]["label_sim"]
    assert ((S != 0) & (S != 1)).any()
    assert load("weights")[4]["hyper_alpha"] == 0.0
    assert load("odd")[2:4] == (24, 72)
    assert len(load("consecutive")[6]) == 3
    assert abs(np.linalg.norm(load("odd")[6][0]["inputs"][0], axis=1) - 1).max() > 0.1      # rows not normalised


# ---- the model side (no GPU involved) -------------------------------------------------------------------------------------------
def _mith(**cfg):
    from xmh.models.mith import MITH
    from xmh.utils.config import Config
    return MITH.from_config(Config(dict({"clip_path": SYNTH_CLIP}, **cfg)), output_dim=16, train_num=300)


def _inputs(B=4, K=16, D=512):
    g = torch.Generator().manual_seed(3)
    return dict(res_img_cls=torch.randn(B, D, generator=g), res_txt_cls=torch.randn(B, D, generator=g),
                img_cls_hash=torch.rand(B, K, generator=g), txt_cls_hash=torch.rand(B, K, generator=g),
                tokens_hash_i=torch.rand(B, K, generator=g), tokens_hash_t=torch.rand(B, K, generator=g),
                trans_tokens_i=torch.randn(K, B, D, generator=g), trans_tokens_t=torch.randn(K, B, D, generator=g))


def test_buffer_is_one_tensor_outside_the_state_dict():
    import xmh.models  # noqa: F401
    from oracle import runner_fixture as RF
    from xmh.common.register import registry
    from xmh.utils.config import Config
    m = _mith()
    assert m.img_buffer_cls is m.txt_buffer_cls is m.img_buffer_tokens is m.txt_buffer_tokens
    assert tuple(m.img_buffer_cls.shape) == (300, 16) and m.img_buffer_cls.dtype == torch.float32 and not m.img_buffer_cls.is_cuda
    assert not any("buffer" in k for k in m.state_dict())
    g = np.load(os.path.join(GOLDEN, "runner.npz"))
    want = sorted(str(k) for k in g["MITH_state_keys"])
    model = registry.get_model_class("MITH").from_config(
        Config({"clip_path": "synthetic:%d:vision_layers=%d,transformer_layers=%d" % (RF.SEED, RF.CLIP_LAYERS, RF.CLIP_LAYERS)}),
        output_dim=RF.CASES["MITH"])
    assert sorted(k for k in model.state_dict() if not k.endswith("num_batches_tracked")) == want
    torch.manual_seed(7)
    first = _mith().img_buffer_cls
    torch.manual_seed(8)
    assert torch.equal(_mith().img_buffer_cls, first)                             # a private generator: same draw whatever the global seed


def test_weight_defaults_and_cfg_overrides():
    m = _mith()
    assert [getattr(m, k) for k in WEIGHTS] == [1.0, 1.0, 50.0, 10.0, 8.0, 0.01, 0.99]
    m = _mith(hyper_quan=3, hyper_alpha=0.0, hyper_lambda=0.5)
    assert (m.hyper_quan, m.hyper_alpha, m.hyper_lambda, m.hyper_info_nce) == (3.0, 0.0, 0.5, 50.0)


def test_errors_before_any_launch():
    m = _mith()
    x = _inputs()
    with pytest.raises(AssertionError, match="MITH must provide the label similarity"):
        m.object_function(**x, indexs=np.arange(4))
    S = torch.rand(300, 4)
    with pytest.raises(IndexError):
        m.object_function(**x, indexs=np.array([0, 1, 2, 300]), label_sim=S)
    with pytest.raises(IndexError):
        m.object_function(**x, indexs=torch.tensor([0, -301, 2, 3]), label_sim=S)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.object_function(**x, indexs=np.arange(4), label_sim=S)
    with pytest.raises(RuntimeError, match="do not fit"):
        m.object_function(**x, indexs=np.arange(4), label_sim=torch.rand(299, 4))
    assert torch.equal(m.img_buffer_cls, _mith().img_buffer_cls)                 # nothing was written


# ---- C ABI argument checks (no GPU involved: each call returns before its first HIP call) ------------------------------------
def test_argument_errors_are_reported_without_a_gpu():
    from xmh import _lib
    lib = _lib.lib
    assert lib.xmh_mith_loss_ws_bytes(10000, 100, 128, 512) > 0 and lib.xmh_mith_loss_ws_bytes(1 << 22, 1024, 256, 2048) > 0
    for bad in ((0, 100, 16, 512), (10000, 0, 16, 512), ((1 << 22) + 1, 100, 16, 512), (100, 1025, 16, 512), (100, 10, 257, 512),
                (100, 10, 16, 2049)):
        assert lib.xmh_mith_loss_ws_bytes(*bad) == 0
    need = lib.xmh_mith_loss_ws_bytes(100, 8, 16, 64)
    keep, p = _host(max(need, 1 << 16))
    _, out = _host(128)
    grads = (ctypes.c_void_p * 8)(*([p.value] * 8))

    def args(**kw):
        a = _lib.MithLossArgs(100, 8, 16, 64, *([p.value] * 10), 1.0, 1.0, 50.0, 10.0, 8.0, 0.01, 0.99, 0.07)
        for k, v in kw.items():
            setattr(a, k, v)
        return ctypes.byref(a)

    def loss(a=None, ws=p, ws_bytes=need, out10=out):
        return lib.xmh_mith_loss(a or args(), ws, ws_bytes, out10, None)

    def grad(a=None, ws=p, ws_bytes=need, g=grads):
        return lib.xmh_mith_loss_grad(a or args(), None, g, 0, ws, ws_bytes, None)

    for call, name in ((loss, b"xmh_mith_loss"), (grad, b"xmh_mith_loss_grad")):
        assert call(args(N=0)) == -22 and name + b": bad shape" in lib.xmh_last_error()
        assert call(args(B=-1)) == -22 and call(args(K=0)) == -22 and call(args(D=0)) == -22
        assert call(args(N=(1 << 22) + 1)) == -95 and b"N <= 4194304" in lib.xmh_last_error()
        assert call(args(B=1025)) == -95 and call(args(K=257)) == -95 and call(args(D=2049)) == -95
        for field in ("res_img_cls", "trans_tokens_t", "buffer", "label_sim"):
            assert call(args(**{field: None})) == -22 and b"null pointer" in lib.xmh_last_error()
        assert call(ws=None) == -22
        assert call(ws_bytes=need - 1) == -22 and b"workspace" in lib.xmh_last_error()
        assert call(ws=ctypes.c_void_p(p.value + 8)) == -22 and b"aligned" in lib.xmh_last_error()
        assert lib.xmh_mith_loss(None, p, need, out, None) if name == b"xmh_mith_loss" else \
            lib.xmh_mith_loss_grad(None, None, grads, 0, p, need, None)
        assert name + b": null pointer" in lib.xmh_last_error()
    assert loss(out10=None) == -22 and b"xmh_mith_loss: null pointer" in lib.xmh_last_error()
    assert grad(g=None) == -22 and b"xmh_mith_loss_grad: null pointer" in lib.xmh_last_error()
    del keep
