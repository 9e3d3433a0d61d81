"""CPU: MITH's training objective -- a float64 restatement of the reference expression (models/MITH/MITH.py:116-232) against goldens
written by the reference itself (tools/make_golden_mith_loss.py), the model-side contract (one buffer under four names, weights,
state_dict, the errors raised before any launch) and the argument checks of xmh_mith_loss / xmh_mith_loss_grad, which run before
any HIP call."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN

CASES = ["consecutive", "clamp", "sign0", "float_sim", "weights", "odd"]
INPUTS = ["res_img_cls", "res_txt_cls", "img_cls_hash", "txt_cls_hash", "tokens_hash_i", "tokens_hash_t", "trans_tokens_i",
          "trans_tokens_t"]
WEIGHTS = ["hyper_tokens_intra", "hyper_distill", "hyper_info_nce", "hyper_cls_inter", "hyper_quan", "hyper_alpha", "hyper_lambda"]
TERMS = ["loss", "intra_i", "intra_t", "i2t", "t2i", "quan_i", "quan_t", "nce_cls", "nce_tokens", "distillation"]   # out10
SYNTH_CLIP = "synthetic:1814:vision_layers=1,transformer_layers=1"


def mith_terms(xs, Y, S, w, tau=0.07):
    """The reference expression restated in the inputs' dtype (float64 for an oracle): the TERMS as a list, differentiable in xs.
    Y is the one buffer after the step's row write.  sign() is taken on fp32 codes, op for op, as the reference takes it."""
    rc_i, rc_t, c_i, c_t, t_i, t_t, T_i, T_t = xs
    lam = w["hyper_lambda"]

    def bayes(b):
        s = 0.5 * (Y @ b.T).clamp(min=-64, max=64)
        return -torch.mean(S * s - torch.log(1 + torch.exp(s)))

    def nce(s):                                   # s [n, m, m] logits; rows and columns against the diagonal
        n, m = s.shape[0], s.shape[1]
        tgt = torch.arange(m).repeat(n)
        return 0.5 * (F.cross_entropy(s.reshape(n * m, m), tgt) + F.cross_entropy(s.transpose(1, 2).reshape(n * m, m), tgt))

    f = [t.detach().float() for t in (c_i, t_i, c_t, t_t)]
    Bs = torch.sign((f[0] * lam + f[1] * (1 - lam)) + (f[2] * lam + f[3] * (1 - lam))).to(c_i.dtype)
    B, K = c_i.shape
    t = [None, bayes(t_i), bayes(t_t), bayes(c_t), bayes(c_i),
         ((c_i * 0.5 + t_i * 0.5 - Bs) ** 2).sum() / B / K, ((c_t * 0.5 + t_t * 0.5 - Bs) ** 2).sum() / B / K,
         nce((rc_i @ rc_t.T / tau)[None]), nce(torch.bmm(T_i.permute(1, 0, 2), T_t.permute(1, 2, 0)) / tau)]
    t.append(w["hyper_distill"] * (((c_i.detach() - t_i) ** 2).sum() + ((c_t.detach() - t_t) ** 2).sum()
                                   + 0.1 * (((c_i - t_i.detach()) ** 2).sum() + ((c_t - t_t.detach()) ** 2).sum())) / B)
    t[0] = (w["hyper_tokens_intra"] * (t[1] + t[2]) + w["hyper_cls_inter"] * (t[3] + t[4]) + w["hyper_quan"] * (t[5] + t[6])
            + w["hyper_info_nce"] * (t[7] + w["hyper_alpha"] * t[8]) + t[9])
    return t


def mith_oracle(xs, Y, S, w):
    """float64 terms (numpy [10], TERMS order) and the eight gradients of the loss (float64 numpy)"""
    xs = [torch.as_tensor(np.asarray(x)).double().requires_grad_(True) for x in xs]
    t = mith_terms(xs, torch.as_tensor(np.asarray(Y)).double(), torch.as_tensor(np.asarray(S)).double(), w)
    t[0].backward()
    return np.array([float(v.detach()) for v in t]), [x.grad.numpy() for x in xs]


def load(name):
    """(N, B, K, D, weights dict, buf0, [step dicts with the inputs list, indexs, label_sim, buf, terms, grads list])"""
    g = np.load(os.path.join(GOLDEN, "loss_mith.npz"))
    meta = g[name + "_meta"]
    N, B, K, D, steps = (int(v) for v in meta[:5])
    w = dict(zip(WEIGHTS, (float(v) for v in meta[5:])))
    out = []
    for s in range(steps):
        p = "%s_s%d_" % (name, s)
        out.append({"inputs": [g[p + k] for k in INPUTS], "indexs": g[p + "indexs"], "label_sim": g[p + "label_sim"], "buf": g[p + "buf"],
                    "terms": g[p + "terms"], "grads": [g[p + "g_" + k] for k in INPUTS]})
    return N, B, K, D, w, g[name + "_buf0"], out


def grads_close(got, ref):
    """relative to the largest entry of the matrix (test_oracle_losses.grads_close)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(got - ref).max()) <= 2e-5 * float(np.abs(ref).max()) + 1e-9


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
def _host(n):
    """a 256-byte aligned host address with n bytes behind it (never dereferenced by a call that fails its checks)"""
    buf = np.zeros(n + 256, dtype=np.uint8)
    return buf, ctypes.c_void_p((buf.ctypes.data + 255) & ~255)


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
