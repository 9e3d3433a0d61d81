#!/usr/bin/env python3
"""Golden vectors of MITH's training objective and of its gradients (loss.backward() with respect to the eight head outputs),
produced by the UNMODIFIED reference (models/MITH/MITH.py) through oracle._ref_import:
python oracle/make_golden_mith_loss.py [DIR] -> tests/golden/loss_mith.npz (or DIR/).  Needs the reference checkout; nothing at test time runs this.

The model is the reference's own class with only its backbone replaced (oracle/_ref_models.py: load_backbone -> (D, Identity)).  Before the first step its
four buffer names are bound to ONE tensor: that is what the reference's device branch (MITH.py:169-173) leaves behind on every GPU run,
and this machine has no GPU to take that branch.  Each step then runs the reference's object_function and loss.backward().

Per case: <case>_meta (N, B, K, D, steps, the seven weights), <case>_buf0 (the buffer before the first step) and per step s
<case>_s<s>_<name> for the eight inputs, indexs, label_sim, buf (the buffer after the step), terms (loss and the nine loss_dict
leaves in xmh_mith_loss's out10 order) and g_<input> (the eight gradients).  Feature inputs are rounded to multiples of 1/64 so that
the file stays small."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import _ref_models  # noqa: E402
from oracle.fixtures import out_path, q64  # noqa: E402
from oracle.losses import MITH_CASES as CASES, MITH_INPUTS as INPUTS, MITH_WEIGHTS as WEIGHTS  # noqa: E402

DEFAULT = dict(zip(WEIGHTS, (1.0, 1.0, 50.0, 10.0, 8.0, 0.01, 0.99)))    # configs/MITH/config.yaml


def features(g, B, K, D, normalise):
    rows = [torch.randn(B, D, generator=g) * 1.5, torch.randn(B, D, generator=g) * 1.5,
            torch.randn(K, B, D, generator=g) * 0.2, torch.randn(K, B, D, generator=g) * 0.2]
    if normalise:
        rows = [F.normalize(r, dim=-1) for r in rows]
    return [q64(r) for r in rows]


def codes(g, B, K):
    return [torch.tanh(torch.randn(B, K, generator=g) * 1.5) for _ in range(4)]      # c_i, c_t, t_i, t_t


def binary_sim(g, N, B, p=0.3):
    return (torch.rand(N, B, generator=g) < p).float()


def pm1(g, *shape):
    return torch.where(torch.rand(*shape, generator=g) < 0.5, -1.0, 1.0)


def one_step(g, N, B, K, D, idx, normalise=False, S=None, cs=None):
    rc_i, rc_t, T_i, T_t = features(g, B, K, D, normalise)
    c_i, c_t, t_i, t_t = codes(g, B, K) if cs is None else cs
    return (rc_i, rc_t, c_i, c_t, t_i, t_t, T_i, T_t), np.array(idx, dtype=np.int64), binary_sim(g, N, B) if S is None else S


def case_steps(name, g):
    """(N, B, K, D, weights, buf0, [(inputs in INPUTS order, indexs, label_sim), ...])"""
    w = dict(DEFAULT)
    if name == "consecutive":                     # three steps on one instance, overlapping rows
        N, B, K, D = 64, 8, 16, 64
        buf0 = torch.randn(N, K, generator=g)
        return N, B, K, D, w, buf0, [one_step(g, N, B, K, D, idx, normalise=True)
                                     for idx in (np.arange(0, 8), np.arange(4, 12)[::-1], [0, 63, 5, 20, 9, 33, 11, 2])]
    if name == "clamp":
        # +-1 codes and buffer at K 128: Y[n] . x = 128 - 2 flips hits +-64 exactly (32 or 96 flips), and goes beyond it
        N, B, K, D = 24, 4, 128, 64
        z = pm1(g, K)
        Y = pm1(g, N, K)
        for n, f in enumerate((0, 31, 32, 33, 64, 95, 96, 97, 128, 30, 34, 32, 96)):
            r = z.clone()
            r[torch.randperm(K, generator=g)[:f]] *= -1.0
            Y[B + n] = r
        cs = []
        for j in range(4):
            x = pm1(g, B, K)
            x[j % B] = z                                                   # one row of each code is z itself
            cs.append(x)
        return N, B, K, D, w, Y, [one_step(g, N, B, K, D, np.arange(B), cs=cs)]
    if name == "sign0":
        N, B, K, D = 40, 6, 16, 64
        c_i, c_t, t_i, t_t = codes(g, B, K)
        zero = torch.rand(B, K, generator=g) < 0.4
        c_t = torch.where(zero, -c_i, c_t)                             # (c_i l + t_i (1 - l)) + (c_t l + t_t (1 - l)) == 0 exactly
        t_t = torch.where(zero, -t_i, t_t)
        return N, B, K, D, w, torch.randn(N, K, generator=g), [one_step(g, N, B, K, D, np.arange(10, 16), cs=(c_i, c_t, t_i, t_t))]
    if name == "float_sim":
        N, B, K, D = 48, 8, 16, 64
        S = torch.rand(N, B, generator=g) * 1.5 - 0.25
        return N, B, K, D, w, torch.randn(N, K, generator=g), [one_step(g, N, B, K, D, np.arange(40, 48), S=S)]
    if name == "weights":
        N, B, K, D = 48, 8, 16, 64
        w = dict(zip(WEIGHTS, (0.5, 2.0, 3.0, 0.25, 1.5, 0.0, 0.7)))
        return N, B, K, D, w, torch.randn(N, K, generator=g), [one_step(g, N, B, K, D, np.arange(8) * 5, normalise=True)]
    if name == "odd":
        N, B, K, D = 50, 6, 24, 72
        return N, B, K, D, w, torch.randn(N, K, generator=g), [one_step(g, N, B, K, D, [49, 0, 17, 3, 30, 8])]
    raise KeyError(name)


def leaves(d):
    """loss_dict leaves in xmh_mith_loss's out10 order"""
    return [d["All loss"], d["LikeHood"]["intra_tokens"]["image"], d["LikeHood"]["intra_tokens"]["text"], d["LikeHood"]["cls_inter"]["image"],
            d["LikeHood"]["cls_inter"]["text"], d["Quantization"]["image"], d["Quantization"]["text"], d["InfoNCE"]["cls"],
            d["InfoNCE"]["tokens"], d["Distillation"]]


def main():
    out = {}
    for ci, name in enumerate(CASES):
        g = torch.Generator().manual_seed(1814 + ci)
        N, B, K, D, w, buf0, steps = case_steps(name, g)
        m = _ref_models.mith(N, K, D, w)
        buf = buf0.clone()
        m.img_buffer_cls = m.txt_buffer_cls = m.img_buffer_tokens = m.txt_buffer_tokens = buf     # the device branch's outcome
        out[name + "_meta"] = np.array([N, B, K, D, len(steps)] + [w[k] for k in WEIGHTS], dtype=np.float64)
        out[name + "_buf0"] = buf0.numpy()
        for s, (xs, idx, S) in enumerate(steps):
            xs = [x.clone().requires_grad_(True) for x in xs]
            kw = dict(zip(INPUTS, xs))
            loss, d = m.object_function(**kw, labels=None, indexs=idx, label_sim=S)
            loss.backward()                                                   # runners/MITH/runner.py:121
            assert m.txt_buffer_tokens is buf and m.img_buffer_cls is buf
            p = "%s_s%d_" % (name, s)
            for k, x in kw.items():
                out[p + k] = x.detach().numpy()
                out[p + "g_" + k] = x.grad.numpy().copy()
            out[p + "indexs"] = idx
            out[p + "label_sim"] = S.numpy()
            out[p + "buf"] = buf.numpy().copy()
            out[p + "terms"] = np.array([float(v) for v in leaves(d)], dtype=np.float64)
            print(name, s, "terms", out[p + "terms"])
    np.savez_compressed(out_path("loss_mith.npz"), **out)


if __name__ == "__main__":
    main()
