"""No GPU: the float64 restatement of DNPH's objective (tests/dnph_cases.py) against the golden of the reference's own Loss, gene_noise
and DNPH.compute_loss (tests/golden/dnph.npz, tools/make_golden_dnph.py); the assignment solver; the new C symbols and their argument
errors; the registry, the head's state dict and the defaults of the Python layer.

Tolerance against the golden: the reference's numbers are float32 results, its distances torch.cdist ** 2 on the matmul route, so the
float64 restatement on the same inputs is expected within a few tens of eps32 of them, every scalar relative to itself and every
gradient relative to its largest entry.  Measured: 7.0e-7 at most (g_P of `mid`; 2.8e-7 in `small`; the scalars 1.2e-7 at most),
which is 5.9 eps32.  ROUND = 24 eps32 is 4 times that."""
import ctypes
import inspect
import itertools
import os
import re
import types

import numpy as np
import pytest
import torch

import dnph_cases as DC
from conftest import ROOT

ROUND = 24 * float(np.finfo(np.float32).eps)
NEW = ("xmh_dnph_loss_ws_bytes", "xmh_dnph_loss", "xmh_dnph_loss_grad", "xmh_assign_min_cost", "xmh_linear_backward")
SMALL = "synthetic:1814:vision_layers=1,transformer_layers=1,vision_width=128,transformer_width=128,embed_dim=64,image_resolution=64"


def _golden(name):
    G = np.load(DC.GOLDEN)
    g = {k.split("__", 1)[1]: G[k] for k in G.files if k.startswith(name + "__")}
    return dict(g, labels=g["labels"].astype(np.int64), mrg=float(g["mrg"]), alpha=float(g["noise_alpha"]), up=1.0,
                noise_img=g["noise_img"].astype(np.float32), noise_txt=g["noise_txt"].astype(np.float32))


@pytest.mark.parametrize("name", list(DC.GOLDEN_CASES))
def test_restatement_reproduces_the_reference(name):
    g = _golden(name)
    shape = DC.GOLDEN_CASES[name]
    assert g["f_img"].shape == (shape["B"], shape["K"]) and g["P"].shape == (shape["C"], shape["K"]) and g["p_img"].shape[1] == 80
    assert g["labels"][0].sum() == 0 and g["labels"][1].all()                       # a row without a label, a row with every label
    r1 = DC.objective(g, torch.float64, noise=False)                                 # Loss.forward and its backward
    worst = {"loss1": abs(r1["loss"][0] / float(g["loss1"]) - 1)}
    for k in DC.GRADS:
        worst[k] = DC.rel_err(r1[k], g[k])
    r = DC.objective(g, torch.float64)                                               # compute_loss with the recorded assignment
    worst["loss"] = abs(r["loss"][0] / float(g["loss"]) - 1)
    worst["noise_img"] = abs(r["noise_img"][0] / float(g["noise_mean_img"]) - 1)
    worst["noise_txt"] = abs(r["noise_txt"][0] / float(g["noise_mean_txt"]) - 1)
    print(name, " ".join("%s %.2e" % kv for kv in worst.items()))
    assert all(v <= ROUND for v in worst.values()), worst
    # what the bound is there for: a margin of the wrong sign, or a noise weight 1 % off, is far outside it
    flipped = DC.objective(g, torch.float64, mrg=-g["mrg"], noise=False)
    wrong = {k: DC.rel_err(flipped[k], g[k]) for k in ("g_f_img", "g_f_txt", "g_P")}
    wrong["loss1"] = abs(flipped["loss"][0] / float(g["loss1"]) - 1)
    wrong["loss"] = abs(DC.objective(g, torch.float64, alpha=1.01 * g["alpha"])["loss"][0] / float(g["loss"]) - 1)
    print(name, "wrong:", " ".join("%s %.2e" % kv for kv in wrong.items()))
    assert all(v > 100 * ROUND for v in wrong.values()), wrong


def test_float32_restatement_is_a_yardstick():
    """every tensor kind has a float32 error above zero somewhere in the pool, and none is absurd; the designed rows are there"""
    pool = DC.pool()
    print(pool)
    assert set(pool) == set(DC.KINDS) and all(0 < v < 1e-5 for v in pool.values()), pool
    c = DC.build("b65_k16_c33_zero")
    assert c["labels"][0].sum() == 0 and c["labels"][1].all() and not c["f_img"][DC.ZERO_ROW].any()
    r = DC.reference("b65_k16_c33_zero")
    big = np.abs(r["g_f_img"][DC.ZERO_ROW]).max()
    assert big > 1e6 * np.abs(r["nz_f_img"]).max() > 0                               # du / 1e-12: the eps branch sets the tensor's scale


def _cost(n, kind, seed=0):
    rng = np.random.default_rng(seed)
    if kind == "equal":
        return np.full((n, n), 2.5)
    if kind == "ties":
        return rng.integers(0, 3, (n, n)).astype(np.float64)
    return rng.random((n, n)) * 10 - 3


@pytest.mark.parametrize("n", [1, 2, 5, 6])
@pytest.mark.parametrize("kind", ["generic", "equal", "ties"])
def test_solver_equals_brute_force(n, kind):
    from xmh.models.dnph import assign_min_cost
    for seed in range(4):
        cost = _cost(n, kind, seed)
        cols = assign_min_cost(cost)
        assert cols.dtype == np.int32 and sorted(cols.tolist()) == list(range(n))
        best = min(sum(cost[i, p[i]] for i in range(n)) for p in itertools.permutations(range(n)))
        assert cost[np.arange(n), cols].sum() == pytest.approx(best, rel=1e-14, abs=0)       # on ties any optimal permutation passes


@pytest.mark.parametrize("n", [37, 128])
def test_solver_against_scipy(n):
    so = pytest.importorskip("scipy.optimize")
    from xmh.models.dnph import assign_min_cost, gene_noise
    rng = np.random.default_rng(n)
    cost = rng.random((n, n)) * 7
    cols = assign_min_cost(cost)
    rows, want = so.linear_sum_assignment(cost)
    assert sorted(cols.tolist()) == list(range(n))
    assert abs(cost[np.arange(n), cols].sum() - cost[rows, want].sum()) <= 1e-12 * cost[rows, want].sum()
    # the use it is put to: 8-bit noise vectors, so that several rows are duplicates -- the assigned matrix is what must agree
    h = np.tanh(rng.standard_normal((n, 8)) * 1.5).astype(np.float32)
    s = rng.integers(0, 2, (n, 8)) * 2 - 1
    assert len(np.unique(s, axis=0)) < n or n == 37
    d = np.stack([np.linalg.norm(h[i][None].repeat(n, 0) - s, axis=1) for i in range(n)])
    rows, want = so.linear_sum_assignment(d)
    assert np.array_equal(gene_noise(h, s), s[want].astype(np.float64))


@pytest.mark.parametrize("name", list(DC.GOLDEN_CASES))
def test_gene_noise_equals_the_reference(name):
    from xmh.models.dnph import gene_noise
    g = _golden(name)
    for m in ("img", "txt"):
        got = gene_noise(g["f_" + m], g["s_vector"])
        assert got.dtype == np.float64 and np.array_equal(got, g["noise_" + m])
        assert not np.array_equal(got, g["s_vector"])                                # the assignment is not the identity


def test_new_symbols_are_declared_exported_and_prototyped():
    from xmh import _lib
    header = open(os.path.join(ROOT, "include", "xmh.h")).read()
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header) and hasattr(so, name) and name in _lib.PROTOTYPES, name


def test_argument_errors_are_reported_without_a_gpu():
    from xmh import _lib
    L = _lib.lib
    one = ctypes.c_void_p(256)                                                       # never dereferenced: every call fails before a launch
    big = 1 << 24
    assert L.xmh_dnph_loss_ws_bytes(100, 16, 80, 80) > 0 and L.xmh_dnph_loss_ws_bytes(100, 16, 80, 79) == 0
    assert L.xmh_dnph_loss_ws_bytes(4097, 16, 80, 80) == 0 and L.xmh_dnph_loss_ws_bytes(4, 16, 0, 80) == 0
    need = L.xmh_dnph_loss_ws_bytes(4, 16, 5, 80)

    def loss(B=4, K=16, C=5, Cp=80, f=one, P=one, lab=one, ws=one, nbytes=big, out=one):
        return L.xmh_dnph_loss(f, one, one, one, P, B, K, C, Cp, lab, 1.0, 0.1, None, None, ws, nbytes, out, None)

    def grad(B=4, K=16, C=5, Cp=80, f=one, ws=one, nbytes=big, outs=(one,) * 5):
        return L.xmh_dnph_loss_grad(f, one, one, one, one, B, K, C, Cp, one, 1.0, 0.1, None, None, None, *outs, 0, ws, nbytes, None)

    for fn, who in ((loss, b"xmh_dnph_loss"), (grad, b"xmh_dnph_loss_grad")):
        assert fn(f=None) == -22 and who in L.xmh_last_error()
        assert fn(B=0) == -22 and fn(K=0) == -22 and fn(C=0) == -22
        assert fn(C=81) == -22 and b"Cp" in L.xmh_last_error()                      # fewer class logits than classes
        assert fn(B=4097) == -95 and fn(K=4097) == -95 and fn(C=1025, Cp=1025) == -95 and fn(Cp=1025) == -95
        assert fn(ws=None) == -22
        assert fn(nbytes=need - 1) == -12 and b"workspace" in L.xmh_last_error()
        assert fn(ws=ctypes.c_void_p(260)) == -22
    assert loss(P=None) == -22 and loss(lab=None) == -22 and loss(out=None) == -22
    assert grad(outs=(None,) * 5) == 0                                               # nothing asked for
    cost = (ctypes.c_double * 4)(1.0, 2.0, 3.0, 1.0)
    cols = (ctypes.c_int * 2)()
    assert L.xmh_assign_min_cost(cost, 2, cols) == 0 and list(cols) == [0, 1]
    assert L.xmh_assign_min_cost(None, 2, cols) == -22 and L.xmh_assign_min_cost(cost, 2, None) == -22
    assert L.xmh_assign_min_cost(cost, 0, cols) == -22 and L.xmh_assign_min_cost(cost, 4097, cols) == -95
    cost[2] = float("nan")
    assert L.xmh_assign_min_cost(cost, 2, cols) == -22 and b"finite" in L.xmh_last_error()

    def lin(B=4, E=64, N=80, w=one, ws=None, nbytes=0, outs=(one, one, one)):
        return L.xmh_linear_backward(w, one, one, B, E, N, *outs, 0, ws, nbytes, None)

    assert lin(w=None) == -22 and b"xmh_linear_backward" in L.xmh_last_error()
    assert lin(B=0) == -22 and lin(B=4097) == -95 and lin(E=2049) == -95 and lin(N=1025) == -95
    assert lin(ws=ctypes.c_void_p(260), nbytes=8) == -22 and lin(nbytes=8) == -22
    assert lin(outs=(None, None, None)) == 0


def test_model_and_runner_are_registered():
    import xmh.models  # noqa: F401
    import xmh.runners  # noqa: F401
    from xmh.common.register import registry
    from xmh.models.dnph import DNPH
    from xmh.runners.methods import DNPHTrainer
    assert registry.get_model_class("DNPH") is DNPH and registry.get_runner_class("DNPHTrainer") is DNPHTrainer
    assert DNPHTrainer.hash_scale == 1
    with pytest.raises(AssertionError, match="tanh"):
        DNPHTrainer(types.SimpleNamespace(model={"hash_func": "softmax"}))


def test_state_dict_defaults_and_generator():
    from xmh.models.dnph import DNPH
    from xmh.models.heads import DNPHHashLayer, DSPHLinearHash
    G = np.load(DC.GOLDEN)
    want = {k: tuple(int(n) for n in s.split(",")) for k, s in zip(G["head_state_keys"].tolist(), G["head_state_shapes"].tolist())}
    head = DNPHHashLayer(inputDim=512, outputDim=16)
    assert {k: tuple(v.shape) for k, v in head.state_dict().items()} == want and list(head.state_dict()) == list(want)
    head.load_state_dict({k: torch.full(s, 0.25) for k, s in want.items()}, strict=True)
    assert float(head.text_pre.fc.weight.detach()[3, 7]) == 0.25 and isinstance(head.image_hash, DSPHLinearHash)
    fresh = DNPHHashLayer(inputDim=64, outputDim=16)                                 # weights_init_kaiming: uniform fan_out, zero bias
    assert not fresh.image_hash.fc.bias.any() and not fresh.text_pre.fc.bias.any()
    assert float(fresh.image_pre.fc.weight.detach().abs().max()) <= (6.0 / 80) ** 0.5 and float(fresh.image_hash.fc.weight.detach().abs().max()) <= (6.0 / 16) ** 0.5
    assert torch.equal(fresh.quantization(torch.tensor([0.5])), torch.tanh(torch.tensor([0.5])))
    # the constructor's and from_config's defaults, the reference's quirk included
    sig = inspect.signature(DNPH.__init__).parameters
    assert (sig["outputDim"].default, sig["numclass"].default, sig["mrg"].default, sig["noise_alpha"].default) == (16, 80, 1.0, 0.1)
    state = np.random.get_state()[1].copy()
    cfg = types.SimpleNamespace(get=lambda k, d=None, _c={"clip_path": SMALL}: _c.get(k, d))
    m = DNPH.from_config(cfg, output_dim=16)
    assert (m.noise_alpha, m.loss.mrg, tuple(m.loss.proxies.shape), m.output_dim) == (1.0, 1.0, (80, 16), 16)
    assert tuple(m.hash.image_pre.fc.weight.shape) == (80, 64)
    keys = set(m.state_dict())
    assert "loss.proxies" in keys and {"hash." + k for k in want} <= keys and all(k.split(".")[0] in ("backbone", "hash", "loss") for k in keys)
    m2 = DNPH(cfg, clipPath=SMALL, numclass=24)
    assert m2.noise_alpha == 0.1 and tuple(m2.loss.proxies.shape) == (24, 16) and tuple(m2.hash.text_pre.fc.weight.shape) == (80, 64)
    # the proxies and the noise vectors come from the model's own generators: same seed, same draws, the global streams untouched
    assert torch.equal(m.loss.proxies[:24], DNPH(cfg, clipPath=SMALL, seed=0).loss.proxies[:24]) and 0.05 < float(m.loss.proxies.detach().std()) < 0.2
    a, b = m.rand_unit_rect(9, 16), m2.rand_unit_rect(9, 16)
    assert a.shape == (9, 16) and set(np.unique(a).tolist()) == {-1, 1} and np.array_equal(a, b) and not np.array_equal(a, m.rand_unit_rect(9, 16))
    assert np.array_equal(np.random.get_state()[1], state)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.loss(torch.zeros(3, 16), torch.zeros(3, 16), torch.zeros(3, 80), torch.zeros(3, 80), torch.ones(3, 80), torch.ones(3, 80))
    with pytest.raises(RuntimeError, match="numclass == batch size"):
        m.object_function(torch.zeros(3, 16), torch.zeros(3, 16), torch.zeros(3, 80), torch.zeros(3, 80))
