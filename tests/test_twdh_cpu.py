"""No GPU: the float64 restatement of TwDH's objective (tests/twdh_cases.py) against the golden of the reference's own compute_loss
(tests/golden/twdh_loss.npz, tools/make_golden_twdh_loss.py), the new C symbols, their argument errors, and what the Python layer
refuses.

Tolerance against the golden: the reference's numbers are float32 results of expressions a handful of operations deep and of
pairwise means, so the float64 restatement on the same inputs is expected within ROUND = 16 eps32 of them: every scalar relative to
itself, every gradient relative to its largest entry, once whole (the saturated entries, 0.5 / 1e-12 / n, set the scale) and once
with the saturated entries zeroed on both sides (the ordinary entries at their own scale).  Measured: 1.8e-7 at most."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import twdh_cases as TC
from conftest import ROOT

ROUND = 16 * float(np.finfo(np.float32).eps)
NEW = ("xmh_twdh_targets", "xmh_twdh_loss_ws_bytes", "xmh_twdh_loss", "xmh_twdh_loss_grad", "xmh_twdh_short_forward", "xmh_twdh_short_backward")
SMALL = "synthetic:1814:vision_layers=1,transformer_layers=1,vision_width=128,transformer_width=128,embed_dim=64,image_resolution=64"


def _golden(name):
    G = np.load(TC.GOLDEN)
    return {k.split("__", 1)[1]: G[k] for k in G.files if k.startswith(name + "__")}


@pytest.mark.parametrize("name", TC.GOLDEN_CASES)
def test_restatement_reproduces_the_reference(name):
    g = _golden(name)
    lens = tuple(int(k) for k in g["lens"])
    centres, ties = [g["centre_%d" % i] for i in range(len(lens))], [g["tie_%d" % i] for i in range(len(lens))]
    bits = TC.targets(g["labels"], centres, ties)
    assert np.array_equal(bits, g["bits"])
    s = g["labels"].astype(np.int64) @ np.concatenate(centres, 1).astype(np.int64)
    assert ((s == 0) & (g["labels"].sum(1) > 0)[:, None]).any(), "the case has no tie"
    if name == "small":
        assert g["labels"][0].sum() == 0 and not bits[0].any()                       # the reference's NaN mean: every bit off
    qa, lr = float(g["quan_alpha"]), float(g["low_rate"])
    terms = TC.loss(g["img_long"], g["img_short"], g["txt_long"], g["txt_short"], bits, lens, qa, lr).numpy()
    known = ~np.isnan(g["terms"])
    assert known.sum() == 5 + 2 * (len(lens) - 1) and np.isfinite(terms).all()
    worst = {"terms": float(np.abs(terms[known] / g["terms"][known] - 1).max())}       # every recorded scalar at its own scale
    flipped = {}
    for m in ("img", "txt"):
        grads = dict(zip(("long", "short"), TC.loss_grad(g[m + "_long"], g[m + "_short"], bits, lens, qa, lr, 1.0)))
        wrong = dict(zip(("long", "short"), TC.loss_grad(g[m + "_long"], g[m + "_short"], bits, lens, -qa, 1.01 * lr, 1.0)))
        for which in ("long", "short"):
            gold, sat = g["d_%s_%s" % (m, which)], TC.saturated(g["%s_%s" % (m, which)])
            assert sat.sum() == 6 and np.abs(gold[sat]).max() > 0.4 / 1e-12 / gold.size  # the saturated entries: 0.5 / 1e-12 / n
            worst["d_%s_%s" % (which, m)] = TC.rel_err(grads[which].numpy(), gold)
            # the ordinary entries at their own scale: the saturated ones zeroed on both sides
            worst["ord_%s_%s" % (which, m)] = TC.rel_err(np.where(sat, 0, grads[which].numpy()), np.where(sat, 0, gold))
            flipped["ord_%s_%s" % (which, m)] = TC.rel_err(np.where(sat, 0, wrong[which].numpy()), np.where(sat, 0, gold))
    print(name, " ".join("%s %.2e" % kv for kv in worst.items()))
    assert all(v <= ROUND for v in worst.values()), worst
    # what the ordinary entries are there for: a wrong sign of the quantisation part, or a weight 1 % off, is far outside ROUND
    assert all(v > 100 * ROUND for v in flipped.values()), flipped


def test_pack_bits_and_pair_targets():
    bits = np.zeros((2, 44), np.uint8)
    bits[0, [0, 31, 32, 43]] = 1
    bits[1, 5] = 1
    w = TC.pack_bits(bits)
    assert w.dtype == np.uint32 and w.shape == (2, 2) and w.tolist() == [[0x80000001, 0x801], [0x20, 0]]
    assert TC.pair_targets(np.array([[0, 1]]), torch.float64).tolist() == [[1.0, 0.0, 0.0, 1.0]]


def test_float32_restatement_is_a_yardstick():
    """every tensor kind has a float32 error above zero somewhere in the pool, and none is absurd"""
    pool = TC.pool()
    print(pool)
    assert set(pool) == set(TC.KINDS) and all(0 < v < 1e-5 for v in pool.values()), pool
    c = TC.build("b65_c80")
    s = c["labels"].astype(np.int64) @ np.concatenate(c["centres"], 1).astype(np.int64)
    assert ((s == 0) & (c["labels"].sum(1) > 0)[:, None]).any() and c["labels"][0].sum() == 0 and c["labels"][1].all()
    p = TC.short_forward(c["img_long"], c["T"], torch.float32).numpy()             # in float32 exp(-160) is an exact zero
    assert (p[:, :4] == (1, 0, 0, 1)).all(), "no saturated pairs from the offset transform columns"


def test_new_symbols_are_declared_exported_and_prototyped():
    from xmh import _lib
    header = open(os.path.join(ROOT, "include", "xmh.h")).read()
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header) and hasattr(so, name) and name in _lib.PROTOTYPES, name
    assert "XMH_TWDH_MAX_STREAMS %d" % _lib.TwdhStreams.MAX in header


def test_argument_errors_are_reported_without_a_gpu():
    from xmh import _lib
    L = _lib.lib
    one = ctypes.c_void_p(256)                                                       # never dereferenced: every call fails before a launch
    assert L.xmh_twdh_targets(None, 1, None, None, 1, 1, None, None) == -22 and b"xmh_twdh_targets" in L.xmh_last_error()
    assert L.xmh_twdh_targets(one, 0, one, one, 1, 1, one, None) == -22
    assert L.xmh_twdh_targets(one, 1025, one, one, 1, 1, one, None) == -95
    assert L.xmh_twdh_targets(one, 1, one, one, 1, 4097, one, None) == -95
    st = _lib.TwdhStreams()
    st.n = 2
    st.bit[0], st.K[0], st.bit[1], st.K[1] = 0, 32, 32, 4
    ref = ctypes.byref(st)
    assert L.xmh_twdh_loss_ws_bytes(65, 2) == 256 and L.xmh_twdh_loss_ws_bytes(4097, 2) == 0
    assert L.xmh_twdh_loss(None, one, one, one, one, one, 4, 0.5, 0.0, one, one, 1 << 20, None) == -22
    assert L.xmh_twdh_loss(ref, one, one, one, one, None, 4, 0.5, 0.0, one, one, 1 << 20, None) == -22
    assert L.xmh_twdh_loss(ref, one, None, one, one, one, 4, 0.5, 0.0, one, one, 1 << 20, None) == -22      # image without its shorts
    assert L.xmh_twdh_loss(ref, one, one, one, one, one, 4, 0.5, 0.0, one, one, 8, None) == -12 and b"workspace" in L.xmh_last_error()
    assert L.xmh_twdh_loss(ref, one, one, one, one, one, 4097, 0.5, 0.0, one, one, 1 << 20, None) == -95
    assert L.xmh_twdh_loss(ref, ctypes.c_void_p(260), one, one, one, one, 4, 0.5, 0.0, one, one, 1 << 20, None) == -22
    st.bit[1] = 30                                                                   # the streams must tile the bits in order
    assert L.xmh_twdh_loss(ref, one, one, one, one, one, 4, 0.5, 0.0, one, one, 1 << 20, None) == -22
    assert L.xmh_twdh_loss_grad(ref, one, one, one, 4, 0.5, 0.0, None, one, one, None) == -22
    st.bit[1], st.n = 32, 9
    assert L.xmh_twdh_loss_grad(ref, one, one, one, 4, 0.5, 0.0, None, one, one, None) == -95
    st.n = 2
    assert L.xmh_twdh_loss_grad(ref, None, one, one, 4, 0.5, 0.0, None, one, one, None) == -22
    assert L.xmh_twdh_loss_grad(ref, one, one, one, 4, 0.5, 0.0, None, None, None, None) == 0                # nothing asked for
    assert L.xmh_twdh_short_forward(None, one, 4, 64, 24, one, None) == -22
    assert L.xmh_twdh_short_forward(one, one, 4, 63, 24, one, None) == -22
    assert L.xmh_twdh_short_forward(one, one, 4097, 64, 24, one, None) == -95
    assert L.xmh_twdh_short_backward(one, one, one, 4, 64, 24, one, 0, None, 0, None) == -22
    assert L.xmh_twdh_short_backward(one, one, one, 4, 64, 24, one, 0, one, 4 * 4 * 24 - 1, None) == -12
    assert L.xmh_twdh_short_backward(one, one, one, 0, 64, 24, one, 0, one, 1 << 20, None) == -22


def _model(**over):
    from xmh.models.twdh import TwDH
    kw = dict(cfg=None, long_dim=32, clipPath=SMALL, trans="synthetic", short_dims=[4, 8], long_center="synthetic", short_center="synthetic",
              num_classes=12)
    kw.update(over)
    return TwDH(**kw)


def test_python_layer_without_a_gpu(tmp_path):
    from xmh.models.twdh import TwDH
    from xmh.runners.methods import TwDHTrainer
    m = _model()
    assert tuple(m.long_center.shape) == (12, 32) and list(m.short_center) == ["4", "8"] and tuple(m.short_center["8"].shape) == (12, 8)
    assert set(m.long_center.unique().tolist()) == {-1.0, 1.0} and torch.equal(m.long_center, _model().long_center)
    codes = (torch.rand(3, 64), torch.rand(3, 64), {"4": torch.rand(3, 8), "8": torch.rand(3, 16)}, {"4": torch.rand(3, 8), "8": torch.rand(3, 16)})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.object_function(*codes)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.soft_argmax_hash_loss(codes[0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m._short_train(codes[0])
    # the reference's draws, in its order: the long centre, then the short ones
    torch.manual_seed(7)
    want = [torch.randint_like(c[0], 2) * 2 - 1 for c in [m.long_center, m.short_center["4"], m.short_center["8"]]]
    torch.manual_seed(7)
    ties = m.draw_ties()
    assert list(ties) == ["long", "4", "8"] and all(torch.equal(a, b) for a, b in zip(ties.values(), want))
    # no centres: the defaults' paths do not exist
    bare = _model(long_center="./no/such/32.pkl", short_center="./no/such")
    assert bare.long_center is None and bare.short_center == {}
    with pytest.raises(ValueError, match="long_center.*short_center"):
        bare.object_function(*codes)
    # centre files by the reference's path rules; a key the transforms do not have
    os.makedirs(os.path.join(str(tmp_path), "long"))
    os.makedirs(os.path.join(str(tmp_path), "short"))
    torch.save(m.long_center.long(), os.path.join(str(tmp_path), "long", "32.pkl"))          # the shipped long centres are int64
    torch.save(m.short_center["4"], os.path.join(str(tmp_path), "short", "4.pkl"))
    torch.save(m.short_center["8"], os.path.join(str(tmp_path), "short", "16.pkl"))
    cfg = types.SimpleNamespace(get=lambda k, d=None, _c={"long_dim": 32, "clip_path": SMALL, "trans_matrix": "synthetic", "short_dims": [4, 8],
                                                           "long_center": os.path.join(str(tmp_path), "long"),
                                                           "short_center": os.path.join(str(tmp_path), "short")}: _c.get(k, d))
    loaded = TwDH.from_config(cfg, output_dim=4)
    assert loaded.long_center.dtype == torch.float32 and torch.equal(loaded.long_center, m.long_center) and sorted(loaded.short_center) == ["16", "4"]
    with pytest.raises(ValueError, match="short_center.*trans_matrix"):
        loaded.object_function(*codes)
    one = _model(short_center=os.path.join(str(tmp_path), "short", "4.pkl"))                 # a single file: its stem is the key
    assert list(one.short_center) == ["4"]
    # a centre with an entry other than +-1 is refused at load time
    bad = m.long_center.clone()
    bad[3, 5] = 0
    torch.save(bad, os.path.join(str(tmp_path), "long", "32.pkl"))
    with pytest.raises(ValueError, match=r"\+1 / -1"):
        TwDH.from_config(cfg, output_dim=4)
    # the two pinned refusals, and where they point
    with pytest.raises(NotImplementedError, match="TwDH.*forward_train_codes"):
        TwDH.forward_train(types.SimpleNamespace(), None, None)
    with pytest.raises(NotImplementedError, match="TwDH's head.*train_epoch_codes"):
        TwDHTrainer.train_epoch(types.SimpleNamespace(), 0)
    assert all(callable(getattr(TwDHTrainer, n)) for n in ("train_epoch_codes", "train", "compute_loss"))
