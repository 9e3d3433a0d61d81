"""The whole-training-step suite of DIMCH without a GPU: the float64 restatement of tests/dimch_train_step_cases.py (which
tests/test_gpu_dimch_train_step.py leans on) on the two cases, `smooth` and `softmax`, five steps each.

Conditions on the inputs (not measurements of the port), asserted on the float64 run at every step; margin is the float64 distance
from the kink, noise the largest |float32 - float64| of the same quantity over the steps, and margin > TOL_FACTOR = 4 noise is asked.
Measured at the dataset seed 1828 -- smooth: hinge 5.95e-3 against 1.5e-6, 1 - s 0.67 against 5.6e-7, the four relus 3.4e-4 / 3.9e-4 /
3.1e-4 / 2.1e-4 against 6.2e-6 / 9.9e-6 / 4.0e-6 / 5.5e-6 (the narrowest ratio 39); softmax: hinge 8.1e-2 against 3.6e-7, 1 - s 0.64
against 4.4e-7, the gap behind a maximum 1.79e-4 against 1.1e-6 (guard 1e-4), the relus 8.7e-5 / 6.9e-4 / 2.0e-4 / 2.7e-4 against
6.6e-6 / 8.9e-6 / 6.7e-6 / 9.5e-6 (the narrowest ratio 13).  No relu decision differs in float32, every triplet term has between 7 and
14 live triplets, every row has a label.  The seed is the first from 1814 on that meets all of it in both cases: 1814 to 1827 each miss
in `softmax` -- nine of them on one of the 2560 gaps behind a hard maximum (inside dimch_cases' guard of 1e-4, 1814 with 9.8e-5, or
within four float32 differences), 1817, 1820, 1821 and 1826 on a relu pre-activation within four float32 differences of zero, 1819 on a
batch whose rows all share a label, so that no triplet is live -- and 1816, 1819 and 1826 miss in `smooth` too.

Sets: backbone.logit_scale is the only parameter without a gradient, and the null set (max|g64| < 1e-10 at every step) is empty; the
smallest max|g64| of any tensor is 0.19 (smooth) and 0.047 (softmax).

The float32 run against the float64 run is the yardstick of the GPU module; here its figures are printed and held to a sanity bound
(finite, below 1e-2; measured: loss and terms <= 9.2e-7, codes <= 6.3e-6, grad / clipped <= 1.0e-5, m / v <= 6.8e-6, delta <= 1.8e-4).

Structure of the float64 run: step 0 (rate 0) moves no parameter while m and v are filled; positional rows at or beyond L and token
ids absent from the batch have exact-zero gradients; the scheduled rates are lr_f64 of each group.  Run again with the same masks,
the restatement reproduces itself to the bit."""
import math

import numpy as np
import pytest
import torch

import dimch_train_step_cases as DS

_cache = {}
NULL = {"smooth": (), "softmax": ()}


def _case(case, tmp_path_factory):
    """trainer on the CPU (model and loader only: nothing of it runs), the float64 and float32 runs on the same masks; once"""
    if case not in _cache:
        t = DS.trainer(case, tmp_path_factory.mktemp(case), "cpu")
        cap = DS.capture(t, case)
        masks = DS.draw_masks(cap)
        r64 = DS.run(cap, masks)
        r32 = DS.run(cap, masks, dtype=torch.float32)
        null = DS.null_set(r64)
        per, pooled, _ = DS.yardstick(cap, r64, r32, null)
        _cache[case] = dict(cap=cap, masks=masks, r64=r64, r32=r32, per=per, pool=pooled, null=null)
    return _cache[case]


@pytest.fixture(params=list(DS.CASES))
def case(request, tmp_path_factory):
    return request.param, _case(request.param, tmp_path_factory)


def test_the_inputs_meet_the_conditions_at_every_step(case):
    name, c = case
    assert len(c["r64"]) == DS.STEPS and len(c["cap"]["raw"]) == 3
    cond = DS.check_conditions(c["cap"], c["r64"], c["r32"])
    print("\n".join(DS.condition_lines(name, cond)))
    if name == "smooth":                                                                # a mask per head and step, neither all nor nothing
        assert len(c["masks"]) == DS.STEPS and all(tuple(k.shape) == (DS.B * 3, 32) and 0.5 < float(k.float().mean()) < 0.9 for ms in c["masks"] for k in ms)
        assert not torch.equal(c["masks"][0][0], c["masks"][0][1]) and not torch.equal(c["masks"][0][0], c["masks"][1][0])
    else:
        assert c["masks"] is None and c["r64"][0]["outs"][1].shape == (DS.B, 24) and "gap" in cond
        np.testing.assert_allclose(c["r64"][0]["outs"][1].reshape(DS.B, 12, 2).sum(-1), 1.0, rtol=0, atol=1e-12)
    for rec in c["r64"]:                                                                # both relus are at work in both heads
        assert all(0.05 < float((z > 0).mean()) < 0.95 for mod in DS.MODS for z in rec["pre"][mod])


def test_the_sets_are_pinned(case):
    name, c = case
    r64 = c["r64"]
    assert DS.no_grad_set(c["cap"], r64) == ("backbone.logit_scale",)
    assert all(sorted(rec["grad"]) == sorted(r64[0]["grad"]) for rec in r64)
    small = min((float(np.abs(DS.dense(rec["grad"][k])).max()), k) for rec in r64 for k in rec["grad"] if k not in c["null"])
    print(name, "null set", c["null"], "smallest max|g64| of any other tensor %.3e (%s)" % small)
    assert c["null"] == NULL[name] and small[0] > 1e3 * DS.NULL_G


def test_float32_against_float64_is_an_fp32_error(case):
    name, c = case
    print("\n".join(DS.table(name, c["pool"])))
    worst = {}
    for (q, kind), e in c["pool"].items():
        worst[q] = max(worst.get(q, 0.0), e)
    print(name, "worst per quantity:", " ".join("%s %.2e" % kv for kv in sorted(worst.items())))
    assert set(worst) == {"loss", "terms", "codes", "grad", "clipped", "delta", "m", "v"}
    for s, errs in enumerate(c["per"]):
        for key, e in errs.items():
            assert np.isfinite(e) and e < 1e-2, (name, s, key, e)
    assert all(e == 0.0 for (q, n), e in c["per"][0].items() if q == "delta")           # rate 0: the float32 run does not move either
    assert worst["grad"] > 2.0 ** -27                                                   # and it is a float32 run
    assert all(rec["p"][k].dtype == np.float32 for rec in c["r32"] for k in rec["p"])


def test_structure_of_the_float64_run(case):
    name, c = case
    cap, r64 = c["cap"], c["r64"]
    sd0 = cap["sd0"]
    tok, pos = "backbone.token_embedding.weight", "backbone.positional_embedding"
    vocab = sd0[tok].shape[0]
    assert {DS.group_of(k) for k in r64[0]["grad"]} == {"backbone", "hash"} and sd0[pos].shape[0] > 32
    assert sum(k.startswith("hash.") for k in r64[0]["grad"]) == 12
    for s, rec in enumerate(r64):
        for group, lr in (("backbone", DS.OPT_CFG["backbone_lr"]), ("hash", DS.OPT_CFG["lr"])):
            want = 0.0 if s == 0 else lr * 0.5 * (1.0 + math.cos(math.pi * s / DS.STEPS))
            assert rec["lr"][group] == want and rec["count"] == s + 1, (s, group, rec["lr"])
            assert rec["next_lr"][group] == lr * 0.5 * (1.0 + math.cos(math.pi * (s + 1) / DS.STEPS))
        ids = cap["raw"][s % 3][1].numpy()
        absent = np.setdiff1d(np.arange(vocab), np.unique(ids))
        g_tok, g_pos = DS.dense(rec["grad"][tok]), DS.dense(rec["grad"][pos])
        assert not g_tok[absent].any() and g_tok.any() and not g_pos[ids.shape[1]:].any() and g_pos[0].any()
        assert rec["terms"][0] == rec["loss"] and np.isfinite(rec["terms"]).all()
    for k in r64[0]["grad"]:                                                            # step 0: rate 0
        assert np.array_equal(r64[0]["p"][k], sd0[k].numpy().astype(np.float64)), k
        if k not in c["null"]:
            assert DS.dense(r64[0]["m"][k]).any() and DS.dense(r64[0]["v"][k]).any(), k
            assert not np.array_equal(r64[1]["p"][k], r64[0]["p"][k]), k                # and the next one moves everything


def test_given_the_same_masks_the_restatement_reproduces_itself_to_the_bit(case):
    name, c = case
    again = DS.run(c["cap"], c["masks"])
    for a, b in zip(c["r64"], again):
        assert a["loss"] == b["loss"] and np.array_equal(a["terms"], b["terms"])
        assert all(np.array_equal(x, y) for x, y in zip(a["outs"], b["outs"]))
        for kind in ("grad", "clipped", "p", "m", "v"):
            assert sorted(a[kind]) == sorted(b[kind])
            assert all(np.array_equal(DS.dense(a[kind][k]), DS.dense(b[kind][k])) for k in a[kind]), kind
