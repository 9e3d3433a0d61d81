"""The whole-training-step suite of MITH without a GPU: the float64 restatement of tests/mith_train_step_cases.py (which
tests/test_gpu_mith_train_step.py leans on) on the two cases, `narrow` and `wide`, five steps each.

Conditions on the inputs (not measurements of the port), asserted on the float64 run with its own selection at every step: the
clamp (max|Y[n] . x| over the four codes; measured at most 7.9 against 64 - GAP), the keep-set (the float32 restatement with its own
selection chooses the float64 run's keep-set in every step and modality -- zero entries differ --, and the smallest finite margin is
more than TOL_FACTOR = 4 times the largest score difference: narrow 1.51e-4 against 2.2e-6, 68 x; wide 7.2e-5 against 2.4e-6, 30 x),
and the empty concepts (between 8 and 28 (sample, concept) pairs without a kept token per step and modality).  The dataset seed 1814
meets them in both cases, so it stays.

Sets: backbone.logit_scale is the only parameter without a gradient, and the null set (max|g64| < 1e-10 at every step) is empty; the
smallest max|g64| of any tensor is 0.045 (narrow) and 0.0065 (wide).

The float32 run against the float64 run is the yardstick of the GPU module; here its figures are printed and held to a sanity bound
(finite, below 1e-2; measured: loss and terms <= 1.1e-6, grad / clipped <= 6.6e-6, m / v <= 8.6e-6, delta <= 2.0e-4, buffer <= 1.1e-6).

Structure of the float64 run: step 0 (rate 0) moves no parameter while m and v are filled; positional rows at or beyond L and token
ids absent from the batch have exact-zero gradients; buffer rows outside the batches seen so far equal the initial buffer and the
batch's rows hold tokens_hash_t; the scheduled rates are lr_f64 of each group.  Run with keeps= its own recorded sets, the restatement
reproduces itself to the bit."""
import math

import numpy as np
import pytest
import torch

import mith_train_step_cases as MS

_cache = {}


def _case(case, tmp_path_factory):
    """trainer on the CPU (model and loader only: nothing of it runs), the float64 and float32 runs with their own selection; once"""
    if case not in _cache:
        t = MS.trainer(case, tmp_path_factory.mktemp(case), "cpu")
        cap = MS.capture(t, case)
        assert t.model.hash.gcl_i is t.model.hash.gcl_t and not any(n.startswith("hash.gcl_t.") for n in cap["sd0"])
        r64 = MS.run(cap)
        r32 = MS.run(cap, dtype=torch.float32)
        per, pooled = MS.yardstick(cap, r64, r32)
        _cache[case] = dict(cap=cap, r64=r64, r32=r32, per=per, pool=pooled)
    return _cache[case]


@pytest.fixture(params=list(MS.CASES))
def case(request, tmp_path_factory):
    return request.param, _case(request.param, tmp_path_factory)


def test_the_inputs_meet_the_conditions_at_every_step(case):
    name, c = case
    assert len(c["r64"]) == MS.STEPS and len(c["cap"]["raw"]) == 3
    padded = [int(n) for b in c["cap"]["raw"] for n in b[2].sum(1)]
    print(name, "padded positions per caption", padded)
    assert min(padded) >= 1 and max(padded) < 32 and len(set(padded)) > 4               # masks that differ from row to row
    cond = MS.check_conditions(c["r64"], c["r32"])
    print("\n".join(MS.condition_lines(name, cond)))
    for g in MS.MODS:                                                                    # the selection is at work: neither all nor nothing
        for rec in c["r64"]:
            looked_at = np.isfinite(rec["margin"][g])
            assert 0 < rec["keep"][g][looked_at].mean() < 1 and not rec["keep"][g][~looked_at].any()


def test_the_sets_are_pinned(case):
    name, c = case
    r64 = c["r64"]
    assert MS.no_grad_set(c["cap"], r64) == ("backbone.logit_scale",)
    assert all(sorted(rec["grad"]) == sorted(r64[0]["grad"]) for rec in r64)
    small = min(float(np.abs(MS.dense(rec["grad"][k])).max()) for rec in r64 for k in rec["grad"])
    print(name, "null set", MS.null_set(r64), "smallest max|g64| of any tensor %.3e" % small)
    assert MS.null_set(r64) == () and small > 1e3 * MS.NULL_G


def test_float32_against_float64_is_an_fp32_error(case):
    name, c = case
    print("\n".join(MS.table(name, c["pool"])))
    worst = {}
    for (q, kind), e in c["pool"].items():
        worst[q] = max(worst.get(q, 0.0), e)
    print(name, "worst per quantity:", " ".join("%s %.2e" % kv for kv in sorted(worst.items())))
    assert set(worst) == {"loss", "terms", "buffer", "grad", "clipped", "delta", "m", "v"}
    for s, errs in enumerate(c["per"]):
        for key, e in errs.items():
            assert np.isfinite(e) and e < 1e-2, (name, s, key, e)
    assert all(e == 0.0 for (q, n), e in c["per"][0].items() if q == "delta")           # rate 0: the float32 run does not move either
    assert worst["grad"] > 2.0 ** -27                                                   # and it is a float32 run
    assert all(rec["p"][k].dtype == np.float32 and rec["Y"].dtype == np.float32 for rec in c["r32"] for k in rec["p"])


def test_structure_of_the_float64_run(case):
    name, c = case
    cap, r64 = c["cap"], c["r64"]
    init = MS.initial(cap["sd0"])
    Y0 = cap["Y0"].numpy().astype(np.float64)
    tok, pos = "backbone.token_embedding.weight", "backbone.positional_embedding"
    vocab = init[tok].shape[0]
    assert {MS.group_of(k) for k in r64[0]["grad"]} == {"backbone", "hash"} and init[pos].shape[0] > 32
    for s, rec in enumerate(r64):
        for group, lr in (("backbone", MS.OPT_CFG["backbone_lr"]), ("hash", MS.OPT_CFG["lr"])):
            want = 0.0 if s == 0 else lr * 0.5 * (1.0 + math.cos(math.pi * s / MS.STEPS))
            assert rec["lr"][group] == want and rec["count"] == s + 1, (s, group, rec["lr"])
            assert rec["next_lr"][group] == lr * 0.5 * (1.0 + math.cos(math.pi * (s + 1) / MS.STEPS))
        ids = cap["raw"][s % 3][1].numpy()
        absent = np.setdiff1d(np.arange(vocab), np.unique(ids))
        g_tok, g_pos = MS.dense(rec["grad"][tok]), MS.dense(rec["grad"][pos])
        assert not g_tok[absent].any() and g_tok.any() and not g_pos[ids.shape[1]:].any() and g_pos[0].any()
        written = MS.written_rows(cap, s)
        rest = np.setdiff1d(np.arange(MS.TRAIN_NUM), written)
        assert len(written) == min(4 * (s + 1), MS.TRAIN_NUM) and np.array_equal(rec["Y"][rest], Y0[rest])
        assert np.array_equal(rec["Y"][rec["rows"]], rec["outs"][6]) and np.array_equal(rec["rows"], np.arange(4 * (s % 3), 4 * (s % 3) + 4))
        if s > 0:                                                                       # rows of other batches keep an earlier step's codes
            other = np.setdiff1d(np.arange(MS.TRAIN_NUM), rec["rows"])
            assert np.array_equal(rec["Y"][other], r64[s - 1]["Y"][other])
        if s >= 3:                                                                      # the second visit writes other codes
            assert not np.array_equal(rec["Y"][rec["rows"]], r64[s - 3]["Y"][rec["rows"]])
    for k in r64[0]["grad"]:                                                            # step 0: rate 0
        assert np.array_equal(r64[0]["p"][k], init[k]), k
        assert MS.dense(r64[0]["m"][k]).any() and MS.dense(r64[0]["v"][k]).any(), k
        assert not np.array_equal(r64[1]["p"][k], r64[0]["p"][k]), k                    # and the next one moves everything
    # the shared module: one set of leaves received both modalities' gradients
    keys = {MS.head_key(k) for k in r64[0]["grad"] if k.startswith("hash.")}
    assert {g for g, _ in keys} == {"gcl", "i", "t"}
    assert {k for g, k in keys if g == "i"} == {k for g, k in keys if g == "t"}


def test_given_its_own_keep_sets_the_restatement_reproduces_itself_to_the_bit(case):
    name, c = case
    again = MS.run(c["cap"], keeps=MS.keeps_of(c["r64"]))
    for a, b in zip(c["r64"], again):
        assert a["loss"] == b["loss"] and np.array_equal(a["terms"], b["terms"]) and np.array_equal(a["Y"], b["Y"])
        for g in MS.MODS:
            assert np.array_equal(a["keep"][g], b["keep"][g]) and np.array_equal(a["scores"][g], b["scores"][g])
        for kind in ("grad", "clipped", "p", "m", "v"):
            assert sorted(a[kind]) == sorted(b[kind])
            assert all(np.array_equal(MS.dense(a[kind][k]), MS.dense(b[kind][k])) for k in a[kind]), kind
