"""The whole-training-step suite of DNPH without a GPU: the float64 restatement of tests/dnph_train_step_cases.py (which
tests/test_gpu_dnph_train_step.py leans on) on the two cases, `plain` and `wide`, five steps each.

Conditions on the inputs (not measurements of the port), asserted on the float64 run at every step.  The assignment: the best of the
24 permutations lies below the second best by more than TOL_FACTOR = 4 times the largest float32-against-float64 change of any
permutation's total, and the float32 run takes the same permutation -- measured at the dataset seed 1814, the smallest gap against the
largest change over the ten assignments of a case: plain 2.41e-2 against 4.5e-6 (5300 x), wide 1.11e-2 against 6.9e-6 (1600 x).  The
smallest row norm of a code or proxy is 0.365 (plain) and 0.545 (wide) against 1e-6, every row has a label.  Seed 1814 meets all of it
in both cases, so it stays.

Sets: backbone.logit_scale is the only parameter without a gradient, and the null set (max|g64| < 1e-10 at every step) is empty; the
smallest max|g64| of any tensor is 0.046 (plain) and 0.038 (wide), both of hash.text_hash.fc.bias.  The 80 - 6 prediction rows that are
never a target still receive the softmax's gradient.

The float32 run against the float64 run is the yardstick of the GPU module; here its figures are printed and held to a sanity bound
(finite, below 1e-2; measured: loss <= 1.2e-7, terms <= 4.1e-7, codes <= 9.2e-6, grad / clipped <= 6.8e-6, m / v <= 6.5e-6, delta <= 1.9e-4).

Structure of the float64 run: step 0 (rate 0) moves no BertAdam parameter while m and v are filled, and the proxies, whose SGD has no
schedule, move by -lr g at every step; positional rows at or beyond L and token ids absent from the batch have exact-zero gradients;
the scheduled rates are lr_f64 of each group.  Run with perms= its own recorded assignments, the restatement reproduces itself to the
bit.  Where scipy is importable the brute-force assignment equals scipy.optimize.linear_sum_assignment's."""
import math

import numpy as np
import pytest
import torch

import dnph_train_step_cases as NS

_cache = {}
NULL = {"plain": (), "wide": ()}


def _case(case, tmp_path_factory):
    """trainer on the CPU (model and loader only: nothing of it runs), the float64 and float32 runs with their own assignments; once"""
    if case not in _cache:
        t = NS.trainer(case, tmp_path_factory.mktemp(case), "cpu")
        cap = NS.capture(t, case)
        assert t.model.noise_alpha == NS.NOISE_ALPHA and t.model.loss.mrg == NS.MRG and float(t.model.hash.image_hash.drop_out.p) == NS.DROP_P
        masks, noises = NS.draw_masks(cap), NS.draw_noises(cap)
        r64 = NS.run(cap, masks, noises)
        r32 = NS.run(cap, masks, noises, dtype=torch.float32)
        null = NS.null_set(r64)
        per, pooled, _ = NS.yardstick(cap, r64, r32, null)
        _cache[case] = dict(cap=cap, masks=masks, noises=noises, r64=r64, r32=r32, per=per, pool=pooled, null=null)
    return _cache[case]


@pytest.fixture(params=list(NS.CASES))
def case(request, tmp_path_factory):
    return request.param, _case(request.param, tmp_path_factory)


def test_the_inputs_meet_the_conditions_at_every_step(case):
    name, c = case
    K = c["cap"]["K"]
    assert len(c["r64"]) == NS.STEPS and len(c["cap"]["raw"]) == 3
    cond = NS.check_conditions(c["r64"], c["r32"])
    print("\n".join(NS.condition_lines(name, cond)))
    assert all(tuple(k.shape) == (NS.B, K) and 0.5 < float(k.float().mean()) < 1.0 for ms in c["masks"] for k in ms)
    assert all(n.shape == (NS.B, K) and set(np.unique(n)) == {-1, 1} for n in c["noises"]) and not np.array_equal(c["noises"][0], c["noises"][1])
    perms = [p for rec in c["r64"] for p in rec["perm"].values()]
    assert len(set(perms)) > 3 and any(p != 0 for p in perms)                           # the identity would not pass for the assignment
    assert any(rec["perm"]["img"] != rec["perm"]["txt"] for rec in c["r64"])            # nor the image's for the text's
    assert c["r64"][0]["outs"][2].shape == (NS.B, NS.CP) and NS.CP > NS.C
    assert any(int(np.argmax(row)) != int(np.flatnonzero(row)[-1]) for rec in c["r64"] for row in rec["labels"])   # a row with two labels


def test_the_sets_are_pinned(case):
    name, c = case
    r64 = c["r64"]
    assert NS.no_grad_set(c["cap"], r64) == ("backbone.logit_scale",)
    assert all(sorted(rec["grad"]) == sorted(r64[0]["grad"]) for rec in r64)
    assert all(NS.PROXIES in rec["grad"] and NS.PROXIES in rec["p"] and not any(NS.PROXIES in rec[k] for k in ("clipped", "m", "v")) for rec in r64)
    small = min((float(np.abs(NS.dense(rec["grad"][k])).max()), k) for rec in r64 for k in rec["grad"] if k not in c["null"])
    print(name, "null set", c["null"], "smallest max|g64| of any other tensor %.3e (%s)" % small)
    assert c["null"] == NULL[name] and small[0] > 1e3 * NS.NULL_G


def test_float32_against_float64_is_an_fp32_error(case):
    name, c = case
    print("\n".join(NS.table(name, c["pool"])))
    worst = {}
    for (q, kind), e in c["pool"].items():
        worst[q] = max(worst.get(q, 0.0), e)
    print(name, "worst per quantity:", " ".join("%s %.2e" % kv for kv in sorted(worst.items())))
    assert set(worst) == {"loss", "terms", "codes", "grad", "clipped", "delta", "m", "v"}
    for s, errs in enumerate(c["per"]):
        for key, e in errs.items():
            assert np.isfinite(e) and e < 1e-2, (name, s, key, e)
    assert all(e == 0.0 for (q, n), e in c["per"][0].items() if q == "delta" and n != NS.PROXIES)   # rate 0: the float32 run does not move either
    assert worst["grad"] > 2.0 ** -27                                                   # and it is a float32 run
    assert all(rec["p"][k].dtype == np.float32 for rec in c["r32"] for k in rec["p"])


def test_structure_of_the_float64_run(case):
    name, c = case
    cap, r64 = c["cap"], c["r64"]
    sd0 = cap["sd0"]
    tok, pos = "backbone.token_embedding.weight", "backbone.positional_embedding"
    vocab = sd0[tok].shape[0]
    assert {NS.group_of(k) for k in r64[0]["grad"]} == {"backbone", "hash", "sgd"} and sd0[pos].shape[0] > 32
    before = sd0[NS.PROXIES].numpy().astype(np.float64)
    for s, rec in enumerate(r64):
        for group, lr in (("backbone", NS.OPT_CFG["backbone_lr"]), ("hash", NS.OPT_CFG["lr"])):
            want = 0.0 if s == 0 else lr * 0.5 * (1.0 + math.cos(math.pi * s / NS.STEPS))
            assert rec["lr"][group] == want and rec["count"] == s + 1, (s, group, rec["lr"])
            assert rec["next_lr"][group] == lr * 0.5 * (1.0 + math.cos(math.pi * (s + 1) / NS.STEPS))
        assert "sgd" not in rec["lr"]
        ids = cap["raw"][s % 3][1].numpy()
        absent = np.setdiff1d(np.arange(vocab), np.unique(ids))
        g_tok, g_pos = NS.dense(rec["grad"][tok]), NS.dense(rec["grad"][pos])
        assert not g_tok[absent].any() and g_tok.any() and not g_pos[ids.shape[1]:].any() and g_pos[0].any()
        assert rec["terms"][0] == rec["loss"] and np.isfinite(rec["terms"]).all()
        assert np.array_equal(rec["p"][NS.PROXIES], before - NS.PROXY_LR * rec["grad"][NS.PROXIES]) and rec["grad"][NS.PROXIES].any()
        before = rec["p"][NS.PROXIES]
    for k in r64[0]["m"]:                                                               # step 0: rate 0
        assert np.array_equal(r64[0]["p"][k], sd0[k].numpy().astype(np.float64)), k
        if k not in c["null"]:
            assert NS.dense(r64[0]["m"][k]).any() and NS.dense(r64[0]["v"][k]).any(), k
            assert not np.array_equal(r64[1]["p"][k], r64[0]["p"][k]), k                # and the next one moves everything


def test_given_its_own_assignments_the_restatement_reproduces_itself_to_the_bit(case):
    name, c = case
    again = NS.run(c["cap"], c["masks"], c["noises"], perms=NS.perms_of(c["r64"]))
    for a, b in zip(c["r64"], again):
        assert a["loss"] == b["loss"] and np.array_equal(a["terms"], b["terms"]) and a["perm"] == b["perm"]
        assert all(np.array_equal(x, y) for x, y in zip(a["outs"], b["outs"]))
        for kind in ("grad", "clipped", "p", "m", "v"):
            assert sorted(a[kind]) == sorted(b[kind])
            assert all(np.array_equal(NS.dense(a[kind][k]), NS.dense(b[kind][k])) for k in a[kind]), kind


def test_the_brute_force_assignment_is_scipys(case):
    optimize = pytest.importorskip("scipy.optimize")
    name, c = case
    for s, rec in enumerate(c["r64"]):
        for mod, code in zip(NS.MODS, rec["outs"][:2]):
            h, n = code.astype(np.float64), c["noises"][s].astype(np.float64)
            cost = np.sqrt(((h[:, None, :] - n[None, :, :]) ** 2).sum(-1))
            rows, cols = optimize.linear_sum_assignment(cost)
            assert rows.tolist() == list(range(NS.B)) and cols.tolist() == NS.PERMS[rec["perm"][mod]].tolist(), (s, mod)
