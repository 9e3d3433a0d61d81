"""The whole-training-step suite of TwDH without a GPU: the float64 restatement of tests/twdh_train_step_cases.py (which
tests/test_gpu_twdh_train_step.py leans on) on the two cases, `rated` and `shipped`, five steps each.

Conditions on the inputs (not measurements of the port), asserted on the float64 run at every step: every fc2 pre-activation of
both heads lies outside its tie bound (measured: at least 90 tie bounds, rated, image head, step 2; 91 in shipped, step 3), the
smallest p (1 - p) over the four probability matrices is at least 1e-3 (measured: at least 0.093), steps 0, 2 and 4 run on the batch
whose one two-label row gives tie bits (29 of 224 in rated, 42 of 368 in shipped, between 15 and 22 of them set, so they fall both
ways) and steps 1 and 3 on the batch without any, and the float32 restatement's target bits equal the float64 run's.  The dataset
seed 1814 and TIE_SEED 1814 meet them in both cases, so they stay.

Sets: backbone.logit_scale is the only parameter without a gradient; the null set (max|g64| < 1e-10 at every step) is the DCMHT
three, the biases in front of the image head's BatchNorm.

The float32 run against the float64 run is the yardstick of the GPU module; here its figures are printed and held to a sanity bound
(finite, below 1e-2; measured: loss and terms <= 1.4e-7, codes <= 1.7e-6, grad / clipped / m / v <= 4.1e-5, delta <= 5.4e-4,
running statistics <= 3.4e-7), and its null-set deltas to the budget the GPU module gives the port's (null_delta_budget).

Structure of the float64 run: the set of parameters with a gradient; the scheduled rates are lr_f64 of each group; absent token ids
and positional rows at or beyond L have exact-zero gradients; the q and k thirds of the heads' in_proj have exact-zero gradients;
BatchNorm's batch count; step 0 (rate 0) moves no parameter while m and v are filled and step 1 moves everything.  In `shipped` the
total is the long terms alone while the short terms of the vector are non-zero; in `rated` the way through the transforms is a
visible share of the long code's gradient.  Given its own target bits and relu masks the restatement reproduces itself to the bit;
its objective at step 0 is twdh_cases.loss / loss_grad on the same probabilities; the replayed ties are what model.draw_ties()
returns after the same seed."""
import math

import numpy as np
import pytest
import torch

import twdh_cases as TC
import twdh_train_step_cases as WS

_cache = {}


def _case(case, tmp_path_factory):
    """trainer on the CPU (model and loader only: nothing of it trains), the float64 and float32 runs, the null set, the yardstick; once"""
    if case not in _cache:
        t = WS.trainer(case, tmp_path_factory.mktemp(case), "cpu")
        cap = WS.capture(t, case)
        named = [n for n, _ in t.model.named_parameters()]
        r64 = WS.run(cap)
        r32 = WS.run(cap, dtype=torch.float32)
        null = WS.null_set(r64)
        per, pooled, noise = WS.yardstick(cap, r64, r32, null)
        _cache[case] = dict(t=t, cap=cap, named=named, r64=r64, r32=r32, null=null, per=per, pool=pooled, noise=noise)
    return _cache[case]


@pytest.fixture(params=list(WS.CASES))
def case(request, tmp_path_factory):
    return request.param, _case(request.param, tmp_path_factory)


def test_the_cases_are_the_ones_stated():
    for name, lens, ktot, starts, low_rate in (("rated", (32, 8, 16), 56, (0, 32, 40), 0.3), ("shipped", (64, 4, 8, 16), 92, (0, 64, 68, 76), 0)):
        c = WS.CASES[name]
        o = WS.offsets(c["lens"])
        assert c["lens"] == lens and c["low_rate"] == low_rate and o[-1] == ktot and tuple(o[:-1]) == starts and ktot % 32 != 0
    assert any(s % 32 for s in WS.offsets(WS.CASES["shipped"]["lens"])[1:-1])          # streams that start inside a target word
    assert (WS.STEPS, WS.B, WS.C, WS.QUAN_ALPHA, WS.TOL_FACTOR) == (5, 4, 6, 0.5, 4.0)
    assert WS.OPT_CFG == {"lr": 0.002, "backbone_lr": 0.0005, "e": 1e-3} and WS.ADAM["t_total"] == 5


def test_the_inputs_meet_the_conditions_at_every_step(case):
    name, c = case
    assert len(c["r64"]) == WS.STEPS and len(c["cap"]["batches"]) == 2
    cond = WS.check_conditions(c["r64"], WS.bits_of(c["r32"]))
    print("\n".join(WS.condition_lines(name, cond)))
    n = sum(c["cap"]["lens"])
    assert all(rec["bits"].shape == (WS.B, n) and set(np.unique(rec["bits"])) <= {0, 1} for rec in c["r64"])
    assert [cond[(s, "ties")][0] > 0 for s in range(WS.STEPS)] == [True, False, True, False, True]
    # the same batch draws other ties at another step: the per-step draw shows in the targets
    assert not np.array_equal(c["r64"][0]["bits"], c["r64"][2]["bits"]) and np.array_equal(c["r64"][1]["bits"], c["r64"][3]["bits"])


def test_the_sets_are_pinned(case):
    name, c = case
    r64 = c["r64"]
    assert c["null"] == WS.NULL_TWDH
    others = [n for n in r64[0]["grad"] if n not in c["null"]]
    small = min(float(np.abs(WS.dense(rec["grad"][n])).max()) for rec in r64 for n in others)
    print(name, "null set", c["null"], "float64 max|g|", [["%.1e" % np.abs(rec["grad"][n]).max() for n in c["null"]] for rec in r64],
          "float32 max|g|", [["%.1e" % v for v in step.values()] for step in c["noise"]], "smallest max|g| of the others %.2e" % small)
    assert small > 1e3 * WS.NULL_G                                                      # nothing sits between noise and a gradient
    for step in c["noise"]:
        assert all(0 < v < 1e-4 for v in step.values())


def test_the_float32_run_keeps_the_null_deltas_within_the_budget(case):
    """null_delta_budget on the float32 restatement itself: the rule the GPU module applies to the port (argued in the cases module)"""
    name, c = case
    sd0, r64, r32 = c["cap"]["sd0"], c["r64"], c["r32"]
    for n in c["null"]:
        for s in range(WS.STEPS):
            lrs = [r64[j]["lr"][WS.group_of(n)] for j in range(s + 1)]
            gs = [c["noise"][j][n] for j in range(s + 1)]
            p_max = float(np.abs(r32[s]["p"][n]).max())
            d = float(np.abs(WS.quantity(r32[s], "delta", n, sd0).astype(np.float64) - WS.quantity(r64[s], "delta", n, sd0)).max())
            print("%s step %d %-40s |delta32 - delta64| %.3e  noise part %.3e  storage part %.3e" % (
                name, s, n, d, WS.null_delta_budget(lrs, gs, 0.0), WS.null_delta_budget(lrs, gs, p_max) - WS.null_delta_budget(lrs, gs, 0.0)))
            assert d <= WS.null_delta_budget(lrs, gs, p_max), (name, s, n)
    assert WS.null_delta_budget([0.0, 0.5, 0.25], [2e-9, 1e-9, 4e-9], 0.5) == (0.5 * 2e-9 + 0.25 * 4e-9) / 1e-3 + 2 * 2.0 ** -24 * 0.5


def test_float32_against_float64_is_an_fp32_error(case):
    name, c = case
    print("\n".join(WS.table(name, c["pool"])))
    worst = {}
    for (q, kind), e in c["pool"].items():
        worst[q] = max(worst.get(q, 0.0), e)
    print(name, "worst per quantity:", " ".join("%s %.2e" % kv for kv in sorted(worst.items())))
    assert set(worst) == {"loss", "terms", "codes", "buffer", "grad", "clipped", "delta", "m", "v"}
    assert {k for q, k in c["pool"] if q == "codes"} == set(WS.CODES)
    for s, errs in enumerate(c["per"]):
        for key, e in errs.items():
            assert np.isfinite(e) and e < 1e-2, (name, s, key, e)
    assert all(e == 0.0 for (q, n), e in c["per"][0].items() if q == "delta")           # rate 0: the float32 run does not move either
    assert worst["grad"] > 2.0 ** -27                                                   # and it is a float32 run
    assert all(rec["p"][k].dtype == np.float32 for rec in c["r32"] for k in rec["p"])


def test_structure_of_the_float64_run(case):
    name, c = case
    r64, cap, named = c["r64"], c["cap"], c["named"]
    sd0 = cap["sd0"]
    adam = [n for n in named if n != "backbone.logit_scale"]
    assert "backbone.logit_scale" in named and {WS.group_of(n) for n in adam} == {"backbone", "hash"}
    tok, pos = "backbone.token_embedding.weight", "backbone.positional_embedding"
    for s, rec in enumerate(r64):
        assert sorted(rec["grad"]) == sorted(adam) and "backbone.logit_scale" not in rec["p"]
        for group, lr in (("backbone", WS.OPT_CFG["backbone_lr"]), ("hash", WS.OPT_CFG["lr"])):
            want = 0.0 if s == 0 else lr * 0.5 * (1.0 + math.cos(math.pi * s / WS.STEPS))
            assert rec["lr"][group] == want and rec["count"] == s + 1, (s, group, rec["lr"])
            assert rec["next_lr"][group] == lr * 0.5 * (1.0 + math.cos(math.pi * (s + 1) / WS.STEPS))
        ids = cap["batches"][s % 2][1]
        absent = np.setdiff1d(np.arange(sd0[tok].shape[0]), np.unique(ids.numpy()))
        g_tok, g_pos = WS.dense(rec["grad"][tok]), WS.dense(rec["grad"][pos])
        assert not g_tok[absent].any() and g_tok.any() and not g_pos[ids.shape[1]:].any() and g_pos[0].any()
        for mod in WS.MODS:
            e = sd0["hash.%s_hash.norm.weight" % mod].shape[0]
            for k in ("in_proj_weight", "in_proj_bias"):
                g = rec["grad"]["hash.%s_hash.atten.%s" % (mod, k)]
                assert not g[:2 * e].any() and g[2 * e:].any(), (s, mod, k)
        assert rec["buffers"]["hash.img_hash.norm.num_batches_tracked"] == s + 1
        assert s == 0 or not np.array_equal(rec["buffers"]["hash.img_hash.norm.running_mean"], r64[s - 1]["buffers"]["hash.img_hash.norm.running_mean"])
        assert rec["terms"].shape == (1 + 6 * len(cap["lens"]),) and rec["terms"][0] == rec["loss"]
    for n in adam:                                                                      # step 0: rate 0
        assert np.array_equal(r64[0]["p"][n], sd0[n].numpy().astype(np.float64)), n
        assert WS.dense(r64[0]["m"][n]).any() and WS.dense(r64[0]["v"][n]).any(), n
        assert not np.array_equal(r64[1]["p"][n], r64[0]["p"][n]), n                    # and the next one moves everything


def test_the_short_terms_weigh_what_the_case_says(case):
    name, c = case
    cap = c["cap"]
    n = len(cap["lens"])
    for rec in c["r64"]:
        means = rec["terms"][1 + 4 * n:]
        per = rec["terms"][1:1 + 4 * n]
        assert np.allclose(means, (per[:2 * n] + per[2 * n:]) / 2, rtol=1e-15, atol=0)
        long_only = means[0] + WS.QUAN_ALPHA * means[1]
        assert (means[2:] > 0.1).all()                                                  # the short terms are computed in either case
        if name == "shipped":
            assert rec["loss"] == long_only
        else:
            assert abs(rec["loss"] - (long_only + 0.3 * means[2:].sum())) < 1e-14 and rec["loss"] - long_only > 0.1


def test_the_way_through_the_transforms_is_a_visible_share_of_the_long_gradient(case):
    name, c = case
    cap, rec = c["cap"], c["r64"][0]
    T = torch.cat([cap["trans"][k] for k in cap["keys"]], 1)
    for mod in WS.MODS:
        p_long, p_short = rec["probs"][mod + "_long"], rec["probs"][mod + "_short"]
        dl, ds = TC.loss_grad(p_long, p_short, rec["bits"], cap["lens"], cap["quan_alpha"], cap["low_rate"], 1.0)
        through = TC.short_backward(ds, torch.tensor(p_short), T)
        gap = TC.rel_err((dl + through).numpy(), dl.numpy())
        print(name, mod, "d_long with and without short_backward: %.3e relative" % gap)
        if name == "rated":
            assert gap > 1e-3
        else:
            assert gap == 0.0 and not ds.numpy().any()                                  # low_rate 0: an exact zero


def test_given_its_own_bits_and_masks_the_restatement_reproduces_itself_to_the_bit(case):
    name, c = case
    again = WS.run(c["cap"], bits=WS.bits_of(c["r64"]), masks=WS.masks_of(c["r64"]))
    for a, b in zip(c["r64"], again):
        assert a["loss"] == b["loss"] and np.array_equal(a["terms"], b["terms"]) and np.array_equal(a["bits"], b["bits"])
        for mod in WS.MODS:
            assert np.array_equal(a["z"][mod], b["z"][mod]) and np.array_equal(a["masks"][mod], b["masks"][mod])
        assert all(np.array_equal(a["probs"][k], b["probs"][k]) for k in WS.CODES)
        assert all(np.array_equal(a["buffers"][k], b["buffers"][k]) for k in a["buffers"])
        for kind in ("grad", "clipped", "p", "m", "v"):
            assert sorted(a[kind]) == sorted(b[kind])
            assert all(np.array_equal(WS.dense(a[kind][k]), WS.dense(b[kind][k])) for k in a[kind]), kind


def test_the_restated_objective_is_the_pinned_one(case):
    """objective() at step 0 against twdh_cases.loss / loss_grad, which tests/golden/twdh_loss.npz pins to the reference"""
    name, c = case
    cap, rec = c["cap"], c["r64"][0]
    lens, qa, lr = cap["lens"], cap["quan_alpha"], cap["low_rate"]
    leaves = {k: torch.tensor(rec["probs"][k]).requires_grad_(True) for k in WS.CODES}
    total, terms = WS.objective({m: leaves[m + "_long"] for m in WS.MODS}, {m: leaves[m + "_short"] for m in WS.MODS}, rec["bits"], lens, qa, lr,
                                torch.float64)
    total.backward()
    want = TC.loss(rec["probs"]["img_long"], rec["probs"]["img_short"], rec["probs"]["txt_long"], rec["probs"]["txt_short"], rec["bits"], lens, qa, lr)
    assert terms.shape == want.shape and TC.rel_err(terms.numpy(), want.numpy()) < 1e-14 and float(total.detach()) == rec["loss"]
    for mod in WS.MODS:
        dl, ds = TC.loss_grad(rec["probs"][mod + "_long"], rec["probs"][mod + "_short"], rec["bits"], lens, qa, lr, 1.0)
        assert TC.rel_err(leaves[mod + "_long"].grad.numpy(), dl.numpy()) < 1e-14
        g_short = leaves[mod + "_short"].grad.numpy()
        assert (TC.rel_err(g_short, ds.numpy()) < 1e-14 and g_short.any()) if lr else not g_short.any()
    # and the short codes of the record are the transforms of its long codes
    T = torch.cat([cap["trans"][k] for k in cap["keys"]], 1)
    assert all(TC.rel_err(rec["probs"][m + "_short"], TC.short_forward(rec["probs"][m + "_long"], T).numpy()) < 1e-14 for m in WS.MODS)
    assert WS.loss_dict_places(len(lens))[:5] == [0, 1, 1 + 2 * len(lens), 2, 2 + 2 * len(lens)]
    assert len(WS.loss_dict_places(len(lens))) == len(WS.loss_dict_names(cap["keys"])) == 5 + 2 * len(cap["keys"])


def test_the_replayed_ties_are_the_models_draw(case):
    name, c = case
    model, cap = c["t"].model, c["cap"]
    for s in range(WS.STEPS):
        torch.manual_seed(WS.TIE_SEED + s)
        before = torch.random.get_rng_state()
        replay = WS.replay_ties(cap, s)
        assert torch.equal(torch.random.get_rng_state(), before)                        # the replay leaves the global generator alone
        drawn = model.draw_ties()
        assert list(drawn) == ["long"] + cap["keys"] == list(replay)
        for k in drawn:
            assert drawn[k].dtype == torch.float32 and torch.equal(drawn[k], replay[k]) and set(drawn[k].tolist()) <= {-1.0, 1.0}, (s, k)
        assert np.array_equal(np.concatenate([drawn[k].numpy() for k in drawn]), c["r64"][s]["ties"])
    assert not torch.equal(WS.replay_ties(cap, 0)["long"], WS.replay_ties(cap, 1)["long"])
