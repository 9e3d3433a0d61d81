"""The whole-training-step suite of UMoED without a GPU: the float64 restatement of tests/umoed_train_step_cases.py (which
tests/test_gpu_umoed_train_step.py leans on) on the two cases, `small` and `deep`, five steps each.

Conditions on the inputs (not measurements of the port), asserted on the float64 run at every step; margin is the float64 distance
from the kink, noise the largest |float32 - float64| of the same quantity over the steps, and margin > TOL_FACTOR = 4 noise is asked.
Measured at the dataset seed 1821 and the mask seed 1814 -- small: hinge 1.58e-2 against 5.8e-7, the similarity under the clamp 0.204
against 1.6e-6 (softmaxed rows: it cannot reach 0, the clamp is inert here), the gap of the two largest logits 4.4e-2 / 6.2e-2 against
8.5e-7 / 5.7e-7 (umoed_cases.head_gap 0.07 at least), the ReLU of the image / text call 5.0e-4 / 1.19e-3 against 8.5e-7 / 6.4e-7; deep:
hinge 1.9e-4 against 1.1e-6, clamp 1.6e-2 against 1.1e-6, gap 7.4e-3 / 6.1e-3 against 3.9e-6 / 3.4e-6 (head_gap 3.4e-3 at least, the
guard is 1e-3), the four ReLUs 1.6e-4 / 6.0e-4 / 7.2e-4 / 2.4e-4 against 3.0e-6 / 3.6e-6 / 2.1e-6 / 2.5e-6 (the narrowest ratio 52).  No
ReLU decision and no code bit differs in float32, the two triplet terms have between 4 and 14 live summands, every row has a label, the
mask sections keep between 0.53 and 0.83 of their entries, and the float32 run's worst gradient error per step is 6.4e-6, 2.7e-6, 1.2e-5,
2.0e-5, 1.7e-5 (small) and 3.2e-6, 2.8e-6, 2.9e-6, 3.3e-6, 5.2e-6 (deep) against the cap of 1e-4.  The GPU module asserts the same on the
masks the device draws (with them small has 7.5e-4 / 1.6e-4 / 2.1e-4 for hinge and the two ReLUs, and at most 1.2e-5 for the cap on the
MI355X host, 3.7e-5 on another CPU).

Seeds.  MASK_SEED is 1814, the first tried.  DATA_SEED is the first from 1814 on that meets every condition in both cases, with the CPU's
masks here and with the device's masks in the GPU module; 1814 to 1820 each miss.  1814: small's float32 gradient error 1.16e-4 at step 4
(above the cap), deep a row of embeds with its two largest logits 1.6e-4 of the largest apart (guard 1e-3).  1815: small's cap at step 4
(2.0e-3), deep's logit gap (8.8e-4).  1816: deep, a ReLU pre-activation 2.7e-6 from zero against max|pre| 3.7 (the guard asks 1e-5 of
it).  1817: small, a ReLU pre-activation 2.0e-6 from zero; deep's logit gap (9.98e-4).  1818: deep, a ReLU pre-activation 2.8e-5 from
zero against max|pre| 4.06.  1819: small, a ReLU pre-activation 6.0e-8 from zero; deep, a batch whose rows all share a label, so that no
triplet is live.  1820: small and deep, ReLU pre-activations 1.8e-5 and 2.8e-5 from zero against max|pre| 2.07 and 3.68.  (Further on,
1825 meets all of it with the CPU's masks and, with the device's, on one CPU only: on another the cap is missed with 1.13e-4.)

Sets: backbone.logit_scale is the only parameter without a gradient, and the null set (max|g64| < 1e-10 at every step) is empty; the
smallest max|g64| of any tensor is 8.1e-4 (small: phi, under the module's own init) and 9.7e-4 (deep: the second layer's experts' bias).

The float32 run against the float64 run is the yardstick of the GPU module; here its figures are printed and held to a sanity bound
(finite, below 1e-2; measured: loss and terms <= 4.7e-6, embeds <= 1.3e-6, codes exact, grad / clipped <= 2.0e-5, m <= 4.7e-5, v <= 1.4e-5,
delta <= 4.5e-4), the gradients besides to the cap of 1e-4 that the conditions set.

Structure of the float64 run: step 0 (rate 0) moves no parameter while m and v are filled; positional rows at or beyond L and token
ids absent from the batch have exact-zero gradients; the scheduled rates are lr_f64 of each group.  Run again with the same masks,
the restatement reproduces itself to the bit.  The head's gradient is the sum of the two calls' contributions: the restatement with
the image call's embeds cut off the graph gives the text call's share (and no gradient in the image tower), with the text call's cut
off the image call's, and the two add up to the whole run's gradient of every head tensor to 1e-12 of its size, neither being small."""
import math

import numpy as np
import pytest
import torch

import umoed_train_step_cases as US

_cache = {}
NULL = {"small": (), "deep": ()}


def _case(case, tmp_path_factory):
    """trainer on the CPU (model and loader only: nothing of it runs), the float64 and float32 runs on the same masks; once"""
    if case not in _cache:
        t = US.trainer(case, tmp_path_factory.mktemp(case), "cpu")
        cap = US.capture(t, case)
        masks = US.draw_masks(cap)
        r64 = US.run(cap, masks)
        r32 = US.run(cap, masks, dtype=torch.float32)
        null = US.null_set(r64)
        per, pooled, _ = US.yardstick(cap, r64, r32, null)
        _cache[case] = dict(cap=cap, masks=masks, r64=r64, r32=r32, per=per, pool=pooled, null=null, head=t.model.hash.hash_module)
    return _cache[case]


@pytest.fixture(params=list(US.CASES))
def case(request, tmp_path_factory):
    return request.param, _case(request.param, tmp_path_factory)


def test_the_inputs_meet_the_conditions_at_every_step(case):
    name, c = case
    cap = c["cap"]
    assert len(c["r64"]) == US.STEPS and len(cap["raw"]) == 3
    cond = US.check_conditions(cap, c["r64"], c["r32"], c["masks"])
    print("\n".join(US.condition_lines(name, cond)))
    spec = cap["spec"]
    if name == "small":                                                                 # two masks a step, cut as the head lays them out
        assert spec["V"] == 2 and len(c["masks"]) == US.STEPS and all(len(ms) == 2 for ms in c["masks"])
        head = c["head"]
        for ms in c["masks"]:
            for call, T in zip(ms, (5, 32)):
                assert [m.size for m in call[0]] == head.keep_sections(US.B, T) and len(call) == spec["layers"]
        g = torch.Generator().manual_seed(US.MASK_SEED)                                 # the replay is the head's own draw
        head.generator = g
        for call, T in zip(c["masks"][0], (5, 32)):
            assert np.array_equal(head.draw_keep_mask(US.B, T, "cpu").numpy(), US.UT.flat_keep(call))
        head.generator = None
    else:
        assert c["masks"] is None and c["head"].draw_keep_mask(US.B, 5, "cpu") is None
        assert spec["V"] == 16 and c["r64"][0]["outs"][1].shape == (US.B, 24) and c["r64"][0]["outs"][0].shape == (US.B, 6, 16)
        P = US.UC.head_params(spec, US.HEAD_SEED)                                       # the loaded head is what was captured
        assert all(np.array_equal(cap["sd0"][US.HEAD + k].numpy(), v) for k, v in P.items())
    for rec in c["r64"]:                                                                # the ReLU is at work in every layer of both calls
        assert all(0.05 < float((z > 0).mean()) < 0.95 for mod in US.MODS for z in rec["pre"][mod])
        assert all(set(np.unique(code)) <= {-1.0, 1.0} for code in rec["outs"][1::2])


def test_the_sets_are_pinned(case):
    name, c = case
    r64 = c["r64"]
    assert US.no_grad_set(c["cap"], r64) == ("backbone.logit_scale",)
    assert all(sorted(rec["grad"]) == sorted(r64[0]["grad"]) for rec in r64)
    small = min((float(np.abs(US.dense(rec["grad"][k])).max()), k) for rec in r64 for k in rec["grad"] if k not in c["null"])
    print(name, "null set", c["null"], "smallest max|g64| of any other tensor %.3e (%s)" % small)
    assert c["null"] == NULL[name] and small[0] > 1e3 * US.NULL_G


def test_float32_against_float64_is_an_fp32_error(case):
    name, c = case
    print("\n".join(US.table(name, c["pool"])))
    worst = {}
    for (q, kind), e in c["pool"].items():
        worst[q] = max(worst.get(q, 0.0), e)
    print(name, "worst per quantity:", " ".join("%s %.2e" % kv for kv in sorted(worst.items())))
    assert set(worst) == {"loss", "terms", "codes", "grad", "clipped", "delta", "m", "v"}
    for s, errs in enumerate(c["per"]):
        for key, e in errs.items():
            assert np.isfinite(e) and e < 1e-2, (name, s, key, e)
            assert key[0] != "grad" or e <= US.GRAD_CAP, (name, s, key, e)
    assert all(e == 0.0 for (q, n), e in c["per"][0].items() if q == "delta")           # rate 0: the float32 run does not move either
    assert all(e == 0.0 for errs in c["per"] for (q, n), e in errs.items() if q == "codes" and n.endswith("_hash"))
    assert worst["grad"] > 2.0 ** -27                                                   # and it is a float32 run
    assert all(rec["p"][k].dtype == np.float32 for rec in c["r32"] for k in rec["p"])


def test_structure_of_the_float64_run(case):
    name, c = case
    cap, r64 = c["cap"], c["r64"]
    sd0 = cap["sd0"]
    tok, pos = "backbone.token_embedding.weight", "backbone.positional_embedding"
    vocab = sd0[tok].shape[0]
    assert {US.group_of(k) for k in r64[0]["grad"]} == {"backbone", "hash"} and sd0[pos].shape[0] > 32
    assert sum(k.startswith("hash.") for k in r64[0]["grad"]) == 1 + 19 * cap["spec"]["layers"] + 2
    for s, rec in enumerate(r64):
        for group, lr in (("backbone", US.OPT_CFG["backbone_lr"]), ("hash", US.OPT_CFG["lr"])):
            want = 0.0 if s == 0 else lr * 0.5 * (1.0 + math.cos(math.pi * s / US.STEPS))
            assert rec["lr"][group] == want and rec["count"] == s + 1, (s, group, rec["lr"])
            assert rec["next_lr"][group] == lr * 0.5 * (1.0 + math.cos(math.pi * (s + 1) / US.STEPS))
        ids = cap["raw"][s % 3][1].numpy()
        absent = np.setdiff1d(np.arange(vocab), np.unique(ids))
        g_tok, g_pos = US.dense(rec["grad"][tok]), US.dense(rec["grad"][pos])
        assert not g_tok[absent].any() and g_tok.any() and not g_pos[ids.shape[1]:].any() and g_pos[0].any()
        assert rec["terms"][0] == rec["loss"] and np.isfinite(rec["terms"]).all() and len(rec["terms"]) == 5
    for k in r64[0]["grad"]:                                                            # step 0: rate 0
        assert np.array_equal(r64[0]["p"][k], sd0[k].numpy().astype(np.float64)), k
        if k not in c["null"]:
            assert US.dense(r64[0]["m"][k]).any() and US.dense(r64[0]["v"][k]).any(), k
            assert not np.array_equal(r64[1]["p"][k], r64[0]["p"][k]), k                # and the next one moves everything


def test_given_the_same_masks_the_restatement_reproduces_itself_to_the_bit(case):
    name, c = case
    again = US.run(c["cap"], c["masks"])
    for a, b in zip(c["r64"], again):
        assert a["loss"] == b["loss"] and np.array_equal(a["terms"], b["terms"])
        assert all(np.array_equal(x, y) for x, y in zip(a["outs"], b["outs"]))
        for kind in ("grad", "clipped", "p", "m", "v"):
            assert sorted(a[kind]) == sorted(b[kind])
            assert all(np.array_equal(US.dense(a[kind][k]), US.dense(b[kind][k])) for k in a[kind]), kind


def test_the_heads_gradient_is_the_sum_of_the_two_calls_contributions(case):
    """steps 0 and 1 (step 0 runs at rate 0, so all three runs hold the same parameters at both)"""
    name, c = case
    cap, whole = c["cap"], c["r64"]
    part = {mod: US.run(cap, c["masks"], steps=2, detach=mod) for mod in US.MODS}      # detach img: the text call's share is left
    worst = 0.0
    for s in range(2):
        assert whole[s]["loss"] == part["img"][s]["loss"] == part["txt"][s]["loss"]
        for k, g in whole[s]["grad"].items():
            a, b = (part[mod][s]["grad"].get(k) for mod in US.MODS)
            if k.startswith("hash."):
                g, a, b = US.dense(g), US.dense(a), US.dense(b)
                scale = np.abs(g).max()
                e = np.abs(a + b - g).max() / scale
                worst = max(worst, e)
                assert e <= 1e-12, (s, k, e)
                assert np.abs(a).max() > 1e-3 * scale and np.abs(b).max() > 1e-3 * scale, (s, k, "one call's share is negligible")
            else:                                                                        # a tower is reached through its own call alone
                image_tower = k.startswith("backbone.visual.")
                own, other = (b, a) if image_tower else (a, b)
                assert other is None and np.array_equal(US.dense(own), US.dense(g)), (s, k)
    print(name, "head gradient: |text share + image share - whole| / max|whole| at most %.2e" % worst)
