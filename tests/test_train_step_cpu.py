"""The whole-training-step suite without a GPU: the float64 restatement of tests/train_step_cases.py (which tests/test_gpu_train_step.py
leans on) on the two cases, DCMHT and DSPH, five steps each.

Conditions on the inputs (not measurements), asserted on the float64 run at every step: every fc2 pre-activation of both DCMHT heads
lies outside its tie bound (oracle.heads_train), every cosine that HyP compares with its threshold keeps GAP from it, nothing
excluded.  The dataset seed 1814 meets both, so it stays.  With that seed only one row of the eight carries two labels, so HyP's
regulariser has no pair in either batch: its three terms are zero throughout and contribute no cosine (printed as a count of 0).

The null set (gradients that are identically zero in exact arithmetic, defined by max|g64| < 1e-10 at every step) is pinned: for
DCMHT the three biases in front of the image head's BatchNorm -- hash.img_hash.atten.in_proj_bias, hash.img_hash.atten.out_proj.bias
and backbone.visual.ln_post.bias; measured here in float64 2e-16 .. 7e-15 against 1e-6 and more for every other tensor, fp32 noise
9e-8 .. 4e-6 -- and for DSPH, which has no BatchNorm, the empty set.

The float32 run against the float64 run is the yardstick of the GPU module; here its figures are printed and held to a sanity bound
(finite, below 1e-2; measured: loss <= 4e-7, grad <= 3e-5, m / v <= 2.2e-5, delta <= 2.5e-4, running statistics <= 1.6e-6).

Structure: logit_scale has no gradient; the q and k thirds of the heads' in_proj have exact-zero gradients; positional rows >= L and
absent token ids have exact-zero gradients and their delta is weight decay alone; step 0 (rate 0) changes no parameter while m and v
are filled; the scheduled rates are lr_f64 of each group."""
import math

import numpy as np
import pytest
import torch

import train_step_cases as TS
from oracle import heads_train as HT

_cache = {}


def _case(arch, tmp_path_factory):
    """trainer on the CPU (model and loader only: nothing of it runs), the float64 run, the null set and the float32 yardstick; once"""
    if arch not in _cache:
        t = TS.trainer(arch, tmp_path_factory.mktemp(arch), "cpu")
        sd0, raw = TS.capture(t)
        named = [n for n, _ in t.model.named_parameters()]
        masks = TS.cpu_masks() if arch == "DSPH" else None
        batches = TS.batches_of(raw)
        r64 = TS.run(arch, sd0, batches, masks=masks)
        null = TS.null_set(r64)
        per, pooled, noise = TS.yardstick(arch, sd0, batches, r64, masks, null)
        _cache[arch] = dict(sd0=sd0, raw=raw, named=named, batches=batches, r64=r64, null=null, per=per, pool=pooled, noise=noise)
    return _cache[arch]


@pytest.fixture(params=list(TS.ARCHS))
def case(request, tmp_path_factory):
    return request.param, _case(request.param, tmp_path_factory)


def test_the_inputs_meet_the_conditions_at_every_step(case):
    arch, c = case
    got = TS.check_conditions(arch, c["r64"])
    for key, v in got.items():
        print(arch, "step %d %-6s" % key, ("min|z| %.2e = %.0f tie bounds" if arch == "DCMHT" else "%d cosines, nearest %.2e from the threshold") % v)
    assert len(c["r64"]) == TS.STEPS and len(c["batches"]) == 2
    if arch == "DSPH":
        assert all(v[0] == 0 for (s, key), v in got.items() if key.startswith("reg"))       # what the docstring says of this seed
        assert all(np.isin(m.numpy(), (0, 1)).all() and 0.5 < float(m.float().mean()) < 1 for pair in TS.cpu_masks() for m in pair)


def test_the_null_set_is_pinned(case):
    arch, c = case
    r64 = c["r64"]
    assert c["null"] == (TS.NULL_DCMHT if arch == "DCMHT" else ())
    others = [n for n in r64[0]["grad"] if n not in c["null"]]
    small = min(float(np.abs(TS.dense(rec["grad"][n])).max()) for rec in r64 for n in others)
    print(arch, "null set", c["null"], "float64 max|g|", [["%.1e" % np.abs(rec["grad"][n]).max() for n in c["null"]] for rec in r64],
          "float32 max|g|", [["%.1e" % v for v in step.values()] for step in c["noise"]], "smallest max|g| of the others %.2e" % small)
    assert small > 1e3 * TS.NULL_G                                                      # nothing sits between noise and a gradient
    for step in c["noise"]:
        assert all(0 < v < 1e-4 for v in step.values())


def test_float32_against_float64_is_an_fp32_error(case):
    arch, c = case
    print("\n".join(TS.table(arch, c["pool"])))
    worst = {}
    for (q, kind), e in c["pool"].items():
        worst[q] = max(worst.get(q, 0.0), e)
    print(arch, "worst per quantity:", " ".join("%s %.2e" % kv for kv in sorted(worst.items())))
    assert {"loss", "grad", "clipped", "delta", "m", "v"} <= set(worst) and (arch != "DCMHT" or "buffer" in worst) and (arch != "DSPH" or "buf" in worst)
    for s, errs in enumerate(c["per"]):
        for key, e in errs.items():
            assert np.isfinite(e) and e < 1e-2, (arch, s, key, e)
    # rate 0: the float32 run does not move either (the proxies' SGD has no warm-up)
    assert all(e == 0.0 for (q, n), e in c["per"][0].items() if q == "delta" and n != "hyp.proxies")
    assert worst["grad"] > 2.0 ** -27                                                   # and it is a float32 run


def test_structure_of_the_float64_run(case):
    arch, c = case
    r64, sd0, named = c["r64"], c["sd0"], c["named"]
    adam = [n for n in named if TS.group_of(n) != "hyp" and n != "backbone.logit_scale"]
    assert "backbone.logit_scale" in named and {TS.group_of(n) for n in adam} == {"backbone", "hash"}
    for s, rec in enumerate(r64):
        assert sorted(rec["grad"]) == sorted(adam + (["hyp.proxies"] if arch == "DSPH" else [])) and "backbone.logit_scale" not in rec["p"]
        for group, lr in (("backbone", TS.OPT_CFG["backbone_lr"]), ("hash", TS.OPT_CFG["lr"])):
            want = 0.0 if s == 0 else lr * 0.5 * (1.0 + math.cos(math.pi * s / TS.STEPS))
            assert rec["lr"][group] == want and rec["count"] == s + 1, (s, group, rec["lr"])
        ids = c["batches"][s % 2][1]
        absent = np.setdiff1d(np.arange(sd0["backbone.token_embedding.weight"].shape[0]), np.unique(ids.numpy()))
        g_tok, g_pos = (TS.dense(rec["grad"]["backbone." + k]) for k in ("token_embedding.weight", "positional_embedding"))
        assert not g_tok[absent].any() and g_tok.any() and not g_pos[ids.shape[1]:].any() and g_pos[0].any()
        if arch == "DCMHT":
            for mod in ("img", "txt"):
                e = sd0["hash.%s_hash.norm.weight" % mod].shape[0]
                for k in ("in_proj_weight", "in_proj_bias"):
                    g = rec["grad"]["hash.%s_hash.atten.%s" % (mod, k)]
                    assert not g[:2 * e].any() and g[2 * e:].any(), (s, mod, k)
            assert rec["buffers"]["hash.img_hash.norm.num_batches_tracked"] == s + 1
            assert not np.array_equal(rec["buffers"]["hash.img_hash.norm.running_mean"], r64[s - 1]["buffers"]["hash.img_hash.norm.running_mean"]) or s == 0
    for n in adam:                                                                      # step 0: rate 0
        assert np.array_equal(r64[0]["p"][n], sd0[n].numpy().astype(np.float64)), n
        assert TS.dense(r64[0]["m"][n]).any() and TS.dense(r64[0]["v"][n]).any(), n
        assert not np.array_equal(r64[1]["p"][n], r64[0]["p"][n]), n                    # and the next one moves everything
    # rows without a gradient at any step: weight decay alone
    seen = np.unique(np.concatenate([b[1].numpy().reshape(-1) for b in c["batches"]]))
    decay = np.prod([1.0 - rec["lr"]["backbone"] * TS.ADAM["weight_decay"] for rec in r64])
    for key, rows in (("backbone.token_embedding.weight", np.setdiff1d(np.arange(sd0["backbone.token_embedding.weight"].shape[0]), seen)),
                      ("backbone.positional_embedding", np.arange(32, sd0["backbone.positional_embedding"].shape[0]))):
        assert len(rows) > 0
        p0 = sd0[key].numpy().astype(np.float64)[rows]
        assert TS.rel_err(r64[-1]["p"][key][rows], p0 * decay) < 1e-14 and 0 < 1 - decay < 1e-3, key
        assert not TS.dense(r64[-1]["m"][key])[rows].any() and not TS.dense(r64[-1]["v"][key])[rows].any()
    if arch == "DSPH":
        assert r64[0]["proxy_buf"].any() and not np.array_equal(r64[0]["p"]["hyp.proxies"], sd0["hyp.proxies"].numpy().astype(np.float64))


def test_the_heads_of_the_restatement_are_the_oracles():
    """dcmht_head / dsph_head against the closed forms of oracle.heads_train, which tests/golden/head_grad.npz pins to the reference"""
    E, Bn, Kn = 64, 5, 16
    x, up = HT.draw_batch(11, Bn, 2 * Kn, e=E)
    for bn in (True, False):
        P = HT.draw_dcmht(12 + bn, Kn, bn, e=E)
        t = {HT.DCMHT_KEYS[k]: torch.tensor(P[k]).double().requires_grad_(True) for k in HT.DCMHT_PARAMS}
        xt = torch.tensor(x).double().requires_grad_(True)
        probs, aux = TS.dcmht_head(xt, t, bn)
        (probs * torch.tensor(up).double()).sum().backward()
        want = HT.dcmht_f64(x, P, bn, up)
        assert TS.rel_err(probs.detach().numpy(), want["probs"]) < 1e-13 and TS.rel_err(aux["z"].detach().numpy(), want["z"]) < 1e-13
        assert TS.rel_err(TS.tie_bound(aux["n"].detach().numpy(), P["w2"]), want["tie"]) < 1e-13
        assert TS.rel_err(xt.grad.numpy(), want["g_x"]) < 1e-12
        for k in ("out_w", "norm_w", "norm_b", "w2", "b2"):
            assert TS.rel_err(t[HT.DCMHT_KEYS[k]].grad.numpy(), want["g_" + k]) < 1e-12, (bn, k)
        if bn:
            assert TS.rel_err(aux["o"].detach().mean(0).numpy(), want["mean"]) < 1e-13
            assert TS.rel_err(aux["o"].detach().var(0, unbiased=True).numpy(), want["var_unbiased"]) < 1e-13
    P = HT.draw_dsph(14, Kn, e=E)
    keep = (np.random.default_rng(15).random((Bn, Kn)) >= 0.2)
    y = TS.dsph_head(torch.tensor(x).double(), torch.tensor(P["w"]).double(), torch.tensor(P["b"]).double(), torch.tensor(keep).double())
    assert TS.rel_err(y.numpy(), HT.dsph_f64(x, P, keep, 0.2, up[:, :Kn])["y"]) < 1e-13
