"""CPU: the float64 restatement of a DISTRIBUTED training step (tests/ddp_train_step_cases.py, which tests/test_gpu_ddp_train.py leans
on) for DCMHT and DSPH.

With one rank it is train_step_cases.run to the bit (same operations, same order) on train_step_cases' own case.  With two ranks on
IDENTICAL shards the gradient is the one-shard gradient to float64 rounding: BatchNorm over [o; o] has o's mean and biased variance,
and (l + l) / 2 = l; the unbiased running variance is the one thing that differs (n_total - 1), and it is checked to differ as
var n / (n - 1) says.  The conditions of train_step_cases.check_conditions hold on every shard of the case's float64 run with the
recorded DATA_SEED, the null set is train_step_cases' own, and the float32 run of the distributed step against the float64 one --
the yardstick of the GPU module -- is an fp32-sized error."""
import numpy as np
import pytest

import ddp_train_step_cases as DS
import train_step_cases as TS

_cache = {}


def _single(arch, tmp_path_factory):
    """train_step_cases' own case: trainer on the CPU, two batches of B rows"""
    key = ("single", arch)
    if key not in _cache:
        t = TS.trainer(arch, tmp_path_factory.mktemp("s" + arch), "cpu")
        sd0, raw = TS.capture(t)
        _cache[key] = (sd0, TS.batches_of(raw))
    return _cache[key]


def _case(arch, tmp_path_factory):
    if arch not in _cache:
        t = DS.trainer(arch, tmp_path_factory.mktemp("d" + arch), "cpu")
        sd0 = {k: v.detach().cpu().clone() for k, v in t.model.state_dict().items()}
        batches = DS.shards(t.train_loader.dataset)
        masks = DS.cpu_masks() if arch == "DSPH" else None
        r64 = DS.run(arch, sd0, batches, masks=masks)
        _cache[arch] = dict(sd0=sd0, batches=batches, masks=masks, r64=r64)
    return _cache[arch]


@pytest.mark.parametrize("arch", list(TS.ARCHS))
def test_one_rank_is_the_single_process_restatement_to_the_bit(arch, tmp_path_factory):
    sd0, batches = _single(arch, tmp_path_factory)
    masks = TS.cpu_masks(steps=2) if arch == "DSPH" else None
    want = TS.run(arch, sd0, batches, steps=2, masks=masks)
    got = DS.run(arch, sd0, [[b] for b in batches], steps=2, masks=None if masks is None else [[m] for m in masks], hyper=TS.hyper_of)
    for s, (a, b) in enumerate(zip(got, want)):
        assert a["loss"] == b["loss"] and a["losses"] == [b["loss"]], s
        for kind in ("grad", "clipped", "p", "m", "v"):
            assert sorted(a[kind]) == sorted(b[kind])
            for n in b[kind]:
                assert np.array_equal(TS.dense(a[kind][n]), TS.dense(b[kind][n])), (s, kind, n)
        for n, v in b["buffers"].items():
            assert np.array_equal(a["buffers"][n], v), (s, n)
        if arch == "DSPH":
            assert np.array_equal(a["proxy_buf"], b["proxy_buf"])


@pytest.mark.parametrize("arch", list(TS.ARCHS))
def test_two_ranks_on_identical_shards_give_the_one_shard_gradient(arch, tmp_path_factory):
    sd0, batches = _single(arch, tmp_path_factory)
    masks = TS.cpu_masks(steps=1) if arch == "DSPH" else None
    one = DS.run(arch, sd0, [[batches[0]]], steps=1, masks=None if masks is None else [[masks[0]]])[0]
    two = DS.run(arch, sd0, [[batches[0], batches[0]]], steps=1, masks=None if masks is None else [[masks[0], masks[0]]])[0]
    assert two["losses"][0] == two["losses"][1] and abs(two["loss"] - one["loss"]) <= 1e-14 * abs(one["loss"])
    null = TS.NULL_DCMHT if arch == "DCMHT" else ()
    worst = 0.0
    for n, g in one["grad"].items():
        a, b = TS.dense(two["grad"][n]), TS.dense(g)
        if n in null:
            assert np.abs(a).max() < TS.NULL_G
            continue
        worst = max(worst, TS.rel_err(a, b))
    print(arch, "two identical shards against one: worst rel_err of a gradient %.2e" % worst)
    assert worst < 1e-12                                                                 # float64 rounding of another summation
    if arch == "DCMHT":
        n = TS.B
        pre = "hash.img_hash.norm."
        moved = lambda rec: (rec["buffers"][pre + "running_var"] - (1 - TS.BN_MOMENTUM) * sd0[pre + "running_var"].double().numpy()) / TS.BN_MOMENTUM   # noqa: E731
        # unbiased over n_total = 2 n rows: biased var * 2n / (2n - 1) against biased var * n / (n - 1)
        assert np.allclose(moved(two) * (2 * n - 1) / (2 * n), moved(one) * (n - 1) / n, rtol=1e-10, atol=1e-14)
        assert np.allclose(two["buffers"][pre + "running_mean"], one["buffers"][pre + "running_mean"], rtol=1e-13, atol=1e-16)
        assert two["buffers"][pre + "num_batches_tracked"] == one["buffers"][pre + "num_batches_tracked"] == 1


@pytest.mark.parametrize("arch", list(TS.ARCHS))
def test_the_shards_meet_the_conditions_and_float32_is_an_fp32_error(arch, tmp_path_factory):
    c = _case(arch, tmp_path_factory)
    assert len(c["batches"]) == 2 and all(len(step) == DS.W and all(b[0].shape[0] == TS.B for b in step) for step in c["batches"])
    got = DS.check_conditions(arch, c["r64"])
    for key, v in got.items():
        print(arch, "step %d rank %d %-6s" % key, ("min|z| %.2e = %.0f tie bounds" if arch == "DCMHT" else "%d cosines, nearest %.2e from the threshold") % v)
    assert len(c["r64"]) == DS.STEPS
    null = TS.null_set(c["r64"])
    assert null == (TS.NULL_DCMHT if arch == "DCMHT" else ())
    per, pooled, noise = DS.yardstick(arch, c["sd0"], c["batches"], c["r64"], c["masks"], null)
    print("\n".join(TS.table(arch + " W=2", pooled)))
    for s, errs in enumerate(per):
        for key, e in errs.items():
            assert np.isfinite(e) and e < 1e-2, (arch, s, key, e)
    assert max(e for (q, _), e in pooled.items() if q == "grad") > 2.0 ** -27            # and it is a float32 run
    for rec in c["r64"]:                                                                 # each rank logs its own loss; the step uses the mean
        assert len(rec["losses"]) == DS.W and abs(rec["loss"] - sum(rec["losses"]) / DS.W) <= 1e-15 * abs(rec["loss"])
        assert rec["losses"][0] != rec["losses"][1]
        assert "backbone.logit_scale" not in rec["grad"] and "backbone.logit_scale" not in rec["p"]
