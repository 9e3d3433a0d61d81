"""CPU: the restatement of tests/twdh_transform_cases.py against what the reference's own code computed
(tests/golden/twdh_transform.npz, written by tools/make_golden_twdh_transform.py: Matrix, hash_center_multilables, hash_convert,
BertAdam imported, soft_argmax_hash_loss and check compiled from the generator's train.py), and its `check` on the two shipped
transforms of tests/golden/twdh_transform_shipped.npz.

The reference runs in float32.  Its objective has an ill-conditioned place (BCELoss' backward divides by max(p (1 - p), 1e-12), and
1 - p loses every digit as p approaches 1), so its gradient stands 1e-5 to 3e-4 of max|g| from the float64 one; the float32 run of
the restatement shows the same figure and stands 1e-7 to 3e-7 from the reference in the gradients and moments (measured when the
golden was written; the golden records that it is not bit-equal).  The assertions are the project's rule turned round: the reference lies within TOL_FACTOR float32
yardsticks of the float64 restatement, as the port must."""
import numpy as np
import pytest

import twdh_transform_cases as TT


@pytest.fixture(scope="module")
def golden():
    g = np.load(TT.GOLDEN)
    inp = TT.trajectory_inputs(int(g["seed"]))
    return g, inp, TT.run(inp), TT.run(inp, np.float32)


def test_the_stored_draws_are_the_case_builders(golden):
    g, inp, _, _ = golden
    assert int(g["seed"]) == TT.TRAJ_SEED
    assert np.array_equal(g["M0"], inp["M0"]) and np.array_equal(g["labels"], inp["labels"])
    assert np.array_equal(g["long_c"], inp["long_c"]) and np.array_equal(g["short_c"], inp["short_c"])
    n = len(g["terms"])
    assert np.array_equal(g["ties_long"], np.stack([inp["ties"][s][0] for s in range(n)]))
    assert np.array_equal(g["ties_short"], np.stack([inp["ties"][s][1] for s in range(n)]))
    flat = np.concatenate([np.concatenate(inp["batches"][e]) for e in range(int(g["epoch"]) + 1)])
    assert np.array_equal(g["batches"], flat)
    sizes = [len(b) for b in inp["batches"][0]]
    assert sizes == [64, 64, 64, 8] and int(g["per_epoch"]) == 4          # the last partial batch is kept


def test_targets_equal_the_references(golden):
    g, inp, r64, _ = golden
    mine = np.concatenate([r64["steps"][s]["bits"] for s in range(TT.TRAJ_STEPS)])
    assert np.array_equal(mine, g["bits"])


def test_the_reference_follows_the_float64_restatement_within_the_float32_yardstick(golden):
    g, inp, r64, r32 = golden
    problems = []
    for s in range(TT.TRAJ_STEPS):
        ref, ref32 = r64["steps"][s], r32["steps"][s]
        got = {k: g[k][s] for k in ("grad", "clipped", "M", "m", "v")}
        if not np.abs(g["terms"][s] - ref["terms"]).max() <= 5e-5 * np.abs(ref["terms"]).max() + 1e-6:
            problems.append((s, "terms", g["terms"][s].tolist(), ref["terms"].tolist()))
        if not abs(g["next_lr"][s] - ref["next_lr"]) <= 1e-15:
            problems.append((s, "get_lr", g["next_lr"][s], ref["next_lr"]))
        for q in TT.QUANTITIES:
            want = TT.quantity(ref, q, inp["M0"])
            e, e_ref = TT.rel_err(TT.quantity(got, q, inp["M0"]), want), TT.rel_err(TT.quantity(ref32, q, inp["M0"]), want)
            if not e <= TT.TOL_FACTOR * e_ref:
                problems.append((s, q, e, e_ref))
    assert not problems, problems[:8]
    assert not np.any(g["M"][0] != inp["M0"])                             # step 0 runs at rate 0


def test_the_reference_and_the_restatement_stop_lossless(golden):
    g, inp, r64, r32 = golden
    assert bool(g["passed"][-1]) and not g["passed"][:-1].any() and int(g["epoch"]) <= 60
    assert r64["lossless"] and r64["epoch"] < inp["post_epochs"]
    assert not TT.check(g["M_final"], inp["long_c"], inp["short_c"])[0].any()
    print("stopping epoch: reference %d, float64 restatement %d, float32 restatement %d" % (int(g["epoch"]), r64["epoch"], r32["epoch"]))


@pytest.mark.parametrize("ds, want", [("coco", [(70, 2), (70, 3)]), ("nuswide", [])])
def test_check_on_the_shipped_transforms(ds, want):
    f = np.load(TT.SHIPPED)
    lc, sc, M = f[ds + "__long"], f[ds + "__short"], f[ds + "__trans"]
    assert lc.dtype == np.int8 and sc.dtype == np.int8 and M.shape == (2 * lc.shape[1], 2 * sc.shape[1]) == (1024, 32)
    wrong, margin = TT.check(M, lc, sc)
    assert margin == float(f[ds + "__margin"]) and margin > TT.order_bound(M)
    assert [tuple(x) for x in np.argwhere(wrong)] == want == [tuple(x) for x in f[ds + "__wrong"]]
    # the same verdict in float32, whose summation order cannot move a logit across the margin
    assert np.array_equal(TT.check(M, lc, sc, np.float32)[0], wrong)


def test_equal_logits_give_bit_zero():
    lc = np.array([[1, -1, 1]], np.int8)
    M = np.zeros((6, 4), np.float32)
    M[:, 2], M[:, 3] = 0.5, 0.25                                           # pair 0: equal logits; pair 1: z0 > z1
    assert not TT.check(M, lc, np.array([[-1, -1]], np.int8))[0].any()
    assert TT.check(M, lc, np.array([[1, -1]], np.int8))[0].tolist() == [[True, False]]


def test_objective_gradient_is_the_derivative():
    """central differences of the float64 objective, on a case with ties and an unlabelled row (no entry of its M is zero, where |M|
    has no derivative)"""
    c = TT.build("ties_and_empty")
    M = c["M"].astype(np.float64)
    o = TT.objective(M, c["bits"], c["L"], c["S"])
    rng = np.random.default_rng(5)
    for _ in range(40):
        i, j = rng.integers(0, M.shape[0]), rng.integers(0, M.shape[1])
        h = 1e-6
        P, N = M.copy(), M.copy()
        P[i, j] += h
        N[i, j] -= h
        num = (TT.objective(P, c["bits"], c["L"], c["S"])["terms"][0] - TT.objective(N, c["bits"], c["L"], c["S"])["terms"][0]) / (2 * h)
        assert abs(num - o["dM"][i, j]) <= 1e-6 * max(1.0, abs(num)), (i, j, num, o["dM"][i, j])
