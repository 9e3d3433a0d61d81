"""GPU: the stage that makes TwDH's transforms (xmh/models/twdh_transform.py over xmh_twdh_trans_loss / _grad / _check, xmh_twdh_targets
and the fused BertAdam) against the float64 restatement of tests/twdh_transform_cases.py.

One step (loss terms and dM through transform_loss and autograd, the packed targets of xmh_twdh_targets compared word for word first)
on the cases straddle (7 x 40 x 12 x 5: the short stream starts inside a target word, B below one tile), tile_edge (12 x 96 x 16 x 67),
wide (80 x 2048 x 64 x 200, the reference's largest shape), ties_and_empty (zero sums with each tie value in both streams, a row
without a label), saturated (|z0 - z1| = 120 on the wrong side and on the right side of two pairs: the -100 clamp of the log and the
1e-12 clamp of the BCE gradient), zeros_and_signs (exact zeros and negative entries of M) and nan (one NaN entry: a NaN total, NaN in
dM exactly where the restatement's rule puts it -- the entry itself and the two columns of its pair in the rows that a reached batch
row selects -- and every other entry compared).  Then: two calls on equal inputs are bit-equal; upstream and accumulate; every XMH_E*
code at its limit.

Fidelity (xmh_twdh_trans_check through transform_fidelity and TwDH.transform_fidelity): the shipped coco 512 -> 16 transform gets
exactly 2 bits wrong, (class 70, bits 2 and 3), the nuswide one none; the stored float64 margins (0.2187, 2.1233) exceed the bound of
any float32 summation order, L 2^-24 sum_l max|M| (0.0069, 0.0136), which is asserted before the comparison.  Two exactly equal
logits give bit 0.

Trajectory: generate_transform on the replayed draws of twdh_transform_cases.trajectory_inputs (C 12, L 32, S 8, N 200, B 64 -- the last
batch has 8 rows -- post_lr 0.01), recorded with monkeypatches only (BertAdam.step, the module's transform_loss); after each of the first
20 steps the loss terms, the gradient as BertAdam receives it and as it leaves it, M - M0, next_m, next_v and get_lr() (to 1e-15)
against the float64 run.  To the end: the same run stops lossless within 100 epochs, the returned matrix passes the float64 check on
the CPU, transform_fidelity reports 0, <short>.pkl and <short>_zeros.pkl exist, hold the returned matrix and load into TwDH, whose
transform_fidelity() reports 0 too.  The stopping epoch is printed beside the reference's (29) and not asserted equal.

Tolerances.  Per tensor e = max|got - f64| / max|f64|; the yardstick e_ref is the float32 restatement against the float64 one on the
same inputs; the port stays within TOL_FACTOR = 4 of it.  Loss terms: rtol 5e-5 (of the largest term), atol 1e-6.  The float32
objective is ill-conditioned where p rounds to 1 (BCELoss' backward then divides by the 1e-12 floor): e_ref is 3e-2 on straddle and
above 1 on tile_edge and wide, where the rule alone would let an indexing error pass.  The one-step gradients are therefore also held
to ONE_ROUNDING = 4 * 2^-24: the kernels compute every element in double and round once (2^-24 of the element, at most that of the
largest), and the double evaluation itself stands within 1e-12 of numpy's.

Measured on an MI355X (profiles/twdh_transform_f64.txt; every figure is printed before the first assertion, and appended to the file
XMH_TWDH_TRANSFORM_TABLE names).  One step, dM: e_port / e_ref (the bound is 4) and e_port (the bound is 2.384e-7) -- straddle 1.7e-6
(4.71e-8 / 2.73e-2), tile_edge 2.4e-10 (4.44e-8 / 1.83e+2), wide 2.0e-11 (4.58e-8 / 2.28e+3), ties_and_empty 9.2e-5 (4.73e-8 / 5.15e-4),
saturated 3.2e-5 (3.17e-8 / 9.88e-4), zeros_and_signs 4.8e-3 (3.03e-8 / 6.32e-6), nan 1.5e-4 (4.30e-8 / 2.91e-4, 120 NaN entries on
both sides); no packed target word differed; the terms agree to float32's last digits.  Trajectory, worst e_port / e_ref over the 20
steps: grad 0.03, clipped 0.03, delta 0.22, m 0.01, v 0.01 (the float32 restatement carries the ill-conditioned place above, the port
does not; delta is the rounding of the stored float32 matrix on both sides).  The port stops lossless at epoch 29, as the reference
and the float64 restatement do.

The module was seen to fail under each of these edits on a scratch copy of the package (the first failing check of each, then what
else).  The short stream read from bit 0 instead of bit L in k_trans_loss_part and k_trans_gz: the terms of straddle (bce 2.4272
against 3.1476), of every other one-step case, dM of nan (e_port 0.66), upstream / accumulate, the trajectory, and the run does not
end lossless.  The quantisation mean taken over B 2S (k_trans_loss_reduce, and n1 in k_trans_gz): the hash term of straddle (0.5980
against 0.1959) and of every one-step case, dM of nan (e_port 0.087), upstream / accumulate, the trajectory.  sign(M) dropped from dM:
the one-rounding bound on straddle (e_port 1.5e-2), tile_edge (2.4e-2) and wide (0.20) -- the yardstick rule alone passes these three
-- the yardstick rule on the other four (ratios 17 to 2700), upstream / accumulate, the trajectory.  The tie for a zero sum taken as
bit 0 in k_twdh_targets: the packed target words of every one-step case (2 of 10 on straddle, 4026 of 13200 on wide), 35 words at
step 0 of the trajectory.  The last partial batch dropped in generate_transform: the trajectory at step 3 (the 8-row batch: the
packed targets have another shape, then every tensor), and the count of steps in the whole run (87 against 4 x 29).  check comparing
against the long centre's bits in k_trans_check: 636 wrong bits for coco instead of 2, 180 for nuswide instead of 0, the equal-logit
case (171 against 191), the whole run's verdict, and the --check-only output."""
import os
import shutil

import numpy as np
import pytest
import torch

import twdh_transform_cases as TT

pytestmark = pytest.mark.gpu

EINVAL, ENOMEM, ENOTSUP = -22, -12, -95
ONE_ROUNDING = 4 * 2.0 ** -24
DEV = "cuda"


def _np(t):
    return t.detach().cpu().numpy()


def _table(lines):
    print("\n".join(lines))                                                # every figure before the first assertion
    if os.environ.get("XMH_TWDH_TRANSFORM_TABLE"):
        with open(os.environ["XMH_TWDH_TRANSFORM_TABLE"], "a") as f:
            f.write("\n".join(lines) + "\n")


def _device_targets(c):
    from xmh import retrieval as R
    from xmh.models import twdh_transform as X
    centres = torch.tensor(np.concatenate([c["long_c"], c["short_c"]], 1)).to(DEV)
    tie = torch.tensor(np.concatenate([c["tie_l"], c["tie_s"]])).to(DEV)
    lab = R.pack_labels((torch.tensor(c["labels"]) == 1).to(torch.uint8).to(DEV))
    return X.transform_targets(lab, c["C"], centres, tie)


@pytest.fixture(scope="module")
def refs():
    """the float64 and float32 restatements of every one-step case, computed once"""
    out = {}
    for name in TT.ONE_STEP:
        c = TT.build(name)
        out[name] = (c, TT.objective(c["M"], c["bits"], c["L"], c["S"]), TT.objective(c["M"], c["bits"], c["L"], c["S"], dtype=np.float32))
    return out


@pytest.mark.parametrize("name", TT.ONE_STEP)
def test_one_step_against_float64(name, refs):
    from xmh.models import twdh_transform as X
    c, r64, r32 = refs[name]
    targets = _device_targets(c)
    want_words = TT.pack_bits(c["bits"])
    words_differ = int((_np(targets).view(np.uint32) != want_words).sum())
    M = torch.tensor(c["M"], device=DEV, requires_grad=True)
    loss, terms = X.transform_loss(M, targets, c["L"], c["S"], TT.ALPHA)
    loss.backward()
    got_t, got_g = _np(terms).astype(np.float64), _np(M.grad)
    nan64 = np.isnan(r64["dM"])
    fin = ~nan64
    e_port = TT.rel_err(np.where(fin, got_g, 0), np.where(fin, r64["dM"], 0))
    e_ref = TT.rel_err(np.where(fin, r32["dM"], 0), np.where(fin, r64["dM"], 0))
    t_err = np.abs(got_t - r64["terms"])
    _table(["%s target words that differ: %d of %d" % (name, words_differ, want_words.size),
            "%s terms port %s f64 %s" % (name, got_t.tolist(), r64["terms"].tolist()),
            "%s dM e_port %.3e e_ref %.3e ratio %.3g (bound %g); one rounding bound %.3e; NaN entries port %d f64 %d"
            % (name, e_port, e_ref, e_port / e_ref if e_ref else np.inf, TT.TOL_FACTOR, ONE_ROUNDING, int(np.isnan(got_g).sum()), int(nan64.sum()))])
    assert words_differ == 0
    assert np.array_equal(_np(loss), _np(terms[0]), equal_nan=True)
    if name == "nan":
        assert np.isnan(got_t).all() and np.isnan(r64["terms"]).all()     # hash, bce and lasso are all reached
        assert np.array_equal(np.isnan(got_g), nan64)
        cols = np.unique(np.argwhere(nan64)[:, 1])
        assert set(cols) == {TT.NAN_AT[1] & ~1, TT.NAN_AT[1] | 1} and nan64[TT.NAN_AT] and not nan64.all(0)[cols].any()
    else:
        assert not nan64.any() and not np.isnan(got_g).any()
        assert (t_err <= 5e-5 * np.abs(r64["terms"]).max() + 1e-6).all(), (got_t, r64["terms"])
    assert e_port <= TT.TOL_FACTOR * e_ref, (e_port, e_ref)
    assert e_port <= ONE_ROUNDING, e_port
    if name == "zeros_and_signs":                                          # sign(0) = 0: at a zero of M the gradient is the data term alone
        zero = c["M"] == 0
        data = r64["dM"] - TT.ALPHA * np.sign(c["M"].astype(np.float64))
        assert np.abs(got_g[zero] - data[zero]).max() <= ONE_ROUNDING * np.abs(r64["dM"]).max()


def _raw_grad(c, targets, up=None, into=None):
    """xmh_twdh_trans_grad called directly"""
    from xmh._lib import lib, ptr, current_stream, workspace
    M = torch.tensor(c["M"], device=DEV)
    dM = torch.empty_like(M) if into is None else into
    n = lib.xmh_twdh_trans_ws_bytes(c["B"], c["L"], c["S"])
    ws = workspace(n, M.device)
    rc = lib.xmh_twdh_trans_grad(ptr(M), ptr(targets), c["B"], c["L"], c["S"], TT.ALPHA, ptr(up), ptr(dM), int(into is not None), ptr(ws), n,
                                 current_stream())
    assert rc == 0
    return dM


def test_two_calls_on_equal_inputs_are_bit_equal(refs):
    from xmh.models import twdh_transform as X
    for name in ("tile_edge", "wide"):
        c = refs[name][0]
        targets = _device_targets(c)
        outs = []
        for _ in range(2):
            M = torch.tensor(c["M"], device=DEV, requires_grad=True)
            loss, terms = X.transform_loss(M, targets, c["L"], c["S"], TT.ALPHA)
            loss.backward()
            outs.append((_np(terms), _np(M.grad)))
        assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


def test_upstream_and_accumulate_are_honoured(refs):
    from xmh.models import twdh_transform as X
    c, r64, _ = refs["tile_edge"]
    targets = _device_targets(c)
    scale = np.abs(r64["dM"]).max()
    up = torch.tensor([2.5], device=DEV)
    got = _np(_raw_grad(c, targets, up=up))
    assert np.abs(got - 2.5 * r64["dM"]).max() <= ONE_ROUNDING * 2.5 * scale
    rng = np.random.default_rng(3)
    before = (rng.standard_normal(c["M"].shape) * scale).astype(np.float32)
    into = torch.tensor(before, device=DEV)
    got = _np(_raw_grad(c, targets, up=up, into=into))
    want = before.astype(np.float64) + 2.5 * r64["dM"]
    assert np.abs(got - want).max() <= ONE_ROUNDING * np.abs(want).max()
    assert np.abs(_np(_raw_grad(c, targets)) - r64["dM"]).max() <= ONE_ROUNDING * scale           # NULL upstream = 1
    # and through autograd: the gradient of 3 * loss
    M = torch.tensor(c["M"], device=DEV, requires_grad=True)
    (3.0 * X.transform_loss(M, targets, c["L"], c["S"], TT.ALPHA)[0]).backward()
    assert np.abs(_np(M.grad) - 3.0 * r64["dM"]).max() <= ONE_ROUNDING * 3.0 * scale


def test_error_codes_at_their_limits():
    """the checks run before anything is launched: the pointers are never dereferenced"""
    from oracle.fixtures import aligned_host
    from xmh._lib import lib
    _, p = aligned_host(64)
    loss = lambda B, L, S, ws=p, n=1 << 40, M=p: lib.xmh_twdh_trans_loss(M, p, B, L, S, 1e-3, ws, n, p, None)      # noqa: E731
    grad = lambda B, L, S, ws=p, n=1 << 40, dM=p: lib.xmh_twdh_trans_grad(p, p, B, L, S, 1e-3, None, dM, 0, ws, n, None)      # noqa: E731
    chk = lambda C, L, S, w=p: lib.xmh_twdh_trans_check(p, p, C, L, S, w, None)      # noqa: E731
    for f in (loss, grad):
        assert f(0, 8, 4) == EINVAL and f(4, 0, 4) == EINVAL and f(4, 8, 0) == EINVAL
        assert f(4, 8, 4, ws=None) == EINVAL
        assert f(4097, 8, 4) == ENOTSUP and f(4, 4000, 97) == ENOTSUP and f(4, 4096, 1) == ENOTSUP
        need = lib.xmh_twdh_trans_ws_bytes(4096, 4000, 96)
        assert need > 0 and f(4096, 4000, 96, n=need - 1) == ENOMEM
        assert b"xmh_twdh_trans" in lib.xmh_last_error()
    assert loss(4, 8, 4, M=None) == EINVAL and grad(4, 8, 4, dM=None) == EINVAL
    assert lib.xmh_twdh_trans_ws_bytes(4097, 8, 4) == 0 and lib.xmh_twdh_trans_ws_bytes(4, 4000, 97) == 0
    assert lib.xmh_twdh_trans_ws_bytes(0, 8, 4) == 0 and lib.xmh_twdh_trans_ws_bytes(4096, 4095, 1) > 0
    assert chk(0, 8, 4) == EINVAL and chk(4, 8, 4, w=None) == EINVAL
    assert chk(1025, 8, 4) == ENOTSUP and chk(4, 4000, 97) == ENOTSUP


def test_shape_mismatches_name_both_shapes():
    from xmh.models import twdh_transform as X
    M = torch.zeros(80, 24, device=DEV)
    with pytest.raises(ValueError, match=r"\(80, 24\).*\[80, 26\]"):
        X.transform_loss(M, torch.zeros(5, 2, dtype=torch.int32, device=DEV), 40, 13)
    with pytest.raises(ValueError, match=r"\(5, 3\).*\(80, 24\)"):
        X.transform_loss(M, torch.zeros(5, 3, dtype=torch.int32, device=DEV), 40, 12)
    lc, sc = torch.ones(7, 40), torch.ones(7, 12)
    with pytest.raises(ValueError, match=r"\(80, 26\).*\(7, 40\).*\(7, 12\)"):
        X.transform_fidelity(lc, sc, torch.zeros(80, 26))
    with pytest.raises(ValueError, match=r"\(7, 40\).*\(6, 12\)"):
        X.transform_fidelity(lc, torch.ones(6, 12), M)
    with pytest.raises(ValueError, match=r"\(9, 8\).*\(7, 52\)"):
        X.generate_transform(torch.ones(9, 8), lc, sc)
    with pytest.raises(ValueError, match="hash centre"):
        X.transform_fidelity(lc * 0.5, sc, M)


# ---- fidelity --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ds, want", [("coco", [(70, 2), (70, 3)]), ("nuswide", [])])
def test_fidelity_of_the_shipped_transforms(ds, want):
    from xmh.models import twdh_transform as X
    f = np.load(TT.SHIPPED)
    lc, sc, M = f[ds + "__long"], f[ds + "__short"], f[ds + "__trans"]
    margin, bound = float(f[ds + "__margin"]), TT.order_bound(M)
    n, wrong = X.transform_fidelity(torch.tensor(lc), torch.tensor(sc), torch.tensor(M))
    _table(["%s 512 -> 16: smallest float64 margin %.4f, bound of any float32 order %.4f; wrong bits on the device %d at %s"
            % (ds, margin, bound, n, np.argwhere(wrong.numpy()).tolist())])
    assert margin > bound                                                  # no summation order can change a decision
    assert wrong.shape == (lc.shape[0], 16) and wrong.dtype == torch.bool
    assert n == len(want) and [tuple(x) for x in np.argwhere(wrong.numpy())] == want


def test_equal_logits_give_bit_zero_and_every_word_of_the_bitmap_is_written():
    from xmh.models import twdh_transform as X
    rng = np.random.default_rng(11)
    C, L, S = 5, 9, 70                                                     # three words of bitmap per class, the last one partial
    lc, sc = rng.integers(0, 2, (C, L)) * 2 - 1, rng.integers(0, 2, (C, S)) * 2 - 1
    M = rng.integers(-3, 4, (2 * L, 2 * S)).astype(np.float32)             # small integers: the logits are exact and many pairs are equal
    want, _ = TT.check(M, lc, sc)
    z = (TT.one_hot(lc > 0, np.float64) @ M).reshape(C, S, 2)
    equal = z[..., 0] == z[..., 1]
    assert equal.sum() > 10 and (equal & (sc > 0)).any() and (equal & (sc < 0)).any()
    n, wrong = X.transform_fidelity(torch.tensor(lc), torch.tensor(sc), torch.tensor(M))
    assert n == int(want.sum()) and np.array_equal(wrong.numpy(), want)
    assert np.array_equal(wrong.numpy()[equal], (sc > 0)[equal])           # an equal pair decides 0: wrong exactly where the centre says 1


# ---- trajectory and the whole run --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def whole_run(tmp_path_factory):
    """one generate_transform run on the replayed draws, to its end, with the first TRAJ_STEPS steps recorded"""
    from xmh.models import twdh_transform as X
    from xmh.optim import BertAdam
    inp = TT.trajectory_inputs()
    save_dir = str(tmp_path_factory.mktemp("trans"))
    steps, seen = [], []
    step, loss_fn = BertAdam.step, X.transform_loss

    def recording_loss(M, targets, L, S, alpha=1e-3):
        out = loss_fn(M, targets, L, S, alpha)
        seen.append((out[1].clone(), targets.clone()))
        return out

    def recording_step(self, closure=None):
        p = self.param_groups[0]["params"][0]
        rec = {"grad": p.grad.detach().clone()} if len(steps) < TT.TRAJ_STEPS else None
        ret = step(self, closure)
        if rec is not None:
            st = self.state[p]
            rec.update(clipped=p.grad.detach().clone(), M=p.detach().clone(), m=st["next_m"].clone(), v=st["next_v"].clone(),
                       next_lr=self.get_lr()[0], t_total=self.param_groups[0]["t_total"])
            steps.append(rec)
        return ret
    mp = pytest.MonkeyPatch()
    mp.setattr(BertAdam, "step", recording_step)
    mp.setattr(X, "transform_loss", recording_loss)
    try:
        lines = []
        out = X.generate_transform(torch.tensor(inp["labels"]), torch.tensor(inp["long_c"]), torch.tensor(inp["short_c"]), batch_size=inp["B"],
                                   post_epochs=inp["post_epochs"], post_lr=inp["post_lr"], init=torch.tensor(inp["M0"]), batches=inp["batches"],
                                   ties=inp["ties"], save_dir=save_dir, logger=lines.append)
    finally:
        mp.undo()
    port = [{k: (_np(v) if torch.is_tensor(v) else v) for k, v in r.items()} for r in steps]
    terms = [_np(t).astype(np.float64) for t, _ in seen]
    words = [_np(w).view(np.uint32) for _, w in seen[:TT.TRAJ_STEPS]]
    return dict(inp=inp, out=out, port=port, terms=terms, words=words, save_dir=save_dir, lines=lines, r64=TT.run(inp), r32=TT.run(inp, np.float32))


def test_twenty_steps_follow_the_float64_trajectory(whole_run):
    w = whole_run
    inp, r64, r32, port = w["inp"], w["r64"], w["r32"], w["port"]
    assert len(port) == TT.TRAJ_STEPS and [len(b) for b in inp["batches"][0]] == [64, 64, 64, 8]
    lines, problems, worst = [], [], {}
    for s in range(TT.TRAJ_STEPS):
        ref, ref32, rec = r64["steps"][s], r32["steps"][s], port[s]
        differ = int((w["words"][s] != TT.pack_bits(ref["bits"])).sum()) if w["words"][s].shape == TT.pack_bits(ref["bits"]).shape else -1
        if differ:
            problems.append((s, "packed targets", differ))
        t = w["terms"][s]
        lines.append("step %2d rows %d terms port %s f64 %s  lr %.6e" % (s, len(ref["bits"]), t.tolist(), ref["terms"].tolist(), rec["next_lr"]))
        if not (np.abs(t - ref["terms"]) <= 5e-5 * np.abs(ref["terms"]).max() + 1e-6).all():
            problems.append((s, "terms", t.tolist(), ref["terms"].tolist()))
        if not abs(rec["next_lr"] - ref["next_lr"]) <= 1e-15 or rec["t_total"] != inp["t_total"]:
            problems.append((s, "get_lr", rec["next_lr"], ref["next_lr"], rec["t_total"]))
        for q in TT.QUANTITIES:
            want = TT.quantity(ref, q, inp["M0"])
            e, e_ref = TT.rel_err(TT.quantity(rec, q, inp["M0"]), want), TT.rel_err(TT.quantity(ref32, q, inp["M0"]), want)
            lines.append("step %2d %-7s e_port %.3e e_ref %.3e ratio %.3g" % (s, q, e, e_ref, e / e_ref if e_ref else (0.0 if e == 0 else np.inf)))
            if e_ref:
                worst[q] = max(worst.get(q, 0.0), e / e_ref)
            if not e <= TT.TOL_FACTOR * e_ref:
                problems.append((s, q, "e_port %.2e" % e, "e_ref %.2e" % e_ref))
    if not np.array_equal(port[0]["M"], inp["M0"]):
        problems.append((0, "step 0 runs at rate 0 and moved the matrix"))
    lines.append("worst e_port / e_ref per quantity over %d steps: %s" % (TT.TRAJ_STEPS, " ".join("%s %.2f" % kv for kv in sorted(worst.items()))))
    lines += ["problem %s" % (p,) for p in problems]
    _table(lines)
    assert not problems, (len(problems), problems[:10])


def test_the_run_ends_lossless_and_its_files_load_into_twdh(whole_run, tmp_path):
    from xmh.models import twdh_transform as X
    from xmh.models.twdh import TwDH
    w = whole_run
    inp, out = w["inp"], w["out"]
    g = np.load(TT.GOLDEN)
    _table(["stopping epoch: port %d, reference %d, float64 restatement %d; epochs logged %d; last line %r"
            % (out.epoch, int(g["epoch"]), w["r64"]["epoch"], len(out.terms), w["lines"][-1])])
    assert out.lossless and out.epoch < 100 and out.terms.shape == (out.epoch + 1, 4) and np.isfinite(out.terms).all()
    assert out.matrix.dtype == torch.float32 and not out.matrix.is_cuda and tuple(out.matrix.shape) == (64, 16)
    wrong, _ = TT.check(out.matrix.numpy(), inp["long_c"], inp["short_c"])
    assert not wrong.any()                                                 # the float64 check on the CPU
    n, bits = X.transform_fidelity(torch.tensor(inp["long_c"]), torch.tensor(inp["short_c"]), out.matrix)
    assert n == 0 and not bits.any()
    # every epoch of the run was a whole one: 4 batches, the last of 8 rows (a dropped partial batch would leave 3 steps per epoch)
    assert len(w["terms"]) == 4 * (out.epoch + 1)
    files = [os.path.join(w["save_dir"], "32", n) for n in ("8.pkl", "8_zeros.pkl")]
    for f in files:
        assert os.path.isfile(f) and torch.equal(torch.load(f), out.matrix)
    assert sorted(os.listdir(os.path.join(w["save_dir"], "32"))) == ["8.pkl", "8_zeros.pkl"]
    # through the config, as a user would: trans_matrix/<long>/<short>.pkl, long_center/<long>.pkl, short_center/<short>.pkl
    from xmh.utils.config import Config
    for d in ("trans/32", "long", "short"):
        os.makedirs(str(tmp_path / d))
    shutil.copy(files[0], str(tmp_path / "trans" / "32" / "8.pkl"))
    torch.save(torch.tensor(inp["long_c"]).float(), str(tmp_path / "long" / "32.pkl"))
    torch.save(torch.tensor(inp["short_c"]).float(), str(tmp_path / "short" / "8.pkl"))
    small = "synthetic:1814:vision_layers=1,transformer_layers=1,vision_width=128,transformer_width=128,embed_dim=64,image_resolution=64"
    m = TwDH.from_config(Config({"clip_path": small, "long_dim": 32, "trans_matrix": str(tmp_path / "trans"), "long_center": str(tmp_path / "long"),
                                 "short_center": str(tmp_path / "short"), "num_classes": 12}), output_dim=8)
    assert list(m.trans) == ["8"] and torch.equal(m.trans["8"], out.matrix)
    fid = m.transform_fidelity()
    assert list(fid) == ["8"] and fid["8"][0] == 0 and not fid["8"][1].any()


# ---- the command-line entry ------------------------------------------------------------------------------------------------------------
def _tool():
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "twdh_make_transform.py")
    spec = importlib.util.spec_from_file_location("twdh_make_transform", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_check_only_prints_the_wrong_bits_of_a_directory_laid_out_like_the_references(tmp_path, capsys):
    f = np.load(TT.SHIPPED)
    for ds in ("coco", "nuswide"):
        for d in ("long", "short", "trans/512"):
            os.makedirs(str(tmp_path / ds / d))
        torch.save(torch.tensor(f[ds + "__long"]).float(), str(tmp_path / ds / "long" / "512.pkl"))
        torch.save(torch.tensor(f[ds + "__short"]).float(), str(tmp_path / ds / "short" / "16.pkl"))
        torch.save(torch.tensor(f[ds + "__trans"]), str(tmp_path / ds / "trans" / "512" / "16.pkl"))
    torch.save(torch.zeros(1024, 64), str(tmp_path / "coco" / "trans" / "512" / "32.pkl"))       # no short centre beside it: skipped
    tool = _tool()
    args = lambda ds: ["--check-only", "--long-dim", "512", "--long-center-path", str(tmp_path / ds / "long"),      # noqa: E731
                       "--short-center-path", str(tmp_path / ds / "short"), "--save-dir", str(tmp_path / ds / "trans")]
    assert tool.main(args("coco")) == 1
    out = capsys.readouterr().out
    assert "16.pkl: 2 wrong of 1280 (class, bit) at [(70, 2), (70, 3)]" in out and "32.pkl: no short centre for it, skipped" in out
    assert tool.main(args("nuswide") + ["--output-dim", "16"]) == 0
    assert "16.pkl: 0 wrong of 336 (class, bit): lossless" in capsys.readouterr().out


def test_the_tool_trains_from_a_label_file_and_writes_the_layout_twdh_reads(tmp_path, capsys):
    import scipy.io as scio
    inp = TT.trajectory_inputs()
    scio.savemat(str(tmp_path / "label.mat"), {"category": inp["labels"]})
    torch.save(torch.tensor(inp["long_c"]).float(), str(tmp_path / "32.pkl"))
    torch.save(torch.tensor(inp["short_c"]).float(), str(tmp_path / "8.pkl"))
    argv = ["--label-file", str(tmp_path / "label.mat"), "--query-num", "40", "--train-num", "100", "--seed", "3", "--batch-size", "64",
            "--post-epochs", "2", "--long-dim", "32", "--output-dim", "8", "--post-lr", "0.01", "--long-center-path", str(tmp_path / "32.pkl"),
            "--short-center-path", str(tmp_path / "8.pkl"), "--save-dir", str(tmp_path / "out")]
    tool = _tool()
    assert tool.main(argv) == 0
    first = capsys.readouterr().out
    M = torch.load(str(tmp_path / "out" / "32" / "8.pkl"))
    assert M.dtype == torch.float32 and tuple(M.shape) == (64, 16) and not M.is_cuda and "epoch 1:" in first and "epoch 2:" not in first
    assert tool.main(argv) == 0                                            # the seed fixes the split, the matrix, the order and the ties
    assert torch.equal(torch.load(str(tmp_path / "out" / "32" / "8.pkl")), M) and capsys.readouterr().out == first
