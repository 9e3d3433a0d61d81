"""GPU: whole training steps of DIMCHTrainer.train_epoch (both CLIP towers through their token outputs, the image tokens with the cls
row first, the token-set head of both modalities with its drawn dropout masks, the set-distance objective, the backward through the
objective, the heads and both towers' token backward, the fused BertAdam step over two groups) against the float64 restatement of
tests/dimch_train_step_cases.py: five steps, each its own train_epoch call on the loader's three batches in turn, on the two cases
`smooth` (tanh, smooth_chamfer, setDim 3, dropout 0.3) and `softmax` (the pair softmax at 24 columns, the hard-max chamfer distance,
setDim 8, no dropout).

Recorded with monkeypatches only: BertAdam.step (the gradients as the optimiser receives them), the trainer's compute_loss (the four
head outputs and the loss), the model's object_function (loss_dict), draw_keep_mask of each head module (the masks) and
DIMCHTokenHash._run (the buffer the train forward fills: the two relu outputs, at the place include/xmh.h and dimch_saved_layout give --
c [B M, E], then a [B M, H] after the dropout, every section rounded up to 256 bytes).  torch.manual_seed(MASK_SEED + s) before step s;
the loader is a list.  The restatement runs on the CPU before the device's first step, on the seeded replay of the masks; nothing is
rerun under the port's own decisions.  The conditions on the inputs are re-asserted on the float64 run before any comparison.

After every step.  Draws: exactly one mask per head and step in the order image then text, each equal to the seeded replay of the
same torch.rand(...) >= p calls; `softmax` draws none (draw_keep_mask returns None).  Loss and log: the loss compute_loss returned,
the epoch's four-decimal log line, every scalar of loss_dict against the float64 terms, All loss being the loss.  Head outputs:
img_embeds, img_hash, txt_embeds, txt_hash as compute_loss receives them.  Optimiser state: p.grad of every parameter as
optimizer.step() receives it and as it leaves it (clipped), delta = p - p_initial, next_m / next_v / step, optimizer.get_lr() in
parameter-group order, t_total.  Exact: logit_scale bit-unchanged, without gradient and without state; the set of parameters with a
gradient; absent token ids and positional rows at or beyond L exact zeros in grad, clipped, m and v; step 0 moving nothing and filling
the moments; the relu decisions of both relus of both heads equal to the float64 run's wherever the mask keeps the entry, and an exact
zero where it drops it -- a differing decision is a problem.

Tolerances.  Per tensor e = max|got - f64| / max|f64|.  Per quantity and tensor kind (train_step_cases.kind_of, pooled over steps
and layers; each of the twelve head tensors a kind of its own, but their delta pooled per head, for the reason and with the two runs'
figures that tests/dimch_train_step_cases.py gives; the four head outputs under `codes`) the yardstick e_ref is the float32
restatement against the float64 one on these very inputs and masks: the port must stay within TOL_FACTOR = 4 times that, the rule and
factor of tests/test_gpu_train_step.py.  The loss and the scalars of loss_dict (relative to the largest term) go by that rule as well,
under `loss` and `terms`, and besides by rtol 5e-5, atol 1e-6 as in the three other trajectory modules.  The null set is empty in both
cases (tests/test_dimch_train_step_cpu.py pins it), so no tensor goes by an absolute rule.

Measured on an MI355X (profiles/dimch_train_step_f64.txt), worst e_port / e_ref per quantity (the bound is 4) -- smooth: codes 1.44
(txt_hash), grad 3.41 (the text block's out_proj.bias; the text tower's kinds lie between 1.1 and 3.4, every other kind at 2.20 or below),
clipped 3.16, delta 2.88, m 2.36, v 2.66, loss 1.20 (4.0e-7 relative), terms 1.20; softmax: codes 1.22, grad 1.20, clipped 1.20, delta
1.57, m 1.58, v 1.87 (the image tower's ln_pre.weight), loss 0.31 (1.1e-7), terms 0.31.  Every drawn mask equalled the replay and no
relu decision differed (1027 to 1054 decisions a head and step in smooth, 6144 in softmax).  The conditions with the device's masks --
smooth: hinge 2.5e-4 against 8.8e-7, 1 - s 0.59 against 3.9e-7, the four relus 1.6e-4 to 3.9e-4 against 5.5e-6 to 9.7e-6 (the narrowest
ratio 29); softmax as in tests/test_dimch_train_step_cpu.py (it has no mask).  As first written, with every head tensor's delta a kind
of its own, smooth missed at one place: the delta of hash.img_token_hash.hash_layer.0.bias at step 1, e_port 3.93e-5 against e_ref
8.95e-6, ratio 4.40, with grad, clipped, m and v of that tensor at 1.43, 1.14, 1.52 and 1.46; the measure was at fault, not the port --
the same float32 restatement run on another CPU gives 2.15e-5 for that yardstick (tests/dimch_train_step_cases.py) -- and pooled per
head the ratio is 1.60.

The module was seen to fail under each of these edits on a scratch copy of the package (the first failing check of each, then what
else; the loss of step 0 is 20.11831 in smooth and 19.25919 in softmax).  _image_tokens putting the cls row last: the relu decisions
of the image head at step 0 (526 of 1035 in smooth, 2674 of 6144 in softmax), then the loss at step 0 (22.92401; 19.40481), its
terms, img_embeds and img_hash, every gradient.  The text head handed the image head's keep mask (smooth; softmax draws none and
passes): "the mask the head was handed is not the replay" for the text head at every step -- the draws themselves still equal the
replay --, then the loss at step 0 (19.86125) and every gradient.  The 1 / (1 - p) of the train forward dropped (smooth; softmax
passes): the loss at step 0 (20.38746), its terms, all four head outputs and every gradient at step 0; relu decisions from step 2 on.
The cls gradient passed as zeros into the image tower's token backward: grad, clipped, m and v of the image tower's 20 (smooth) and 32
(softmax) tensors at step 0, loss, head outputs and the other gradients of step 0 untouched; their delta at step 1; everything from step
2 on.  The head group given backbone_lr: get_lr after steps 0 to 3 (after step 4 both rates are 0), then the delta of the twelve head
tensors at step 1, everything from step 2 on.  optimizer.zero_grad() removed from _train_epoch: absent token ids in grad and clipped
at step 1, every gradient from step 1 on.  From step 2 on each of them also flips relu decisions, which the module reports.

Every figure is printed before the first assertion; with XMH_DIMCH_TRAIN_STEP_TABLE naming a file the table is appended to it
(profiles/dimch_train_step_f64.txt was written so)."""
import os
import re

import numpy as np
import pytest
import torch

import dimch_train_step_cases as DS

pytestmark = pytest.mark.gpu

TOL_FACTOR = DS.TOL_FACTOR
TOK, POS = "backbone.token_embedding.weight", "backbone.positional_embedding"


def _np(t):
    return t.detach().cpu().numpy()


def _relus_of_saved(saved, B, M, E, H):
    """(c > 0 [B, M, E], a > 0 [B, M, H]) from the buffer of xmh_head_dimch_train_forward (c [B M, E], a [B M, H] after the dropout,
    then the pooled pre-activation; every section rounded up to 256 bytes)"""
    a256 = lambda v: (v + 255) & ~255                                                    # noqa: E731
    nc, na = B * M * E * 4, B * M * H * 4
    c = saved[:nc].clone().view(torch.float32).reshape(B, M, E).cpu().numpy()
    a = saved[a256(nc):a256(nc) + na].clone().view(torch.float32).reshape(B, M, H).cpu().numpy()
    return c > 0, a > 0


def _record(t, names, pre, seen, loss_dict):
    """the trainer's state after a step in the layout of a restatement record"""
    outs, loss = seen
    rec = {k: {} for k in ("grad", "clipped", "p", "m", "v")}
    rec["loss"], rec["step"], rec["buffers"] = float(loss), {}, {}
    for n, p in names.items():
        st = t.optimizer.state[p]
        rec["step"][n] = st.get("step")
        if p.grad is None:
            continue
        rec["grad"][n], rec["clipped"][n], rec["p"][n] = _np(pre[n]), _np(p.grad), _np(p)
        rec["m"][n], rec["v"][n] = _np(st["next_m"]), _np(st["next_v"])
    d = loss_dict
    terms = [d["All loss"], d["Tokens"]["Similarity"]["i2t"], d["Tokens"]["Similarity"]["t2i"], d["Tokens"]["Maximum Mean Discrepancy"],
             d["Tokens"]["Diversity"], d["Hash"]["Triplet"]["i2t"], d["Hash"]["Triplet"]["t2i"], d["Hash"]["Quantization"]["image"],
             d["Hash"]["Quantization"]["text"]]
    rec["terms"] = np.array([float(x) for x in terms])
    rec["outs"] = [_np(outs[k]) for k in DS.OUTS]
    return rec


def _structure(s, rec, cap, ref, ids_seen, names, t, problems):
    """the exact zeros and bit equalities of the CPU module's structure list, on the device"""
    def bad(cond, *what):
        if cond:
            problems.append((s,) + what)
    sd0 = cap["sd0"]
    p = names["backbone.logit_scale"]
    bad(not torch.equal(p.detach().cpu(), sd0["backbone.logit_scale"]) or p.grad is not None or len(t.optimizer.state[p]) != 0, "logit_scale")
    bad(sorted(rec["grad"]) != sorted(ref["grad"]), "the parameters with a gradient", sorted(set(rec["grad"]) ^ set(ref["grad"])))
    bad(any(v != s + 1 for n, v in rec["step"].items() if n != "backbone.logit_scale"), "step counters")
    by_id = {id(q): n for n, q in names.items()}
    in_opt = [q for g in t.optimizer.param_groups for q in g["params"]]
    order = [by_id.get(id(q)) for q in in_opt if q.grad is not None]
    want = [ref["next_lr"][DS.group_of(n)] for n in order if n is not None]
    got = t.optimizer.get_lr()
    bad(len(got) != len(want) or not np.allclose(got, want, rtol=1e-15, atol=0), "get_lr", sorted(set(got)), sorted(set(want)))
    bad({g["t_total"] for g in t.optimizer.param_groups} != {DS.STEPS}, "t_total")
    bad(sorted(by_id.get(id(q), "?") for q in in_opt) != sorted(names), "the optimiser's parameters")
    ids = ids_seen[-1]
    vocab = sd0[TOK].shape[0]
    for kind in ("grad", "clipped", "m", "v"):
        if TOK not in rec[kind] or POS not in rec[kind]:
            continue                                                                     # reported above, with the parameters with a gradient
        seen = np.unique(ids if kind in ("grad", "clipped") else np.concatenate(ids_seen))
        absent = np.setdiff1d(np.arange(vocab), seen)
        bad(rec[kind][TOK][absent].any(), kind, "absent token ids")
        bad(rec[kind][POS][ids.shape[1]:].any(), kind, "positional rows >= L")
    if s == 0:                                                                           # rate 0: nothing moves, the moments are filled
        for n in rec["m"]:
            bad(not np.array_equal(rec["p"][n], sd0[n].numpy()), "step 0 moved", n)
            bad(not rec["m"][n].any() or not rec["v"][n].any(), "step 0 left the moments empty", n)


@pytest.mark.parametrize("case", list(DS.CASES))
def test_five_dimch_training_steps_follow_the_float64_trajectory(case, tmp_path, monkeypatch):
    from xmh.models.dimch import DIMCHTokenHash
    from xmh.optim import BertAdam
    t = DS.trainer(case, tmp_path, 0)
    cap = DS.capture(t, case)
    sd0 = cap["sd0"]
    replay = DS.draw_masks(cap, device=t.model.hash.img_token_hash.token_layer.weight.device)
    r64 = DS.run(cap, replay)
    r32 = DS.run(cap, replay, dtype=torch.float32)
    cond = DS.check_conditions(cap, r64, r32)                                            # before any comparison
    assert DS.null_set(r64) == ()
    _, e_ref, _ = DS.yardstick(cap, r64, r32)

    model = t.model
    names = dict(model.named_parameters())
    heads = {"img": model.hash.img_token_hash, "txt": model.hash.txt_token_hash}
    assert all(n.startswith("backbone.") or n.startswith("hash.") for n in names)
    pre, seen, dicts, draws, saved = {}, [], [], [], []
    step, compute_loss, object_function, run_head = BertAdam.step, t.compute_loss, model.object_function, DIMCHTokenHash._run

    def recording_step(self, closure=None):                                              # the gradients as the optimiser receives them
        pre.clear()
        pre.update({n: p.grad.detach().clone() for n, p in names.items() if p.grad is not None})
        return step(self, closure)

    def recording_loss(*a, **kw):
        loss = compute_loss(*a, **kw)
        seen.append(({k: kw[k].detach().clone() for k in DS.OUTS}, loss.detach()))
        return loss

    def recording_objective(**kw):
        loss, loss_dict = object_function(**kw)
        dicts.append(loss_dict)
        return loss, loss_dict

    def recording_draw(mod):
        draw = heads[mod].draw_keep_mask

        def draw_keep_mask(B, device):
            keep = draw(B, device)
            draws.append((mod, None if keep is None else keep.detach().cpu().clone()))
            return keep
        return draw_keep_mask

    def recording_run(self, tokens, keep, train):
        out = run_head(self, tokens, keep, train)
        which = "img" if self is heads["img"] else "txt" if self is heads["txt"] else None
        B, M, E, H = out[2].shape[0], self.token_layer.weight.shape[0], out[2].shape[2], self.hash_layer[0].weight.shape[0]
        saved.append((which, train, None if keep is None else keep.detach().cpu().numpy().reshape(B, M, H) != 0, _relus_of_saved(out[3], B, M, E, H)))
        return out
    monkeypatch.setattr(BertAdam, "step", recording_step)
    monkeypatch.setattr(DIMCHTokenHash, "_run", recording_run)
    t.compute_loss = recording_loss
    model.object_function = recording_objective
    for mod in DS.MODS:
        heads[mod].draw_keep_mask = recording_draw(mod)
    assert getattr(t, "optimizer", None) is None and t.epochs == DS.STEPS

    port, logged, ids_seen, problems, lines = [], [], [], [], []
    for s in range(DS.STEPS):
        t.train_loader = [cap["raw"][s % 3]]
        torch.manual_seed(DS.MASK_SEED + s)
        t.train_epoch(s)
        assert len(seen) == len(dicts) == s + 1 and t.global_step == s + 1
        port.append(_record(t, names, pre, seen[-1], dicts[-1]))
        logged.append(float(re.search(r"loss: (?:tensor\()?([-+0-9.eE]+|nan|inf)", t.lines[-1]).group(1)))
        ids_seen.append(cap["raw"][s % 3][1].numpy().reshape(DS.B, -1))
        _structure(s, port[-1], cap, r64[s], ids_seen, names, t, problems)

    lines += DS.condition_lines(case, cond)
    # draws and relu decisions
    if [w for w, _ in draws] != ["img", "txt"] * DS.STEPS:
        problems.append(("mask draws", [w for w, _ in draws]))
    if [(w, tr) for w, tr, _, _ in saved] != [("img", True), ("txt", True)] * DS.STEPS:
        problems.append(("head forwards", [(w, tr) for w, tr, _, _ in saved]))
    for i, (mod, keep) in enumerate(draws[:2 * DS.STEPS]):
        s = i // 2
        want = None if replay is None else replay[s][DS.MODS.index(mod)]
        same = (keep is None and want is None) or (keep is not None and want is not None and torch.equal(keep.view(torch.uint8), want))
        lines.append("%s step %d %s mask %s  equal to the seeded replay: %s" % (case, s, mod, "none" if keep is None else "kept %d of %d"
                                                                                % (int(keep.sum()), keep.numel()), same))
        if not same:
            problems.append((s, "the drawn mask is not the seeded replay", mod))
    for i, (mod, _, used, (c_on, a_on)) in enumerate(saved[:2 * DS.STEPS]):
        if mod is None:
            continue
        s = i // 2
        c64, a64 = (z > 0 for z in r64[s]["pre"][mod])
        want_keep = None if replay is None else replay[s][DS.MODS.index(mod)].numpy().reshape(a64.shape) != 0
        if (used is None) != (want_keep is None) or (used is not None and not np.array_equal(used, want_keep)):
            problems.append((s, "the mask the head was handed is not the replay", mod))
            continue
        kept = np.ones_like(a64) if used is None else used
        diff = int((c_on != c64).sum()) + int((a_on != a64)[kept].sum())
        dropped_on = int(a_on[~kept].sum())
        lines.append("%s step %d %s relu decisions that differ from float64: %d of %d  dropped entries not zero: %d"
                     % (case, s, mod, diff, c64.size + int(kept.sum()), dropped_on))
        if diff != 0 or dropped_on != 0:
            problems.append((s, "relu decisions", mod, diff, dropped_on))

    per_port = []
    for s in range(DS.STEPS):
        rec, ref = port[s], r64[s]
        common = dict(ref, **{k: {n: a for n, a in ref[k].items() if n in rec[k]} for k in ("grad", "clipped", "p", "m", "v")})
        errs = DS.errors(rec, common, sd0)
        per_port.append(errs)
        lines.append("%s step %d loss %.8f f64 %.8f logged %.4f  lr %s" % (case, s, rec["loss"], ref["loss"], logged[s], ref["lr"]))
        lines.append("%s step %d terms %s" % (case, s, " ".join("%s %.6f/%.6f" % (n, a, b) for n, a, b in zip(DS.TERMS, rec["terms"], ref["terms"]))))
        if not abs(rec["loss"] - ref["loss"]) <= 5e-5 * abs(ref["loss"]) + 1e-6:
            problems.append((s, "loss", rec["loss"], ref["loss"]))
        if not abs(logged[s] - rec["loss"]) <= 5.1e-5 + 1e-6 * abs(rec["loss"]):         # four printed decimals of an fp32 number
            problems.append((s, "logged loss", logged[s], rec["loss"]))
        if not np.abs(rec["terms"] - ref["terms"]).max() <= 5e-5 * np.abs(ref["terms"]).max() + 1e-6:
            problems.append((s, "terms", rec["terms"].tolist(), ref["terms"].tolist()))
        if rec["terms"][0] != np.float32(rec["loss"]):
            problems.append((s, "loss_dict's loss is not the loss", rec["terms"][0], rec["loss"]))
        for (q, n), e in errs.items():
            key = (q, DS.kind_of(n, q) if n else "")
            if not e <= TOL_FACTOR * e_ref[key]:
                problems.append((s, q, n, "e_port %.2e" % e, "e_ref %.2e" % e_ref[key], "ratio %.2f" % (e / e_ref[key] if e_ref[key] else np.inf)))

    e_port = DS.pool(per_port)
    lines += DS.table(case, e_ref, e_port)
    worst = {}
    for key, e in e_port.items():
        if e_ref.get(key):
            worst[key[0]] = max(worst.get(key[0], 0.0), e / e_ref[key])
    lines.append("%s worst e_port / e_ref per quantity: %s" % (case, " ".join("%s %.2f" % kv for kv in sorted(worst.items()))))
    lines += ["%s problem %s" % (case, (p,)) for p in problems]
    print("\n".join(lines))                                                              # every figure before the first assertion
    if os.environ.get("XMH_DIMCH_TRAIN_STEP_TABLE"):
        with open(os.environ["XMH_DIMCH_TRAIN_STEP_TABLE"], "a") as f:
            f.write("\n".join(lines) + "\n")
    assert not problems, (len(problems), problems[:12])
    assert set(e_port) == set(e_ref)
