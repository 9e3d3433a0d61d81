"""GPU: whole training steps of DNPHTrainer.train_epoch (both CLIP towers, the tanh code with its drawn dropout mask and the 80 class
logits of both modalities, the +-1 noise drawn from model.noise_generator and assigned to the codes at minimal cost, the proxy + noise
objective with noise_alpha as the configuration hands it on, the backward through the objective, the heads and the towers, the fused
BertAdam step over two groups and the proxies' own SGD) against the float64 restatement of tests/dnph_train_step_cases.py: five steps,
each its own train_epoch call on the loader's three batches in turn, on the two cases `plain` (K = 16, one block per tower) and `wide`
(K = 24, two blocks per tower at embed_dim 128).

Recorded with monkeypatches only: BertAdam.step (the gradients as the optimiser receives them), torch.optim.SGD.step (the proxies and
their gradient as the SGD receives them), the trainer's compute_loss (the two codes, the two logit matrices and the loss), the
model's object_function (loss_dict), draw_keep_mask of each code layer (the masks), the model's rand_unit_rect (the drawn matrix) and
xmh.models.dnph.gene_noise (the codes it is handed and the noise rows it assigns).  torch.manual_seed(MASK_SEED + s) before step s; the
loader is a list.  The restatement runs on the CPU before the device's first step, on the seeded replays of the masks and of the noise;
its assignment is its own brute force over the 24 permutations, and nothing is rerun under the port's own decisions.  The conditions on
the inputs are re-asserted on the float64 run before any comparison.

After every step.  Draws: exactly one mask per code layer and step in the order image then text, each equal to the seeded replay of
the same torch.rand(B, K) >= 0.2 calls; exactly one +-1 matrix, equal to the replay of np.random.default_rng(seed).  Assignments:
gene_noise is called twice, with the image codes and then the text codes as compute_loss receives them and the drawn matrix both
times, and what it returns is the float64 brute force's rows -- both the brute force of the float64 restatement's codes and that of
the very codes gene_noise was handed; this is the first independent check of xmh_assign_min_cost inside training.  Loss and log: the
loss compute_loss returned, the epoch's four-decimal log line, the three scalars of loss_dict (All loss, Noise image / text) against the
float64 terms, All loss being the loss.  Head outputs: img_hash, txt_hash, img_pre, txt_pre as compute_loss receives them.  Optimiser
state: p.grad of every parameter as optimizer.step() receives it and as it leaves it (clipped), delta = p - p_initial, next_m /
next_v / step, optimizer.get_lr() in parameter-group order, t_total.  The proxies: their gradient and delta against the float64 run by
the rule below; the SGD holds them alone, at optimizer.loss.lr, without momentum, weight decay or state; one step moves them to
p + fl(-lr) g as float32 arithmetic gives it, to the bit (with or without a fused multiply-add, the same choice for the whole tensor);
they carry no BertAdam state and belong to no BertAdam group.  Exact: logit_scale bit-unchanged, without gradient and without state;
the set of parameters with a gradient; absent token ids and positional rows at or beyond L exact zeros in grad, clipped, m and v; step
0 moving no BertAdam parameter and filling the moments.

Tolerances.  Per tensor e = max|got - f64| / max|f64|.  Per quantity and tensor kind (train_step_cases.kind_of, pooled over steps
and layers; each of the eight head tensors a kind of its own, but their delta pooled per modality, for the reason and with the two
runs' figures that tests/dnph_train_step_cases.py gives; the proxies a kind of their own; the four head outputs under `codes`) the yardstick e_ref
is the float32 restatement against the float64 one on these very inputs, masks and assignments: the port must stay within
TOL_FACTOR = 4 times that, the rule and factor of tests/test_gpu_train_step.py.  The loss and the scalars of loss_dict (relative to the largest term) go by that rule as well,
under `loss` and `terms`, and besides by rtol 5e-5, atol 1e-6 as in the three other trajectory modules.  The null set is empty in both cases (tests/test_dnph_train_step_cpu.py pins it), so no tensor goes by an absolute rule.

Measured on an MI355X (profiles/dnph_train_step_f64.txt), worst e_port / e_ref per quantity (the bound is 4) -- plain: codes 2.19
(img_hash), grad 2.63 (hash.text_pre.fc.bias: 2.2e-7 against 8.2e-8), clipped 2.63, delta 1.68, m 1.79, v 1.91, loss 1.09 (1.5e-7
relative), terms 1.41; wide: codes 1.18, grad 1.34, clipped 1.31, delta 1.63, m 1.56, v 1.88, loss 1.35 (2.7e-7), terms 1.25; the
proxies: grad 2.28 and 0.67, delta 1.00 and 1.00.  Every drawn mask and +-1 matrix equalled its replay, all twenty assignments equalled
the float64 brute force (from the float64 codes and from the port's own), and every SGD step was p + fl(-lr) g to the bit.  The
conditions with the device's masks: the best permutation below the second best by 9.8e-3 (plain) and 2.6e-2 (wide) at least, against
4.3e-6 and 3.0e-6, the largest float32 change of a total (2300 x and 9000 x).  With every head tensor's delta a kind of its own the module
passed too, its largest ratio the delta of hash.text_hash.fc.bias in wide, 3.55 (1.74e-5 against 4.90e-6); pooled per modality that
ratio is 1.19.

The module was seen to fail under each of these edits on a scratch copy of the package (the first failing check of each, then what
else; the loss of step 0 is 14.93382 in plain and 16.05162 in wide).  t_noises assigned from the image codes: "gene_noise was not handed
this modality's codes and the drawn matrix" for the text at step 0 and the text's assignment, then the loss at step 0 (15.15854;
16.38723), its terms and every gradient.  The assignment replaced by the identity: both assignments at step 0 (and at every step),
then the loss at step 0 (15.13634; 16.64845) and every gradient.  noise_alpha taken as 1.0: the loss at step 0 (14.00781; 13.40565),
the scalars of loss_dict and every gradient at step 0; assignments from step 2 (plain) or 3 (wide) on, once the codes have moved
elsewhere.  optimizer_loss.step() removed: "the proxies' SGD did not step" and loss.proxies missing from the parameters with a gradient
as the SGD sees them at step 0, then the loss at step 1 (16.47347 against 16.46441; 15.60934 against 15.60650) and everything after.
The proxies' rate read from optimizer.lr: the SGD's lr 0.002 and "the proxies' step is not p - lr g to the bit" (all 96 / 144 entries)
at step 0, the proxies' delta at step 0, then the loss at step 1 (16.47164; 15.60877).  The cross-entropy target taken as the last set
label instead of the first (a scratch build of the library): the loss at step 0 (15.61887; 15.47920) and every gradient at step 0
(e_port 0.5 to 0.8 on the positional embedding).

Every figure is printed before the first assertion; with XMH_DNPH_TRAIN_STEP_TABLE naming a file the table is appended to it
(profiles/dnph_train_step_f64.txt was written so)."""
import os
import re

import numpy as np
import pytest
import torch

import dnph_train_step_cases as NS

pytestmark = pytest.mark.gpu

TOL_FACTOR = NS.TOL_FACTOR
TOK, POS = "backbone.token_embedding.weight", "backbone.positional_embedding"
PLACES = [0, 4, 5]                                                                       # loss_dict's scalars among dnph_cases.TERMS


def _np(t):
    return t.detach().cpu().numpy()


def _record(t, names, pre, seen, loss_dict, sgd_seen):
    """the trainer's state after a step in the layout of a restatement record"""
    outs, loss = seen
    rec = {k: {} for k in ("grad", "clipped", "p", "m", "v")}
    rec["loss"], rec["step"], rec["buffers"] = float(loss), {}, {}
    for n, p in names.items():
        if n == NS.PROXIES:
            continue
        st = t.optimizer.state[p]
        rec["step"][n] = st.get("step")
        if p.grad is None:
            continue
        rec["grad"][n], rec["clipped"][n], rec["p"][n] = _np(pre[n]), _np(p.grad), _np(p)
        rec["m"][n], rec["v"][n] = _np(st["next_m"]), _np(st["next_v"])
    if sgd_seen is not None:
        rec["grad"][NS.PROXIES], rec["p"][NS.PROXIES] = sgd_seen[1], _np(names[NS.PROXIES])
    d = loss_dict
    rec["terms"] = np.full(len(NS.TERMS), np.nan)                                        # loss_dict holds three of the six terms
    rec["terms"][PLACES] = [float(x) for x in (d["All loss"], d["Noise"]["image"], d["Noise"]["text"])]
    rec["outs"] = [_np(outs[k]) for k in NS.OUTS]
    return rec


def _structure(s, rec, cap, ref, ids_seen, names, t, sgd_seen, problems):
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
    want = [ref["next_lr"][NS.group_of(n)] for n in order if n is not None and n != NS.PROXIES]
    got = t.optimizer.get_lr()
    bad(len(got) != len(want) or not np.allclose(got, want, rtol=1e-15, atol=0), "get_lr", sorted(set(got)), sorted(set(want)))
    bad({g["t_total"] for g in t.optimizer.param_groups} != {NS.STEPS}, "t_total")
    bad(sorted(by_id.get(id(q), "?") for q in in_opt) != sorted(n for n in names if n != NS.PROXIES), "the optimiser's parameters")
    # the proxies: the SGD's alone, and nothing of BertAdam's
    prox, sgd = names[NS.PROXIES], t.optimizer_loss
    bad(any(q is prox for q in in_opt) or len(t.optimizer.state.get(prox, {})) != 0, "the proxies are BertAdam's")
    g = sgd.param_groups[0] if isinstance(sgd, torch.optim.SGD) and len(sgd.param_groups) == 1 else {}
    bad([id(q) for q in g.get("params", [])] != [id(prox)] or g.get("lr") != NS.PROXY_LR or g.get("momentum") != 0 or g.get("weight_decay") != 0
        or g.get("nesterov") or g.get("maximize") or len(sgd.state.get(prox, {}) if g else {}) != 0, "the proxies' SGD", {k: v for k, v in g.items() if k != "params"})
    if sgd_seen is None:
        bad(True, "the proxies' SGD did not step")
    else:
        before, grad = sgd_seen
        after, alpha = _np(prox), np.float32(-NS.PROXY_LR)
        fused = (before.astype(np.float64) + np.float64(alpha) * grad.astype(np.float64)).astype(np.float32)
        plain = before + alpha * grad
        bad(not (np.array_equal(after, fused) or np.array_equal(after, plain)), "the proxies' step is not p - lr g to the bit",
            int((after != fused).sum()), int((after != plain).sum()))
        bad(not np.array_equal(grad, _np(prox.grad)) or not grad.any(), "the SGD changed the proxies' gradient, or it is zero")
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


@pytest.mark.parametrize("case", list(NS.CASES))
def test_five_dnph_training_steps_follow_the_float64_trajectory(case, tmp_path, monkeypatch):
    from xmh.models import dnph as D
    from xmh.optim import BertAdam
    t = NS.trainer(case, tmp_path, 0)
    cap = NS.capture(t, case)
    sd0 = cap["sd0"]
    model = t.model
    replay = NS.draw_masks(cap, device=model.loss.proxies.device)
    noises = NS.draw_noises(cap)
    r64 = NS.run(cap, replay, noises)
    r32 = NS.run(cap, replay, noises, dtype=torch.float32)
    cond = NS.check_conditions(r64, r32)                                                 # before any comparison
    assert NS.null_set(r64) == ()
    _, e_ref, _ = NS.yardstick(cap, r64, r32, places=PLACES)                             # both runs took the same assignments: just asserted

    names = dict(model.named_parameters())
    heads = {"img": model.hash.image_hash, "txt": model.hash.text_hash}
    assert sorted(n for n in names if not (n.startswith("backbone.") or n.startswith("hash."))) == [NS.PROXIES]
    pre, seen, dicts, draws, drawn, assigned, sgd_seen = {}, [], [], [], [], [], []
    step, sgd_step, compute_loss, object_function = BertAdam.step, torch.optim.SGD.step, t.compute_loss, model.object_function
    rand_unit_rect, gene_noise = model.rand_unit_rect, D.gene_noise

    def recording_step(self, closure=None):                                              # the gradients as the optimiser receives them
        pre.clear()
        pre.update({n: p.grad.detach().clone() for n, p in names.items() if p.grad is not None})
        return step(self, closure)

    def recording_sgd(self, *a, **kw):
        prox = names[NS.PROXIES]
        sgd_seen.append((_np(prox).copy(), None if prox.grad is None else _np(prox.grad).copy()))
        return sgd_step(self, *a, **kw)

    def recording_loss(*a, **kw):
        loss = compute_loss(*a, **kw)
        seen.append(({k: kw[k].detach().clone() for k in NS.OUTS}, loss.detach()))
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

    def recording_rect(npoints, ndim):
        out = rand_unit_rect(npoints, ndim)
        drawn.append(np.array(out).copy())
        return out

    def recording_gene(embeddings, noises_):
        out = gene_noise(embeddings, noises_)
        assigned.append((np.array(embeddings).copy(), np.array(noises_).copy(), np.array(out).copy()))
        return out
    monkeypatch.setattr(BertAdam, "step", recording_step)
    monkeypatch.setattr(torch.optim.SGD, "step", recording_sgd)
    monkeypatch.setattr(D, "gene_noise", recording_gene)
    t.compute_loss = recording_loss
    model.object_function = recording_objective
    model.rand_unit_rect = recording_rect
    for mod in NS.MODS:
        heads[mod].draw_keep_mask = recording_draw(mod)
    assert getattr(t, "optimizer", None) is None and t.epochs == NS.STEPS

    port, logged, ids_seen, problems, lines = [], [], [], [], []
    for s in range(NS.STEPS):
        t.train_loader = [cap["raw"][s % 3]]
        torch.manual_seed(NS.MASK_SEED + s)
        t.train_epoch(s)
        assert len(seen) == len(dicts) == s + 1 and t.global_step == s + 1
        mine = sgd_seen[s] if len(sgd_seen) == s + 1 and sgd_seen[s][1] is not None else None
        port.append(_record(t, names, pre, seen[-1], dicts[-1], mine))
        logged.append(float(re.search(r"loss: (?:tensor\()?([-+0-9.eE]+|nan|inf)", t.lines[-1]).group(1)))
        ids_seen.append(cap["raw"][s % 3][1].numpy().reshape(NS.B, -1))
        _structure(s, port[-1], cap, r64[s], ids_seen, names, t, mine, problems)

    lines += NS.condition_lines(case, cond)
    # draws and assignments
    if [w for w, _ in draws] != ["img", "txt"] * NS.STEPS:
        problems.append(("mask draws", [w for w, _ in draws]))
    if len(drawn) != NS.STEPS or len(assigned) != 2 * NS.STEPS or len(sgd_seen) != NS.STEPS:
        problems.append(("noise draws", len(drawn), "gene_noise calls", len(assigned), "SGD steps", len(sgd_seen)))
    for i, (mod, keep) in enumerate(draws[:2 * NS.STEPS]):
        s, want = i // 2, replay[i // 2][NS.MODS.index(mod)]
        same = keep is not None and torch.equal(keep.view(torch.uint8), want)
        lines.append("%s step %d %s mask kept %s of %d  equal to the seeded replay: %s" % (case, s, mod, None if keep is None else int(keep.sum()), want.numel(), same))
        if not same:
            problems.append((s, "the drawn mask is not the seeded replay", mod))
    for s, got in enumerate(drawn[:NS.STEPS]):
        same = got.shape == noises[s].shape and np.array_equal(got, noises[s])
        lines.append("%s step %d drawn +-1 matrix equal to the replay of default_rng(%d): %s" % (case, s, NS.MODEL_SEED, same))
        if not same:
            problems.append((s, "the drawn noise is not the seeded replay"))
    for i, (codes, vectors, out) in enumerate(assigned[:2 * NS.STEPS]):
        s, mod = i // 2, NS.MODS[i % 2]
        fed = np.array_equal(codes, port[s]["outs"][i % 2]) and np.array_equal(vectors, noises[s])
        own, _ = NS.brute_force(codes, noises[s])
        want = r64[s]["perm"][mod]
        ok = out.shape == noises[s].shape and np.array_equal(out, noises[s][NS.PERMS[want]].astype(out.dtype))
        lines.append("%s step %d %s assignment: handed compute_loss's %s codes and the drawn matrix: %s  float64 brute force %s  brute force of the port's "
                     "codes %s  the port's rows equal the float64 brute force's: %s" % (case, s, mod, mod, fed, NS.PERMS[want].tolist(), NS.PERMS[own].tolist(), ok))
        if not fed:
            problems.append((s, "gene_noise was not handed this modality's codes and the drawn matrix", mod))
        if not ok or own != want:
            problems.append((s, "assignment", mod, NS.PERMS[want].tolist(), NS.PERMS[own].tolist()))

    per_port = []
    for s in range(NS.STEPS):
        rec, ref = port[s], r64[s]
        common = dict(ref, **{k: {n: a for n, a in ref[k].items() if n in rec[k]} for k in ("grad", "clipped", "p", "m", "v")})
        errs = NS.errors(rec, common, sd0, places=PLACES)
        per_port.append(errs)
        lines.append("%s step %d loss %.8f f64 %.8f logged %.4f  lr %s" % (case, s, rec["loss"], ref["loss"], logged[s], ref["lr"]))
        lines.append("%s step %d terms %s" % (case, s, " ".join("%s %.6f/%.6f" % (NS.TERMS[j], rec["terms"][j], ref["terms"][j]) for j in PLACES)))
        if not abs(rec["loss"] - ref["loss"]) <= 5e-5 * abs(ref["loss"]) + 1e-6:
            problems.append((s, "loss", rec["loss"], ref["loss"]))
        if not abs(logged[s] - rec["loss"]) <= 5.1e-5 + 1e-6 * abs(rec["loss"]):         # four printed decimals of an fp32 number
            problems.append((s, "logged loss", logged[s], rec["loss"]))
        if not np.abs(rec["terms"] - ref["terms"])[PLACES].max() <= 5e-5 * np.abs(ref["terms"][PLACES]).max() + 1e-6:
            problems.append((s, "terms", rec["terms"].tolist(), ref["terms"].tolist()))
        if rec["terms"][0] != np.float32(rec["loss"]):
            problems.append((s, "loss_dict's loss is not the loss", rec["terms"][0], rec["loss"]))
        for (q, n), e in errs.items():
            key = (q, NS.kind_of(n, q) if n else "")
            if not e <= TOL_FACTOR * e_ref[key]:
                problems.append((s, q, n, "e_port %.2e" % e, "e_ref %.2e" % e_ref[key], "ratio %.2f" % (e / e_ref[key] if e_ref[key] else np.inf)))

    e_port = NS.pool(per_port)
    lines += NS.table(case, e_ref, e_port)
    worst = {}
    for key, e in e_port.items():
        if e_ref.get(key):
            worst[key[0]] = max(worst.get(key[0], 0.0), e / e_ref[key])
    lines.append("%s worst e_port / e_ref per quantity: %s" % (case, " ".join("%s %.2f" % kv for kv in sorted(worst.items()))))
    lines += ["%s problem %s" % (case, (p,)) for p in problems]
    print("\n".join(lines))                                                              # every figure before the first assertion
    if os.environ.get("XMH_DNPH_TRAIN_STEP_TABLE"):
        with open(os.environ["XMH_DNPH_TRAIN_STEP_TABLE"], "a") as f:
            f.write("\n".join(lines) + "\n")
    assert not problems, (len(problems), problems[:12])
    assert set(e_port) == set(e_ref)
