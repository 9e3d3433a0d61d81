"""GPU: whole training steps of TwDHTrainer.train_epoch_codes (both CLIP towers forward, the DCMHT hash layer at long_dim bits, the
short codes of both modalities through the transforms, the tie draw, the hash-centre targets, the objective, the backward through the
objective, the transforms, the heads, the towers and their blocks, the fused BertAdam step over two groups) against the float64
restatement of tests/twdh_train_step_cases.py: five steps, each its own train_epoch_codes call on the loader's two batches in turn,
on the two cases `rated` (low_rate 0.3: the long code's gradient arrives both ways) and `shipped` (low_rate 0: the short gradient is
skipped).

Recorded with monkeypatches only: BertAdam.step (the gradients as the optimiser receives them), the trainer's compute_loss (the four
codes and the loss), the model's object_function (loss_dict), the model's draw_ties and hash_targets (the ties and the packed target
words) and DCMHTModalityHash._train_forward (the relu output f it stores, at the place include/xmh.h gives, for the relu decisions).
torch.manual_seed(TIE_SEED + s) before step s; the loader is a list, so nothing else draws from the CPU's generator.  The
restatement runs on the CPU, from what was captured before the device's first step.  The conditions on the inputs are re-asserted on
the float64 run before any comparison.

After every step.  Ties and targets: exactly one draw, the drawn ties equal to the seeded replay, the packed targets equal to
twdh_cases.pack_bits(targets(...)) bit for bit.  Loss and log: the loss compute_loss returned, the epoch's four-decimal log line,
every scalar of loss_dict (All loss, Long NCE / Quan for image and text, Short NCE / Quan per key in key order) against the float64
terms, All loss being the loss.  Codes: the four code matrices as compute_loss receives them.  Optimiser state: p.grad of every
parameter as optimizer.step() receives it and as it leaves it (clipped), delta = p - p_initial, next_m / next_v / step of every
parameter, BatchNorm's running statistics and batch count, optimizer.get_lr() in parameter-group order, t_total.  Exact: logit_scale
bit-unchanged, without gradient and without state; the transforms and centres bit-equal to their initial copies, no parameters and
not in the optimiser; the set of parameters with a gradient; absent token ids, positional rows at or beyond L and the q / k thirds
of in_proj exact zeros in grad, clipped, m and v; step 0 moving nothing and filling the moments.  Relu: a decision of the port that
differs from the float64 run's is a problem (the conditions keep every pre-activation at least 90 tie bounds from zero); nothing is
rerun under the port's mask.

Tolerances.  Per tensor e = max|got - f64| / max|f64|.  Per quantity and tensor kind (train_step_cases.kind_of, pooled over steps
and layers; the four code matrices under `codes`, the running statistics under `buffer`) the yardstick e_ref is the float32
restatement against the float64 one on these very inputs and ties: the port must stay within TOL_FACTOR = 4 times that, the rule and
factor of tests/test_gpu_train_step.py.  The loss: rtol 5e-5, atol 1e-6, the scalars of loss_dict by the same rule relative to the
largest term; the log line prints four decimals.  Null-set tensors (the three biases in front of the image head's BatchNorm) by the
absolute rules of tests/test_gpu_train_step.py: max|g| within NULL_FACTOR = 32 times the float32 restatement's at that step,
|m| <= max|g| and v <= max g^2 over the steps so far, delta within sum_s lr_s max_{j<=s} max|g_port,j| / e of the float64 delta,
plus 2^-24 max|p| per step that moves the parameter, the rounding of the float32 parameter as it is stored
(twdh_train_step_cases.null_delta_budget, argued in that module's docstring from the two restatements alone).

Measured on an MI355X (profiles/twdh_train_step_f64.txt), worst e_port / e_ref per quantity (the bound is 4) -- rated: codes 1.09,
grad 1.67, clipped 1.67, delta 1.25, m 1.37, v 2.16 (the text blocks' out_proj.weight), buffer 1.00, loss 0.72 (6.3e-8 relative),
terms 0.75; shipped: codes 1.46 (img_long), grad 1.73, clipped 1.73, delta 1.24, m 1.83, v 1.99 (the image blocks' ln_2.weight), buffer
0.93, loss 0.96 (7.1e-8), terms 1.23.  Every drawn tie vector equalled the replay, no packed target word and no relu decision
differed.  As first written, with the null deltas by the rule of tests/test_gpu_train_step.py alone, rated missed at one place:
|delta - f64| of backbone.visual.ln_post.bias, 1.793e-9 at step 1 against a budget of 1.47e-9 (3.81e-9 against 3.26e-9 at step 4);
the measure was at fault, not the port -- the float32 restatement's own figure is the same 1.793e-9, the rounding of the stored
parameter, which its noise does not explain either (twdh_train_step_cases) -- and with the storage term the budget is 4.8e-9.

The module was seen to fail under each of these edits on a scratch copy of the package (case rated; the first failing check of
each, then what else).  The text's short codes handed in as the image's in the step: codes img_short at step 0 (e_port 0.25, ratio
3e5), the loss at step 0 (2.23467 against 2.23583) and its terms, every gradient at step 0.  _ShortCodes.backward returning zeros
for the long code: grad of every tensor at step 0 (ratios 4e3 to 1.5e6, e_port 0.2 to 0.3), loss and codes of step 0 untouched.  The
short streams' quantisation weight taken as quan_alpha instead of low_rate in k_twdh_loss_grad: grad of every tensor at step 0
(ratios 9e2 to 9.5e5, e_port 0.04 to 0.09).  n taken as B 2 K_tot instead of B 2 K[s] in k_twdh_loss_grad: grad of every tensor at
step 0 (ratios 1.7e4 to 3e6, e_port 0.4 to 0.5).  A zero sum taking bit 0 instead of tie[k] in k_twdh_targets: the packed targets at
steps 0, 2 and 4 (2 words of 8), the loss at step 0 (2.23251 against 2.23583); steps 1 and 3, without ties, start from moved
parameters only.  The short centres drawn before the long one in draw_ties: the drawn ties at every step, the packed targets at
steps 0, 2 and 4, the loss at step 0 (2.21292).  The backbone group given `lr`: get_lr after steps 0 to 3 (after step 4 both rates
are 0), delta of every backbone tensor at step 1 (e_port 3.0: four times the step).  optimizer.zero_grad() removed from
_train_epoch: absent token ids in grad and clipped at step 1, every gradient from step 1 on.  From step 2 on each of them also
flips relu decisions of both heads, which the module reports.

Every figure is printed before the first assertion; with XMH_TWDH_TRAIN_STEP_TABLE naming a file the table is appended to it
(profiles/twdh_train_step_f64.txt was written so)."""
import os
import re

import numpy as np
import pytest
import torch

import twdh_cases as TC
import twdh_train_step_cases as WS

pytestmark = pytest.mark.gpu

TOL_FACTOR = WS.TOL_FACTOR
NULL_FACTOR = 32.0
TOK, POS = "backbone.token_embedding.weight", "backbone.positional_embedding"


def _np(t):
    return t.detach().cpu().numpy()


def _relu_of_saved(saved, B, E, N):
    """f > 0 [B, N] from the saved buffer of xmh_head_dcmht_train_forward (include/xmh.h: v, nhat, n [B, E], rstd [max(B, E)], f [B, N],
    every section rounded up to 256 bytes)"""
    a256 = lambda v: (v + 255) & ~255                                                    # noqa: E731
    off = 3 * a256(B * E * 4) + a256(max(B, E) * 4)
    return saved[off:off + B * N * 4].clone().view(torch.float32).reshape(B, N).cpu().numpy() > 0


def _record(t, cap, names, pre, seen, loss_dict):
    """the trainer's state after a step in the layout of a restatement record"""
    codes, loss = seen
    rec = {k: {} for k in ("grad", "clipped", "p", "m", "v")}
    rec["loss"], rec["step"] = float(loss), {}
    for n, p in names.items():
        st = t.optimizer.state[p]
        rec["step"][n] = st.get("step")
        if p.grad is None:
            continue
        rec["grad"][n], rec["clipped"][n], rec["p"][n] = _np(pre[n]), _np(p.grad), _np(p)
        rec["m"][n], rec["v"][n] = _np(st["next_m"]), _np(st["next_v"])
    rec["buffers"] = {k: (_np(v) if v.is_floating_point() else int(v)) for k, v in t.model.state_dict().items() if WS.is_buffer(k)}
    d, keys = loss_dict, cap["keys"]
    terms = [d["All loss"], d["Long"]["NCE"]["image"], d["Long"]["NCE"]["text"], d["Long"]["Quan"]["image"], d["Long"]["Quan"]["text"]]
    for k in keys:
        terms += [d["Short"][k]["NCE"], d["Short"][k]["Quan"]]
    rec["terms"] = np.array([float(x) for x in terms])
    rec["short_keys"] = (list(d["Short"]), list(codes["short_img_hash"]), list(codes["short_txt_hash"]))
    rec["probs"] = {"img_long": _np(codes["long_img_hash"]), "txt_long": _np(codes["long_txt_hash"]),
                    "img_short": _np(torch.cat([codes["short_img_hash"][k] for k in keys], 1)),
                    "txt_short": _np(torch.cat([codes["short_txt_hash"][k] for k in keys], 1))}
    return rec


def _structure(s, rec, cap, ref, ids_seen, names, t, problems):
    """the exact zeros and bit equalities of the CPU module's structure list, on the device"""
    def bad(cond, *what):
        if cond:
            problems.append((s,) + what)
    sd0, model = cap["sd0"], t.model
    p = names["backbone.logit_scale"]
    bad(not torch.equal(p.detach().cpu(), sd0["backbone.logit_scale"]) or p.grad is not None or len(t.optimizer.state[p]) != 0, "logit_scale")
    bad(sorted(rec["grad"]) != sorted(ref["grad"]), "the parameters with a gradient", sorted(set(rec["grad"]) ^ set(ref["grad"])))
    bad(any(v != s + 1 for n, v in rec["step"].items() if n != "backbone.logit_scale"), "step counters")
    by_id = {id(q): n for n, q in names.items()}
    in_opt = [q for g in t.optimizer.param_groups for q in g["params"]]
    order = [by_id.get(id(q)) for q in in_opt if q.grad is not None]
    want = [ref["next_lr"][WS.group_of(n)] for n in order if n is not None]
    got = t.optimizer.get_lr()
    bad(len(got) != len(want) or not np.allclose(got, want, rtol=1e-15, atol=0), "get_lr")
    bad({g["t_total"] for g in t.optimizer.param_groups} != {WS.STEPS}, "t_total")
    # the constants: bit-equal, no parameters, not in the optimiser
    bad(sorted(by_id.get(id(q), "?") for q in in_opt) != sorted(names), "the optimiser's parameters")
    bad(list(model.trans) != cap["keys"] or list(model.short_center) != cap["keys"], "the constants' keys")
    consts = [(model.long_center, cap["long_center"])] + [(model.trans[k], cap["trans"][k]) for k in cap["keys"] if k in model.trans] \
        + [(model.short_center[k], cap["short_center"][k]) for k in cap["keys"] if k in model.short_center]
    for now, then in consts:
        bad(not torch.equal(now.detach().cpu(), then) or now.requires_grad or isinstance(now, torch.nn.Parameter) or id(now) in by_id
            or any(now is q for q in in_opt), "a transform or centre changed, or is trained")
    ids = ids_seen[-1]
    vocab = sd0[TOK].shape[0]
    for kind in ("grad", "clipped", "m", "v"):
        if TOK not in rec[kind] or POS not in rec[kind]:
            continue                                                                     # reported above, with the parameters with a gradient
        seen = np.unique(ids if kind in ("grad", "clipped") else np.concatenate(ids_seen))
        absent = np.setdiff1d(np.arange(vocab), seen)
        bad(rec[kind][TOK][absent].any(), kind, "absent token ids")
        bad(rec[kind][POS][ids.shape[1]:].any(), kind, "positional rows >= L")
        for mod in WS.MODS:
            e = sd0["hash.%s_hash.norm.weight" % mod].shape[0]
            for k in ("in_proj_weight", "in_proj_bias"):
                n = "hash.%s_hash.atten.%s" % (mod, k)
                bad(n in rec[kind] and rec[kind][n][:2 * e].any(), kind, mod, k, "q / k thirds")
    if s == 0:                                                                           # rate 0: nothing moves, the moments are filled
        for n in rec["m"]:
            bad(not np.array_equal(rec["p"][n], sd0[n].numpy()), "step 0 moved", n)
            bad(not rec["m"][n].any() or not rec["v"][n].any(), "step 0 left the moments empty", n)
    bad(rec["buffers"]["hash.img_hash.norm.num_batches_tracked"] != s + 1, "num_batches_tracked")


@pytest.mark.parametrize("case", list(WS.CASES))
def test_five_twdh_training_steps_follow_the_float64_trajectory(case, tmp_path, monkeypatch):
    from xmh.models.heads import DCMHTModalityHash
    from xmh.optim import BertAdam
    t = WS.trainer(case, tmp_path, 0)
    cap = WS.capture(t, case)
    sd0, lens, keys = cap["sd0"], cap["lens"], cap["keys"]
    r64 = WS.run(cap)
    r32 = WS.run(cap, dtype=torch.float32)
    cond = WS.check_conditions(r64, WS.bits_of(r32))                                     # before any comparison
    null = WS.null_set(r64)
    assert null == WS.NULL_TWDH
    _, e_ref, noise32 = WS.yardstick(cap, r64, r32, null)
    places = WS.loss_dict_places(len(lens))
    term_names = WS.loss_dict_names(keys)

    model = t.model
    names = dict(model.named_parameters())
    assert all(n.startswith("backbone.") or n.startswith("hash.") for n in names)
    pre, seen, dicts, draws, packed, relus = {}, [], [], [], [], []
    step, compute_loss, object_function = BertAdam.step, t.compute_loss, model.object_function
    draw_ties, hash_targets, train_forward = model.draw_ties, model.hash_targets, DCMHTModalityHash._train_forward

    def recording_step(self, closure=None):                                              # the gradients as the optimiser receives them
        pre.clear()
        pre.update({n: p.grad.detach().clone() for n, p in names.items() if p.grad is not None})
        return step(self, closure)

    def recording_loss(**kw):
        loss = compute_loss(**kw)
        codes = {k: (kw[k].detach().clone() if torch.is_tensor(kw[k]) else {n: x.detach().clone() for n, x in kw[k].items()})
                 for k in ("long_img_hash", "long_txt_hash", "short_img_hash", "short_txt_hash")}
        seen.append((codes, loss.detach()))
        return loss

    def recording_objective(**kw):
        loss, loss_dict = object_function(**kw)
        dicts.append(loss_dict)
        return loss, loss_dict

    def recording_draw():
        ties = draw_ties()
        draws.append({k: v.detach().cpu().clone() for k, v in ties.items()})
        return ties

    def recording_targets(labels, device, ties=None):
        out = hash_targets(labels, device, ties)
        packed.append(_np(out).copy())
        return out

    def recording_forward(self, data):
        probs, x, saved = train_forward(self, data)
        which = "img" if self is model.hash.img_hash else "txt" if self is model.hash.txt_hash else None
        relus.append((which, _relu_of_saved(saved, x.shape[0], x.shape[1], probs.shape[1])))
        return probs, x, saved
    monkeypatch.setattr(BertAdam, "step", recording_step)
    monkeypatch.setattr(DCMHTModalityHash, "_train_forward", recording_forward)
    t.compute_loss = recording_loss
    model.object_function = recording_objective
    model.draw_ties = recording_draw
    model.hash_targets = recording_targets
    assert getattr(t, "optimizer", None) is None and t.epochs == WS.STEPS

    port, logged, ids_seen, problems, lines = [], [], [], [], []
    for s in range(WS.STEPS):
        t.train_loader = [cap["raw"][s % 2]]
        torch.manual_seed(WS.TIE_SEED + s)
        t.train_epoch_codes(s)
        assert len(seen) == len(dicts) == s + 1 and t.global_step == s + 1
        if (len(draws), len(packed)) != (s + 1, s + 1):
            problems.append((s, "draws so far", len(draws), "hash_targets calls so far", len(packed)))
        port.append(_record(t, cap, names, pre, seen[-1], dicts[-1]))
        logged.append(float(re.search(r"loss: (?:tensor\()?([-+0-9.eE]+|nan|inf)", t.lines[-1]).group(1)))
        ids_seen.append(cap["raw"][s % 2][1].numpy().reshape(WS.B, -1))
        _structure(s, port[-1], cap, r64[s], ids_seen, names, t, problems)

    lines += WS.condition_lines(case, cond)
    # ties, targets, relu decisions
    if len(draws) != WS.STEPS or len(packed) != WS.STEPS:
        problems.append(("draws", len(draws), "hash_targets calls", len(packed)))
    if [w for w, _ in relus] != ["img", "txt"] * WS.STEPS:
        problems.append(("head forwards", [w for w, _ in relus]))
    for s in range(min(WS.STEPS, len(draws), len(packed))):
        ref, replay = r64[s], WS.replay_ties(cap, s)
        same = list(draws[s]) == list(replay) and all(torch.equal(draws[s][k], replay[k]) for k in replay)
        want = TC.pack_bits(TC.targets(cap["batches"][s % 2][2], WS.centres_of(cap), WS.ties_list(cap, replay)))
        got = packed[s].view(np.uint32) if packed[s].dtype == np.int32 else packed[s]
        wrong = int((got != want).sum()) if got.shape == want.shape else -1
        lines.append("%s step %d ties equal the seeded replay: %s  packed target words that differ: %d of %d" % (case, s, same, wrong, want.size))
        if not same:
            problems.append((s, "the drawn ties are not the seeded replay"))
        if wrong != 0 or not np.array_equal(want, TC.pack_bits(ref["bits"])):
            problems.append((s, "packed targets", wrong))
    for i, (which, mask) in enumerate(relus[:2 * WS.STEPS]):
        if which is None:
            continue
        want = r64[i // 2]["masks"][which]
        diff = int((mask != want).sum()) if mask.shape == want.shape else -1
        lines.append("%s step %d %s relu decisions that differ from float64: %d of %d" % (case, i // 2, which, diff, want.size))
        if diff != 0:
            problems.append((i // 2, "relu decisions", which, diff))

    per_port = []
    null_g = {n: [] for n in null}
    for s in range(WS.STEPS):
        rec, ref = port[s], r64[s]
        common = dict(ref, **{k: {n: a for n, a in ref[k].items() if n in rec[k]} for k in ("grad", "clipped", "p", "m", "v")})
        errs = WS.errors(rec, common, sd0, null, places)
        per_port.append(errs)
        want_terms = ref["terms"][places]
        lines.append("%s step %d loss %.8f f64 %.8f logged %.4f  lr %s" % (case, s, rec["loss"], ref["loss"], logged[s], ref["lr"]))
        lines.append("%s step %d terms %s" % (case, s, " ".join("%s %.6f/%.6f" % (n, a, b) for n, a, b in zip(term_names, rec["terms"], want_terms))))
        if not abs(rec["loss"] - ref["loss"]) <= 5e-5 * abs(ref["loss"]) + 1e-6:
            problems.append((s, "loss", rec["loss"], ref["loss"]))
        if not abs(logged[s] - rec["loss"]) <= 5.1e-5 + 1e-6 * abs(rec["loss"]):         # four printed decimals of an fp32 number
            problems.append((s, "logged loss", logged[s], rec["loss"]))
        if not np.abs(rec["terms"] - want_terms).max() <= 5e-5 * np.abs(want_terms).max() + 1e-6:
            problems.append((s, "terms", rec["terms"].tolist(), want_terms.tolist()))
        if rec["terms"][0] != np.float32(rec["loss"]):
            problems.append((s, "loss_dict's loss is not the loss", rec["terms"][0], rec["loss"]))
        if rec["short_keys"] != (keys, keys, keys):
            problems.append((s, "the short codes' keys", rec["short_keys"]))
        for (q, n), e in errs.items():
            key = (q, WS.kind_of(n) if n else "")
            if q not in ("loss", "terms") and not e <= TOL_FACTOR * e_ref[key]:
                problems.append((s, q, n, "e_port %.2e" % e, "e_ref %.2e" % e_ref[key], "ratio %.2f" % (e / e_ref[key] if e_ref[key] else np.inf)))
        for n in null:                                                                   # the null set: absolute bounds
            if n not in rec["grad"]:
                continue
            g = float(np.abs(rec["grad"][n]).max())
            null_g[n].append(g)
            budget = WS.null_delta_budget([r64[j]["lr"][WS.group_of(n)] for j in range(s + 1)], null_g[n], float(np.abs(rec["p"][n]).max()))
            d = float(np.abs(WS.quantity(rec, "delta", n, sd0) - WS.quantity(ref, "delta", n, sd0)).max())
            lines.append("%s step %d null %-40s max|g| port %.2e  f32 %.2e  f64 %.2e   |delta - f64| %.2e  bound %.2e"
                         % (case, s, n, g, noise32[s][n], float(np.abs(ref["grad"][n]).max()), d, budget))
            if not g <= NULL_FACTOR * noise32[s][n]:
                problems.append((s, "null gradient", n, g, noise32[s][n]))
            if not d <= budget:
                problems.append((s, "null delta", n, d, budget))
            if float(np.abs(rec["m"][n]).max()) > max(null_g[n]) or float(rec["v"][n].max()) > max(null_g[n]) ** 2:
                problems.append((s, "null moments", n))

    e_port = WS.pool(per_port)
    lines += WS.table(case, e_ref, e_port)
    worst = {}
    for key, e in e_port.items():
        if e_ref.get(key):
            worst[key[0]] = max(worst.get(key[0], 0.0), e / e_ref[key])
    lines.append("%s worst e_port / e_ref per quantity: %s" % (case, " ".join("%s %.2f" % kv for kv in sorted(worst.items()))))
    lines += ["%s problem %s" % (case, (p,)) for p in problems]
    print("\n".join(lines))                                                              # every figure before the first assertion
    if os.environ.get("XMH_TWDH_TRAIN_STEP_TABLE"):
        with open(os.environ["XMH_TWDH_TRAIN_STEP_TABLE"], "a") as f:
            f.write("\n".join(lines) + "\n")
    assert not problems, (len(problems), problems[:12])
    assert set(e_port) == set(e_ref)
