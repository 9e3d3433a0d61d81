"""GPU: whole training steps of DCMHTTrainer and DSPHTrainer (train_epoch: both CLIP towers forward, the hash heads, the loss, the
backward through heads, towers and blocks, the fused BertAdam step over two groups, DSPH's SGD over the proxies) against the float64
restatement of tests/train_step_cases.py, five steps, each its own train_epoch call on the loader's two batches in turn.

After every step: the loss compute_loss returned (and the epoch's log line), p.grad of every parameter as optimizer.step() receives
it and as it leaves it (clipped), delta = p - p_initial, next_m / next_v / step of every parameter, optimizer.get_lr(), BatchNorm's
running statistics and batch count (DCMHT), the proxies, their gradient and momentum buffer (DSPH), logit_scale bit-unchanged and
stateless, and every exact zero of tests/test_train_step_cpu.py's structure list.  The conditions on the inputs are re-asserted on
the float64 run made with the masks the device draws (DSPH), before any comparison.

Tolerances.  Per tensor e = max|got - f64| / max|f64|.  Per quantity and tensor kind (tower_grad_cases.kind_of for tower tensors,
pooled over the layers; the parameter's name for heads and proxies) the yardstick e_ref is the float32 restatement against the float64
one on these very inputs, pooled over the steps: the port must stay within TOL_FACTOR = 4 times that, the rule and factor of
tests/test_gpu_tower_grad.py / test_gpu_block_grad.py.  The float32 run stores its parameters in fp32, so delta's yardstick holds the
once-per-step rounding of the stored parameter.  The loss: rtol 5e-5, atol 1e-6 (tests/test_gpu_bertadam.py's figure for a drifting
trajectory); the log line prints four decimals of it.  Null-set tensors (gradient identically zero, rounding noise only): max|g| within
NULL_FACTOR = 32 times the float32 restatement's max|g| of that tensor at that step (noise of another summation order has no tighter
relation to it; a real gradient there would be its sibling's size, five orders more), |m| <= max|g| and v <= max g^2 over the steps
so far, and delta within sum_s lr_s max_{j<=s} max|g_port,j| / e of the float64 delta, which is what BertAdam can make of that noise
(|m| <= max|g|, |u| <= |m| / e).

Measured on an MI355X: the worst e_port / e_ref is 3.15 (delta of the image tower's class_embedding, DCMHT), every other kind stays
below 3.  The module was seen to fail under each of these edits on a scratch copy of the package: the backbone group given `lr` instead of
`backbone_lr` (get_lr, delta); the upstream gradient doubled before the image tower's backward (every gradient of that tower); the
optimiser's zero_grad() removed from _train_epoch (absent token ids, every gradient from step 1 on); BatchNorm's momentum 0.2 for 0.1
(running statistics, DCMHT).

Every figure is printed before the first assertion; with XMH_TRAIN_STEP_TABLE naming a file the table is appended to it
(profiles/train_step_f64.txt was written so)."""
import os
import re

import numpy as np
import pytest
import torch

import train_step_cases as TS

pytestmark = pytest.mark.gpu

TOL_FACTOR = 4.0
NULL_FACTOR = 32.0


def _np(t):
    return t.detach().cpu().numpy()


def _device_masks(model):
    """seeded device generators for the two heads' dropout, and the same masks drawn from twin generators"""
    masks = [[], []]
    for i, head in enumerate((model.hash.img_hash, model.hash.txt_hash)):
        head.generator = torch.Generator(device="cuda").manual_seed(100 + i)
        twin = torch.Generator(device="cuda").manual_seed(100 + i)
        masks[i] = [(torch.rand(TS.B, TS.K, device="cuda", generator=twin) >= TS.DROP_P).cpu() for _ in range(TS.STEPS)]
    return [(masks[0][s], masks[1][s]) for s in range(TS.STEPS)]


def _record(t, arch, names, pre, loss):
    """the trainer's state after a step in the layout of a restatement record"""
    rec = {k: {} for k in ("grad", "clipped", "p", "m", "v")}
    rec["loss"], rec["step"] = loss, {}
    for n, p in names.items():
        if TS.group_of(n) == "hyp":
            rec["grad"][n], rec["p"][n] = _np(p.grad), _np(p)
            rec["proxy_buf"] = _np(t.optimizer_loss.state[p]["momentum_buffer"])
            continue
        st = t.optimizer.state[p]
        rec["step"][n] = st.get("step")
        if p.grad is None:
            continue
        rec["grad"][n], rec["clipped"][n], rec["p"][n] = _np(pre[n]), _np(p.grad), _np(p)
        rec["m"][n], rec["v"][n] = _np(st["next_m"]), _np(st["next_v"])
    rec["buffers"] = {k: (_np(v) if v.is_floating_point() else int(v)) for k, v in t.model.state_dict().items() if TS.is_buffer(k)}
    return rec


def _structure(arch, s, rec, sd0, r64, ids_seen, names, t, problems):
    """the exact zeros and bit equalities of the CPU module's structure list, on the device"""
    def bad(cond, *what):
        if cond:
            problems.append((s,) + what)
    p = names["backbone.logit_scale"]
    bad(not torch.equal(p.detach().cpu(), sd0["backbone.logit_scale"]) or p.grad is not None or len(t.optimizer.state[p]) != 0, "logit_scale")
    bad(sorted(rec["grad"]) != sorted(r64[s]["grad"]), "the parameters with a gradient", sorted(set(rec["grad"]) ^ set(r64[s]["grad"])))
    bad(any(v != s + 1 for n, v in rec["step"].items() if n != "backbone.logit_scale"), "step counters")
    by_id = {id(q): n for n, q in names.items()}
    order = [by_id[id(q)] for g in t.optimizer.param_groups for q in g["params"] if q.grad is not None]
    want = [r64[s]["next_lr"][TS.group_of(n)] for n in order]
    got = t.optimizer.get_lr()
    bad(len(got) != len(want) or not np.allclose(got, want, rtol=1e-15, atol=0), "get_lr")
    bad({g["t_total"] for g in t.optimizer.param_groups} != {TS.STEPS}, "t_total")
    ids = ids_seen[-1]
    vocab = sd0["backbone.token_embedding.weight"].shape[0]
    for kind in ("grad", "clipped", "m", "v"):
        seen = np.unique(ids if kind in ("grad", "clipped") else np.concatenate(ids_seen))
        absent = np.setdiff1d(np.arange(vocab), seen)
        bad(rec[kind]["backbone.token_embedding.weight"][absent].any(), kind, "absent token ids")
        bad(rec[kind]["backbone.positional_embedding"][ids.shape[1]:].any(), kind, "positional rows >= L")
        if arch == "DCMHT":
            for mod in ("img", "txt"):
                e = sd0["hash.%s_hash.norm.weight" % mod].shape[0]
                for k in ("in_proj_weight", "in_proj_bias"):
                    bad(rec[kind]["hash.%s_hash.atten.%s" % (mod, k)][:2 * e].any(), kind, mod, k, "q / k thirds")
    if s == 0:                                                                           # rate 0: nothing moves, the moments are filled
        for n in rec["m"]:
            bad(not np.array_equal(rec["p"][n], sd0[n].numpy()), "step 0 moved", n)
            bad(not rec["m"][n].any() or not rec["v"][n].any(), "step 0 left the moments empty", n)
    if arch == "DCMHT":
        bad(rec["buffers"]["hash.img_hash.norm.num_batches_tracked"] != s + 1, "num_batches_tracked")


@pytest.mark.parametrize("arch", list(TS.ARCHS))
def test_five_training_steps_follow_the_float64_trajectory(arch, tmp_path, monkeypatch):
    from xmh.optim import BertAdam
    t = TS.trainer(arch, tmp_path, 0)
    sd0, raw = TS.capture(t)
    batches = TS.batches_of(raw)
    masks = _device_masks(t.model) if arch == "DSPH" else None
    r64 = TS.run(arch, sd0, batches, masks=masks)
    cond = TS.check_conditions(arch, r64)                                                # before any comparison
    null = TS.null_set(r64)
    assert null == (TS.NULL_DCMHT if arch == "DCMHT" else ())
    _, e_ref, noise32 = TS.yardstick(arch, sd0, batches, r64, masks, null)

    names = dict(t.model.named_parameters())
    pre, losses = {}, []
    step, compute_loss = BertAdam.step, t.compute_loss

    def recording_step(self, closure=None):                                              # the gradients as the optimiser receives them
        pre.clear()
        pre.update({n: p.grad.detach().clone() for n, p in names.items() if p.grad is not None and TS.group_of(n) != "hyp"})
        return step(self, closure)

    def recording_loss(**kw):
        loss = compute_loss(**kw)
        losses.append(loss.detach())
        return loss
    monkeypatch.setattr(BertAdam, "step", recording_step)
    t.compute_loss = recording_loss
    assert getattr(t, "optimizer", None) is None and t.epochs == TS.STEPS

    per_port, problems, ids_seen, lines = [], [], [], []
    null_g = {n: [] for n in null}
    for s in range(TS.STEPS):
        t.train_loader = [raw[s % 2]]
        t.train_epoch(s)
        assert len(losses) == s + 1 and t.global_step == s + 1
        rec = _record(t, arch, names, pre, float(losses[-1]))
        ids_seen.append(raw[s % 2][1].numpy().reshape(TS.B, -1))
        ref = r64[s]
        _structure(arch, s, rec, sd0, r64, ids_seen, names, t, problems)
        errs = TS.errors(rec, ref, sd0, null)
        per_port.append(errs)
        logged = float(re.search(r"loss: (?:tensor\()?([-+0-9.eE]+|nan|inf)", t.lines[-1]).group(1))
        lines.append("%s step %d loss %.8f f64 %.8f logged %.4f  lr %s" % (arch, s, rec["loss"], ref["loss"], logged, ref["lr"]))
        if abs(rec["loss"] - ref["loss"]) > 5e-5 * abs(ref["loss"]) + 1e-6 or not np.isfinite(rec["loss"]):
            problems.append((s, "loss", rec["loss"], ref["loss"]))
        if abs(logged - rec["loss"]) > 5.1e-5 + 1e-6 * abs(rec["loss"]):                 # four printed decimals of an fp32 number
            problems.append((s, "logged loss", logged, rec["loss"]))
        for (q, n), e in errs.items():
            key = (q, TS.kind_of(n) if n else "")
            if q != "loss" and not e <= TOL_FACTOR * e_ref[key]:
                problems.append((s, q, n, "e_port %.2e" % e, "e_ref %.2e" % e_ref[key], "ratio %.2f" % (e / e_ref[key] if e_ref[key] else np.inf)))
        # the null set: absolute bounds
        for n in null:
            g = float(np.abs(rec["grad"][n]).max())
            null_g[n].append(g)
            budget = sum(r64[j]["lr"][TS.group_of(n)] * max(null_g[n][:j + 1]) / TS.ADAM["e"] for j in range(s + 1))
            d = float(np.abs(TS.quantity(rec, "delta", n, sd0) - TS.quantity(ref, "delta", n, sd0)).max())
            lines.append("%s step %d null %-40s max|g| port %.2e  f32 %.2e  f64 %.2e   |delta - f64| %.2e  bound %.2e"
                         % (arch, s, n, g, noise32[s][n], float(np.abs(ref["grad"][n]).max()), d, budget))
            if not g <= NULL_FACTOR * noise32[s][n]:
                problems.append((s, "null gradient", n, g, noise32[s][n]))
            if not d <= budget:
                problems.append((s, "null delta", n, d, budget))
            if float(np.abs(rec["m"][n]).max()) > max(null_g[n]) or float(rec["v"][n].max()) > max(null_g[n]) ** 2:
                problems.append((s, "null moments", n))

    e_port = TS.pool(per_port)
    for key, v in cond.items():
        lines.append("%s condition step %d %-6s %s" % ((arch,) + key + (v,)))
    lines += TS.table(arch, e_ref, e_port)
    worst = {}
    for key, e in e_port.items():
        if e_ref.get(key):
            worst[key[0]] = max(worst.get(key[0], 0.0), e / e_ref[key])
    lines.append("%s worst e_port / e_ref per quantity: %s" % (arch, " ".join("%s %.2f" % kv for kv in sorted(worst.items()))))
    print("\n".join(lines))                                                              # every figure before the first assertion
    if os.environ.get("XMH_TRAIN_STEP_TABLE"):
        with open(os.environ["XMH_TRAIN_STEP_TABLE"], "a") as f:
            f.write("\n".join(lines) + "\n")
    assert not problems, (len(problems), problems[:12])
    assert set(e_port) == set(e_ref)
