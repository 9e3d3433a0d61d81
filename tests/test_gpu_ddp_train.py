"""GPU, several processes: distributed training (xmh/ddp.py, the runners' epoch with distributed=True).

The processes share cuda:0 and talk over gloo (run.share_gpu, the pattern of tests/test_gpu_runner.py's two-rank evaluation); they are
spawned without joining and joined against a deadline, so that a mismatched collective is a failure and not a hang.  At most four
processes hold the GPU at a time (the test's own and three ranks).

The reducer alone, W = 3, two rounds with different gradients and different parameters missing: every rank ends with the same bits;
a parameter no rank had a gradient for keeps ``.grad is None``; every element is within (W - 1) 2^-24 sum_r |t_r| of the float64 sum
of the W fp32 terms t_r = fl(g_r fl(1 / W)) the bucket carries (the bound of a sum of W fp32 terms in any order: W - 1 additions,
each rounding a partial sum that is at most sum_r |t_r|; tests/test_gpu_bucket.py pins the packed terms to exactly that product),
and within (W + 0.5) 2^-24 sum_r |g_r| / W of the exact mean, which adds the terms' own rounding (2^-25 for fl(1 / 3), 2^-24 for the
product).

DSPH, W = 2, three train_epoch calls on 61 training pairs (the sampler pads to 31 per rank; eight steps of 4, 4, ..., 3 pairs): after
every epoch both ranks hold, to the bit, the parameters, next_m, next_v, step counters, proxies and momentum buffers of a
single-process run that is made of the package's one-process pieces only: per step the forward and backward of rank 0's and rank 1's
batch in turn with that rank's dropout generator, ``p.grad = g0 * 0.5 + g1 * 0.5``, the optimisers' steps.  (A sum of two fp32 terms
does not depend on the order, and halving is exact.)

DCMHT, W = 2, three steps against the float64 restatement of the distributed step: see the test's own docstring.

Measured on an MI355X (gloo, both ranks on one card): the reducer's worst error is 0.91 of the three-term bound (0.77 of the bound
against the exact mean); DSPH bit-equal at every epoch; DCMHT's worst e_port / e_ref per quantity: loss 1.23, grad 2.17, clipped
2.75, delta 3.83 (hash.img_hash.norm.bias: 9.19e-06 against 2.40e-06), m 2.29, v 2.71, running statistics 1.00
(profiles/ddp_train_step_f64.txt).  On the commit before this feature every test of this module fails: xmh.ddp does not exist
(the reducer) and train_epoch raises NotImplementedError with distributed=True (DSPH, DCMHT)."""
import os
import socket
import sys
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _paths():
    for p_ in (ROOT, os.path.join(ROOT, "clip-based-cross-modal-hash_amd"), os.path.join(ROOT, "tests")):
        if p_ not in sys.path:
            sys.path.insert(0, p_)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")


def _free_port():
    with socket.socket() as s_:
        s_.bind(("127.0.0.1", 0))
        return s_.getsockname()[1]


def _spawn(fn, args, nprocs, deadline):
    """mp.spawn without joining; the children are terminated and the test fails when `deadline` seconds pass"""
    import torch.multiprocessing as mp
    ctx = mp.spawn(fn, args=args, nprocs=nprocs, join=False)
    end = time.monotonic() + deadline
    try:
        while not ctx.join(timeout=2.0):                     # raises when a child failed (and ends the others)
            if time.monotonic() > end:
                pytest.fail("%d ranks did not finish within %d s (a collective that not every rank entered?)" % (nprocs, deadline))
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.terminate()
        for p in ctx.processes:
            p.join(10)
            if p.is_alive():
                p.kill()


def _init_group(rank, world, port):
    import torch.distributed as dist
    torch.cuda.set_device(0)
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)


# ---- the reducer alone ----------------------------------------------------------------------------------------------------------------
W3 = 3
CHUNK = 16384
SHAPES = [(3,), (CHUNK + 1,), (129, 65), (1,), (2 * CHUNK + 5,), (7, 9)]
# round -> rank -> the parameters without a gradient there; parameter 3 never has one anywhere
MISSING = [{0: {3}, 1: {3, 2}, 2: {3}}, {0: {3, 0}, 1: {3}, 2: {3, 4, 0}}]


def _toy_model():
    m = torch.nn.Module()
    m.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.zeros(s)) for s in SHAPES])
    m.frozen = torch.nn.Parameter(torch.ones(5), requires_grad=False)                    # not part of the bucket
    return m


def _toy_grad(rnd, rank, i):
    gen = torch.Generator().manual_seed(1000 + 100 * rnd + 10 * rank + i)
    return torch.randn(SHAPES[i], generator=gen) * (10.0 ** (i - 2))


def _reducer_worker(rank, world, port, tmp):
    _paths()
    import torch.distributed as dist
    _init_group(rank, world, port)
    try:
        from xmh import _lib
        from xmh.ddp import GradReducer
        assert int(_lib.lib.xmh_bertadam_chunk()) == CHUNK
        model = _toy_model().cuda()
        with torch.no_grad():
            for i, p in enumerate(model.ps):
                p.copy_(_toy_grad(7 + rank, rank, i))                                    # another start on every rank
        red = GradReducer(model, world)
        assert len(red.params) == len(SHAPES)
        red.broadcast_parameters()
        out = {"params": [p.detach().cpu() for p in model.ps], "rounds": []}
        for rnd, missing in enumerate(MISSING):
            for i, p in enumerate(model.ps):
                p.grad = None if i in missing[rank] else _toy_grad(rnd, rank, i).cuda()
            red.reduce()
            assert all(p.grad is None or p.grad.data_ptr() == v.data_ptr() for p, v in zip(red.params, red.views))
            out["rounds"].append([None if p.grad is None else p.grad.detach().cpu().clone() for p in model.ps])
        out["collectives"] = red.collectives
        assert model.frozen.grad is None
        torch.save(out, os.path.join(tmp, "reducer%d.pt" % rank))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_reducer_three_ranks_same_bits_within_the_bound_of_a_three_term_sum(tmp_path):
    _spawn(_reducer_worker, (W3, _free_port(), str(tmp_path)), W3, 240)
    outs = [torch.load(os.path.join(str(tmp_path), "reducer%d.pt" % r)) for r in range(W3)]
    u = 2.0 ** -24
    for i in range(len(SHAPES)):                                                         # the broadcast: rank 0's start everywhere
        for r in range(W3):
            assert torch.equal(outs[r]["params"][i], _toy_grad(7, 0, i)), (r, i)
    lines = []
    for rnd, missing in enumerate(MISSING):
        for i in range(len(SHAPES)):
            got = [outs[r]["rounds"][rnd][i] for r in range(W3)]
            have = [r for r in range(W3) if i not in missing[r]]
            if not have:
                assert all(g is None for g in got), (rnd, i)
                continue
            assert all(g is not None for g in got), (rnd, i)
            for r in range(1, W3):
                assert torch.equal(got[0].view(torch.int32), got[r].view(torch.int32)), (rnd, i, r)
            terms = [_toy_grad(rnd, r, i) * (1.0 / W3) for r in have]                      # fp32, as the bucket carries them
            total = sum(t.double() for t in terms)
            mag = sum(t.double().abs() for t in terms)
            err = (got[0].double() - total).abs()
            exact = sum(_toy_grad(rnd, r, i).double() for r in have) / W3
            mag_exact = sum(_toy_grad(rnd, r, i).double().abs() for r in have) / W3
            err_exact = (got[0].double() - exact).abs()
            lines.append("round %d parameter %d ranks %s: max err / bound %.3f (terms), %.3f (exact mean)"
                         % (rnd, i, have, float((err / ((W3 - 1) * u * mag)).max()), float((err_exact / ((W3 + 0.5) * u * mag_exact)).max())))
            assert bool((err <= (W3 - 1) * u * mag).all()), lines[-1]
            assert bool((err_exact <= (W3 + 0.5) * u * mag_exact).all()), lines[-1]
    print("\n".join(lines))
    assert [o["collectives"] for o in outs] == [1 + len(MISSING)] * W3                   # one broadcast, one all-reduce per step


# ---- DSPH, two ranks ------------------------------------------------------------------------------------------------------------------
W2 = 2
EPOCHS = 3
TRAIN_NUM = 61


def _dsph_cfg(out_dir, state=""):
    import train_step_cases as TS
    from xmh.utils.config import Config
    c = TS.config("DSPH", out_dir, 0)
    c["dataset"]["retrieval_num"] = 64
    c["run"].update(train_num=TRAIN_NUM, batch_size=2 * TS.B, epochs=EPOCHS, shuffle=True, resume_model=state)
    return Config(c)


def _seed_dropout(model, rank):
    gens = [torch.Generator(device="cuda").manual_seed(100 + 10 * rank + i) for i in range(2)]
    model.hash.img_hash.generator, model.hash.txt_hash.generator = gens
    return gens


def _snapshot(t):
    snap = {}
    for n, p in t.model.named_parameters():
        snap["p/" + n] = p.detach().cpu().clone()
        for opt, keys in ((t.optimizer, ("next_m", "next_v", "step")), (t.optimizer_loss, ("momentum_buffer",))):
            st = opt.state.get(p, {})
            for k in keys:
                if k in st:
                    snap[k + "/" + n] = st[k].detach().cpu().clone() if torch.is_tensor(st[k]) else st[k]
    return snap


def _dsph_worker(rank, world, port, tmp, state):
    _paths()
    import torch.distributed as dist
    import xmh.models  # noqa: F401
    import xmh.runners  # noqa: F401
    from xmh.common.register import registry
    cfg = _dsph_cfg(os.path.join(tmp, "rank%d" % rank), state)
    cfg.run.distributed_addr, cfg.run.distributed_port, cfg.run.share_gpu = "127.0.0.1", port, True
    try:
        t = registry.get_runner_class("DSPHTrainer").from_config(rank, world, True, cfg, None, autorun=False)
        assert dist.get_world_size() == world and t.rank == rank
        per_rank = -(-TRAIN_NUM // world)
        assert len(t.train_loader.sampler) == per_rank and t.train_loader.batch_size == cfg.run.batch_size // world
        _seed_dropout(t.model, rank)
        for epoch in range(EPOCHS):
            t.train_epoch(epoch)
            torch.save(_snapshot(t), os.path.join(tmp, "rank%d_epoch%d.pt" % (rank, epoch)))
        steps = EPOCHS * len(t.train_loader)
        assert t.global_step == steps and t.reducer.collectives == 1 + steps             # one broadcast, one all-reduce per step
        assert t.optimizer.param_groups[0]["t_total"] == steps
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def _emulate(tmp_path, state):
    """the two ranks' steps in ONE process: per step both shards' forward and backward in turn, the halves added, the steps"""
    import xmh.models  # noqa: F401
    import xmh.runners  # noqa: F401
    from torch.utils.data import DataLoader
    from torch.utils.data.distributed import DistributedSampler
    from xmh.common.register import registry
    from xmh.runners.methods import _step
    t = registry.get_runner_class("DSPHTrainer").from_config(cfg=_dsph_cfg(tmp_path / "single", state), autorun=False)
    data = t.train_loader.dataset
    assert len(data) == TRAIN_NUM
    loaders = [DataLoader(data, batch_size=t.cfg.run.batch_size // W2, num_workers=0, collate_fn=getattr(data, "collate", None),
                          sampler=DistributedSampler(data, num_replicas=W2, rank=r, shuffle=True)) for r in range(W2)]
    t.train_loader = loaders[0]                                                          # t_total = steps of ONE rank times the epochs
    t.optimizer, t.optimizer_loss, t.lr_schedu = t.build_optimizer(t.cfg.get("optimizer"))
    gens = [_seed_dropout(t.model, r) for r in range(W2)]
    t.change_state(mode="train")
    params = [p for p in t.model.parameters() if p.requires_grad]
    snaps = []
    for epoch in range(EPOCHS):
        sizes = []
        for times, batches in enumerate(zip(*loaders), 1):
            t.global_step += 1
            halves = []
            for r, (image, text, kpm, label, index) in enumerate(batches):
                t.model.hash.img_hash.generator, t.model.hash.txt_hash.generator = gens[r]
                loss = _step(t, image.cuda(), text.cuda(), kpm, label, index.numpy(), epoch, times)
                t.optimizer.zero_grad()
                t.optimizer_loss.zero_grad()
                loss.backward()
                halves.append([None if p.grad is None else p.grad.detach().clone() for p in params])
                sizes.append(image.shape[0])
            for p, g0, g1 in zip(params, *halves):
                if g0 is None and g1 is None:
                    p.grad = None
                else:
                    p.grad = (torch.zeros_like(p) if g0 is None else g0 * 0.5) + (torch.zeros_like(p) if g1 is None else g1 * 0.5)
            t.optimizer.step()
            t.optimizer_loss.step()
        assert sizes[-1] == 3 and sizes[0] == 4 and len(sizes) == 2 * 8                  # the uneven last batch is part of the case
        snaps.append(_snapshot(t))
    return snaps


def test_dsph_two_ranks_three_epochs_equal_the_single_process_emulation_to_the_bit(tmp_path):
    import xmh.models  # noqa: F401
    import xmh.runners  # noqa: F401
    from xmh.common.register import registry
    state = str(tmp_path / "start.pth")
    first = registry.get_runner_class("DSPHTrainer").from_config(cfg=_dsph_cfg(tmp_path / "init"), autorun=False)
    torch.save(first.model.state_dict(), state)                                          # one start for the emulation and every rank
    del first
    want = _emulate(tmp_path, state)
    torch.cuda.empty_cache()
    _spawn(_dsph_worker, (W2, _free_port(), str(tmp_path), state), W2, 300)
    moved = 0
    for epoch in range(EPOCHS):
        for rank in range(W2):
            got = torch.load(os.path.join(str(tmp_path), "rank%d_epoch%d.pt" % (rank, epoch)))
            assert sorted(got) == sorted(want[epoch]), (epoch, rank, sorted(set(got) ^ set(want[epoch])))
            bad = [k for k, v in want[epoch].items()
                   if not (torch.equal(v.view(torch.int32), got[k].view(torch.int32)) if torch.is_tensor(v) else v == got[k])]
            assert not bad, (epoch, rank, len(bad), bad[:8])
        moved += sum(1 for k, v in want[epoch].items() if k.startswith("p/") and not torch.equal(v, want[0][k]))
    keys = list(want[-1])
    assert any(k.startswith("momentum_buffer/hyp.") for k in keys) and any(k.startswith("next_v/backbone.") for k in keys)
    assert "step/backbone.logit_scale" not in keys and "next_m/backbone.logit_scale" not in keys      # stateless, as in one process
    assert moved > 0                                                                     # the parameters did move between the epochs
    assert all(np.isfinite(v.double().sum().item()) for k, v in want[-1].items() if k.startswith("p/"))


# ---- DCMHT, two ranks, against the float64 restatement of the distributed step ------------------------------------------------------------
def _dcmht_worker(rank, world, port, tmp, state):
    _paths()
    import torch.distributed as dist
    import xmh.models  # noqa: F401
    import xmh.runners  # noqa: F401
    import ddp_train_step_cases as DS
    import train_step_cases as TS
    from test_gpu_train_step import _record
    from xmh.common.register import registry
    from xmh.optim import BertAdam
    from xmh.utils.config import Config
    c = DS.config("DCMHT", os.path.join(tmp, "rank%d" % rank), 0)
    c["run"].update(resume_model=state, distributed_addr="127.0.0.1", distributed_port=port, share_gpu=True)
    try:
        t = registry.get_runner_class("DCMHTTrainer").from_config(rank, world, True, Config(c), None, autorun=False)
        assert t.model.hash.img_hash.sync_group is not None and t.model.hash.txt_hash.sync_group is None
        raw = list(t.train_loader)
        assert len(raw) == 2 and all(b[0].shape[0] == TS.B for b in raw)
        names = dict(t.model.named_parameters())
        scale0 = names["backbone.logit_scale"].detach().clone()
        pre, losses = {}, []
        step, compute_loss = BertAdam.step, t.compute_loss

        def recording_step(self, closure=None):                                          # the gradients as the optimiser receives them
            pre.clear()
            pre.update({n: p.grad.detach().clone() for n, p in names.items() if p.grad is not None})
            return step(self, closure)

        def recording_loss(**kw):
            loss = compute_loss(**kw)
            losses.append(loss.detach())
            return loss
        BertAdam.step, t.compute_loss = recording_step, recording_loss
        for s in range(DS.STEPS):
            t.train_loader = [raw[s % 2]]
            t.train_epoch(s)
            rec = _record(t, "DCMHT", names, pre, float(losses[-1]))
            for kind in ("grad", "clipped", "m", "v"):
                rec[kind] = {n: TS.pack(a) for n, a in rec[kind].items()}
            p = names["backbone.logit_scale"]
            rec["logit_scale_ok"] = bool(torch.equal(p.detach(), scale0)) and p.grad is None and len(t.optimizer.state[p]) == 0
            rec["images"] = raw[s % 2][0].clone()
            rec["collectives"] = t.reducer.collectives
            rec["lr"] = t.optimizer.get_lr()
            torch.save(rec, os.path.join(tmp, "dcmht_rank%d_step%d.pt" % (rank, s)))
        assert t.optimizer.param_groups[0]["t_total"] == DS.STEPS
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_dcmht_two_ranks_three_steps_follow_the_float64_restatement(tmp_path):
    """After every step the two ranks hold the same bits (parameters, clipped gradients, next_m / next_v, BatchNorm's running
    statistics), and every quantity of tests/test_gpu_train_step.py's list follows the float64 restatement of the distributed step
    (tests/ddp_train_step_cases.py) under that module's rule: per kind e_port <= TOL_FACTOR (4) x e_ref, e_ref the float32 restatement
    against float64 on these inputs, pooled over steps and ranks; the null set with its absolute bounds.  Each rank's logged loss is
    its own shard's.  With XMH_DDP_TRAIN_STEP_TABLE naming a file the table is appended to it (profiles/ddp_train_step_f64.txt)."""
    import ddp_train_step_cases as DS
    import train_step_cases as TS
    from test_gpu_train_step import NULL_FACTOR, TOL_FACTOR
    t = DS.trainer("DCMHT", tmp_path / "single", 0)
    sd0 = {k: v.detach().cpu().clone() for k, v in t.model.state_dict().items()}
    state = str(tmp_path / "start.pth")
    torch.save(t.model.state_dict(), state)
    batches = DS.shards(t.train_loader.dataset)
    del t
    torch.cuda.empty_cache()
    r64 = DS.run("DCMHT", sd0, batches)
    cond = DS.check_conditions("DCMHT", r64)                                              # before any comparison
    null = TS.null_set(r64)
    assert null == TS.NULL_DCMHT
    _, e_ref, noise32 = DS.yardstick("DCMHT", sd0, batches, r64, None, null)
    _spawn(_dcmht_worker, (W2, _free_port(), str(tmp_path), state), W2, 300)

    recs = [[torch.load(os.path.join(str(tmp_path), "dcmht_rank%d_step%d.pt" % (r, s)), weights_only=False) for r in range(W2)]
            for s in range(DS.STEPS)]
    per_port, problems, lines = [], [], []
    null_g = {n: [] for n in null}
    for s, (ranks, ref) in enumerate(zip(recs, r64)):
        a, b = ranks
        for r in range(W2):
            if not torch.equal(ranks[r]["images"], batches[s % 2][r][0]):
                problems.append((s, r, "the rank's batch is not the restatement's shard"))
            if not ranks[r]["logit_scale_ok"]:
                problems.append((s, r, "logit_scale"))
            if ranks[r]["collectives"] != 1 + (s + 1):
                problems.append((s, r, "collectives of the bucket", ranks[r]["collectives"]))
            if ranks[r]["buffers"]["hash.img_hash.norm.num_batches_tracked"] != s + 1:
                problems.append((s, r, "num_batches_tracked"))
            if any(v != s + 1 for n, v in ranks[r]["step"].items() if n != "backbone.logit_scale"):
                problems.append((s, r, "step counters"))
            if sorted(ranks[r]["grad"]) != sorted(ref["grad"]):
                problems.append((s, r, "the parameters with a gradient", sorted(set(ranks[r]["grad"]) ^ set(ref["grad"]))))
        for kind in ("grad", "clipped", "p", "m", "v"):                                  # one gradient, one state on both ranks
            for n in a[kind]:
                if not np.array_equal(TS.dense(a[kind][n]).view(np.int32), TS.dense(b[kind][n]).view(np.int32)):
                    problems.append((s, "ranks differ", kind, n))
        for n, v in a["buffers"].items():
            if not (np.array_equal(v, b["buffers"][n]) if isinstance(v, np.ndarray) else v == b["buffers"][n]):
                problems.append((s, "ranks differ", "buffer", n))
        if a["loss"] == b["loss"]:
            problems.append((s, "both ranks report one loss: each logs its own shard's"))
        for r, rec in enumerate(ranks):
            errs = TS.errors(rec, dict(ref, loss=ref["losses"][r]), sd0, null)
            per_port.append(errs)
            lines.append("DCMHT W=2 step %d rank %d loss %.8f f64 %.8f (mean over the ranks %.8f)  lr %s"
                         % (s, r, rec["loss"], ref["losses"][r], ref["loss"], ref["lr"]))
            if abs(rec["loss"] - ref["losses"][r]) > 5e-5 * abs(ref["losses"][r]) + 1e-6 or not np.isfinite(rec["loss"]):
                problems.append((s, r, "loss", rec["loss"], ref["losses"][r]))
            for (q, n), e in errs.items():
                key = (q, TS.kind_of(n) if n else "")
                if q != "loss" and not e <= TOL_FACTOR * e_ref[key]:
                    problems.append((s, r, q, n, "e_port %.2e" % e, "e_ref %.2e" % e_ref[key], "ratio %.2f" % (e / e_ref[key] if e_ref[key] else np.inf)))
        for n in null:                                                                   # the null set: absolute bounds, rank 0 (the ranks agree)
            g = float(np.abs(TS.dense(a["grad"][n])).max())
            null_g[n].append(g)
            budget = sum(r64[j]["lr"][TS.group_of(n)] * max(null_g[n][:j + 1]) / DS.ADAM["e"] for j in range(s + 1))
            d = float(np.abs(TS.quantity(a, "delta", n, sd0) - TS.quantity(ref, "delta", n, sd0)).max())
            lines.append("DCMHT W=2 step %d null %-40s max|g| port %.2e  f32 %.2e  f64 %.2e   |delta - f64| %.2e  bound %.2e"
                         % (s, n, g, noise32[s][n], float(np.abs(ref["grad"][n]).max()), d, budget))
            if not g <= NULL_FACTOR * noise32[s][n]:
                problems.append((s, "null gradient", n, g, noise32[s][n]))
            if not d <= budget:
                problems.append((s, "null delta", n, d, budget))
            if float(np.abs(TS.dense(a["m"][n])).max()) > max(null_g[n]) or float(TS.dense(a["v"][n]).max()) > max(null_g[n]) ** 2:
                problems.append((s, "null moments", n))
    e_port = TS.pool(per_port)
    for key, v in cond.items():
        lines.append("DCMHT W=2 condition step %d rank %d %-6s %s" % (key + (v,)))
    lines += TS.table("DCMHT W=2", e_ref, e_port)
    worst = {}
    for key, e in e_port.items():
        if e_ref.get(key):
            worst[key[0]] = max(worst.get(key[0], 0.0), e / e_ref[key])
    lines.append("DCMHT W=2 worst e_port / e_ref per quantity: %s" % " ".join("%s %.2f" % kv for kv in sorted(worst.items())))
    print("\n".join(lines))                                                              # every figure before the first assertion
    if os.environ.get("XMH_DDP_TRAIN_STEP_TABLE"):
        with open(os.environ["XMH_DDP_TRAIN_STEP_TABLE"], "a") as f:
            f.write("\n".join(lines) + "\n")
    assert not problems, (len(problems), problems[:12])
    assert set(e_port) == set(e_ref)
