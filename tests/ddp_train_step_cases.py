"""Shared by tests/test_ddp_train_step_cpu.py and tests/test_gpu_ddp_train.py (not a test module): the DISTRIBUTED training step of
the DCMHT and DSPH runners restated from the pieces of tests/train_step_cases.py, in the dtype it is handed.

One step over W ranks: every rank's shard goes through the towers and its heads; DCMHT's image BatchNorm takes its statistics from
the concatenation of all shards' inputs (what the reference's SyncBatchNorm computes; the running variance is unbiased over n_total,
the batch counter moves by one); the loss is formed per shard, and the parameters step with the gradient of (1 / W) sum_r loss_r
-- the mean over the ranks that the gradient all-reduce forms.  BertAdam over the backbone and head groups and SGD over DSPH's
proxies are train_step_cases' own.  With W = 1 the operations are those of train_step_cases.run in the same order: the two agree to
the bit.

The case: train_step_cases.config with 16 training pairs and a batch of 2 B = 8, so that two ranks get B = 4 rows per step and two
batches each from torch's DistributedSampler (shuffle on, no set_epoch: every epoch the same order); STEPS = 3 steps on those two
batches in turn, each its own train_epoch call with t_total = STEPS.  The conditions of train_step_cases.check_conditions are re-asserted
per shard (`check_conditions`); DATA_SEED is the first seed from train_step_cases.DATA_SEED on whose shards meet them for both cases."""
import numpy as np
import torch

import bertadam_cases as AC
import dcmht_loss_cases as DC
import train_step_cases as TS
from oracle import encode as enc
from oracle import losses as OL

W = 2
STEPS = 3
TRAIN_NUM = 4 * TS.B
DATA_SEED = TS.DATA_SEED
ADAM = dict(TS.ADAM, t_total=STEPS)


def config(arch, out_dir, device, data_seed=None):
    c = TS.config(arch, out_dir, device, DATA_SEED if data_seed is None else data_seed)
    c["run"].update(train_num=TRAIN_NUM, batch_size=W * TS.B, epochs=STEPS, shuffle=True)
    return c


def trainer(arch, out_dir, device, data_seed=None, **run):
    """a ONE-process runner of the case (model and data: the ranks' shards are cut from its training split by `shards`)"""
    import types
    import xmh.models  # noqa: F401
    import xmh.runners  # noqa: F401
    from xmh.common.register import registry
    from xmh.utils.config import Config
    c = config(arch, out_dir, device, data_seed)
    c["run"].update(run)
    t = registry.get_runner_class(TS.ARCHS[arch]).from_config(cfg=Config(c), autorun=False)
    t.lines = []
    t.logger = types.SimpleNamespace(info=t.lines.append)
    return t


def shards(data, world=W, batch=TS.B):
    """-> list over the batches of a rank's epoch of [per rank: (image, ids, label)], as build_loader cuts them"""
    from torch.utils.data import DataLoader
    from torch.utils.data.distributed import DistributedSampler
    per_rank = []
    for r in range(world):
        loader = DataLoader(data, batch_size=batch, num_workers=0, collate_fn=getattr(data, "collate", None),
                            sampler=DistributedSampler(data, num_replicas=world, rank=r, shuffle=True))
        per_rank.append([(image, ids, label) for image, ids, _, label, _ in loader])
    assert len({len(b) for b in per_rank}) == 1
    return [list(step) for step in zip(*per_rank)]


def hyper_of(name):
    return dict(ADAM, lr=TS.OPT_CFG["backbone_lr" if TS.group_of(name) == "backbone" else "lr"])


def _dcmht_img_heads(xs, t, eps=TS.NORM_EPS):
    """train_step_cases.dcmht_head for the image head of every shard, the BatchNorm over the concatenation of the shards' o"""
    F = torch.nn.functional
    e = xs[0].shape[1]
    os_ = [F.linear(F.linear(x, t["atten.in_proj_weight"][2 * e:], t["atten.in_proj_bias"][2 * e:]), t["atten.out_proj.weight"],
                    t["atten.out_proj.bias"]) for x in xs]
    o = os_[0] if len(os_) == 1 else torch.cat(os_)
    n = (o - o.mean(0)) / torch.sqrt(o.var(0, unbiased=False) + eps) * t["norm.weight"] + t["norm.bias"]
    out = []
    for n_r in (n,) if len(os_) == 1 else torch.split(n, [x.shape[0] for x in xs]):
        z = F.linear(n_r, t["fc2.weight"], t["fc2.bias"])
        f = torch.relu(z)
        out.append((torch.softmax(f.view(f.shape[0], -1, 2), -1).view(f.shape[0], -1), {"z": z, "n": n_r}))
    return out, o


def _forward(arch, t, buf, shard_batches, masks, dtype):
    clip = {k[len("backbone."):]: x for k, x in t.items() if k.startswith("backbone.")}
    heads = {mod: {k[len("hash.%s_hash." % mod):]: x for k, x in t.items() if k.startswith("hash.%s_hash." % mod)} for mod in ("img", "txt")}
    embeds = []
    for image, ids, _ in shard_batches:
        n = image.shape[0]
        fed = dict(clip, **{k: clip[k].unsqueeze(0).repeat(n, 1, 1) for k in ("visual.proj", "text_projection")})
        embeds.append((enc.clip_image(fed, image.to(dtype)), enc.clip_text(fed, ids, None)))
    rec, losses = {"z": {}, "tie": {}, "cos": {}}, []
    if arch == "DCMHT":
        img, o = _dcmht_img_heads([e[0] for e in embeds], heads["img"])
        TS.update_bn(buf, o.detach())
        for r, ((pi, ai), (_, e_txt), (_, _, labels)) in enumerate(zip(img, embeds, shard_batches)):
            pt, at = TS.dcmht_head(e_txt, heads["txt"], False)
            for mod, a in (("img", ai), ("txt", at)):
                rec["z"][(r, mod)] = a["z"].detach().double().numpy()
                rec["tie"][(r, mod)] = TS.tie_bound(a["n"].detach().numpy(), heads[mod]["fc2.weight"].detach().numpy())
            losses.append(DC.terms(pi, pt, labels, TS.K, "euclidean")[0])
    else:
        for r, ((e_img, e_txt), (_, _, labels)) in enumerate(zip(embeds, shard_batches)):
            ci = TS.dsph_head(e_img, heads["img"]["fc.weight"], heads["img"]["fc.bias"], masks[r][0].to(dtype))
            ct = TS.dsph_head(e_txt, heads["txt"]["fc.weight"], heads["txt"]["fc.bias"], masks[r][1].to(dtype))
            rec["cos"][r] = TS.hyp_cosines(ci, ct, t["hyp.proxies"], labels)
            losses.append(OL.hyp_terms(ci, ct, t["hyp.proxies"], labels, TS.HYP_MODEL["threshold"], TS.HYP_MODEL["alpha"])["loss"])
    rec["losses"] = [float(x.detach()) for x in losses]
    rec["loss_t"] = losses[0] if len(losses) == 1 else sum(losses[1:], losses[0]) / len(losses)
    return rec


def run(arch, sd0, batches, steps=STEPS, masks=None, dtype=torch.float64, keep=None, hyper=hyper_of):
    """train_step_cases.run over shards: batches[s % len(batches)] is a list over the ranks of (image, ids, labels); masks (DSPH):
    per step, per rank (keep_img, keep_txt).  A record is train_step_cases' record; loss is (1 / W) sum_r loss_r, losses the ranks'
    own (what each rank logs), z / tie are keyed by (rank, modality) and cos by rank."""
    np_dtype = np.float64 if dtype == torch.float64 else np.float32
    out = []
    with DC.one_thread():
        t = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd0.items() if v.is_floating_point() and not TS.is_buffer(k)}
        buf = {k: (v.detach().to(dtype).clone() if v.is_floating_point() else int(v)) for k, v in sd0.items() if TS.is_buffer(k)}
        adam = [k for k in t if TS.group_of(k) != "hyp"]
        m = {k: np.zeros(tuple(t[k].shape), np_dtype) for k in adam}
        v = {k: np.zeros(tuple(t[k].shape), np_dtype) for k in adam}
        sgd = torch.optim.SGD([t["hyp.proxies"]], **TS.HYP_CFG) if arch == "DSPH" else None
        for s in range(steps):
            for x in t.values():
                x.grad = None
            rec = _forward(arch, t, buf, batches[s % len(batches)], None if masks is None else masks[s], dtype)
            rec["loss_t"].backward()
            rec["loss"] = float(rec.pop("loss_t").detach())
            assert t["backbone.logit_scale"].grad is None
            for kind in TS.QUANTITIES[:2] + ("p",) + TS.QUANTITIES[3:]:
                rec[kind] = {}
            rec["lr"], rec["next_lr"] = {}, {}
            for k in adam:
                if t[k].grad is None:
                    continue
                h = hyper(k)
                g = t[k].grad.numpy().copy()
                rec["lr"][TS.group_of(k)], rec["next_lr"][TS.group_of(k)] = AC.lr_f64(h, s), AC.lr_f64(h, s + 1)
                p, m[k], v[k], gc = AC.step_f64(t[k].detach().numpy(), g, m[k], v[k], AC.lr_f64(h, s), h)
                assert p.dtype == m[k].dtype == v[k].dtype == np_dtype
                with torch.no_grad():
                    t[k].copy_(torch.from_numpy(p))
                rec["grad"][k], rec["clipped"][k], rec["p"][k], rec["m"][k], rec["v"][k] = TS.pack(g), TS.pack(np.asarray(gc)), p, TS.pack(m[k]), TS.pack(v[k])
            rec["count"] = s + 1
            if sgd is not None:
                rec["grad"]["hyp.proxies"] = t["hyp.proxies"].grad.numpy().copy()
                sgd.step()
                rec["p"]["hyp.proxies"] = t["hyp.proxies"].detach().numpy().copy()
                rec["proxy_buf"] = sgd.state[t["hyp.proxies"]]["momentum_buffer"].numpy().copy()
            rec["buffers"] = {k: (b.numpy().copy() if torch.is_tensor(b) else b) for k, b in buf.items()}
            out.append(rec if keep is None else keep(s, rec))
    return out


def check_conditions(arch, r64):
    """train_step_cases.check_conditions for every shard of every step -> what was measured, keyed (step, rank, what)"""
    out = {}
    for s, rec in enumerate(r64):
        if arch == "DCMHT":
            for (r, mod), z in rec["z"].items():
                ratio = np.abs(z) / rec["tie"][(r, mod)]
                out[(s, r, mod)] = (float(np.abs(z).min()), float(ratio.min()))
                assert z.shape[1] == 2 * TS.K and ratio.min() > 1.0, ("fc2 pre-activation inside its tie bound", s, r, mod, out[(s, r, mod)])
        else:
            for r, cos in rec["cos"].items():
                for key, c in cos.items():
                    gap = float(np.abs(c - TS.HYP_MODEL["threshold"]).min()) if c.size else float("inf")
                    out[(s, r, key)] = (int(c.size), gap)
                    assert gap >= TS.GAP, ("HyP cosine within GAP of the threshold", s, r, key, gap)
                assert cos["neg"].size == cos["neg_t"].size > 0
    return out


def yardstick(arch, sd0, batches, r64, masks=None, null=()):
    """train_step_cases.yardstick: the float32 restatement of the distributed step against the float64 one on these very inputs"""
    def keep(s, rec):
        return TS.errors(rec, r64[s], sd0, null), {n: float(np.abs(TS.dense(rec["grad"][n])).max()) for n in null}
    got = run(arch, sd0, batches, len(r64), masks, torch.float32, keep)
    return [g[0] for g in got], TS.pool([g[0] for g in got]), [g[1] for g in got]


def cpu_masks(seed=7, steps=STEPS, world=W, rows=TS.B):
    """DSPH keep masks for the CPU module: per step, per rank (keep_img, keep_txt), p = 0.2, seeded"""
    g = torch.Generator().manual_seed(seed)
    return [[tuple((torch.rand(rows, TS.K, generator=g) >= TS.DROP_P) for _ in range(2)) for _ in range(world)] for _ in range(steps)]
