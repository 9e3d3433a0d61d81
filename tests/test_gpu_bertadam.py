"""GPU: the fused BertAdam step (xmh_optim.hip behind xmh/optim.py) against the reference's own trajectories of
tests/golden/bertadam.npz and against the float64 restatement of tests/bertadam_cases.py (validated against the same goldens by
tests/test_bertadam_cpu.py): every golden case step by step, chunk edges, misaligned views, NaN / inf isolation, parameters
without a gradient, bit-reproducibility, no host synchronisation, the state dict, and five steps of the DCMHT and DSPH heads
behind build_optimizer.

Tolerances.  Per tensor and kind (p, next_m, next_v, post-step grad), e = max|got - fp64| / max|fp64| on the whole tensor.  The
yardstick is the reference's own fp32 error e_ref stored in the golden file per kind (the largest over every case, step and
tensor): the kernel must stay within TOL_FACTOR * e_ref.  Factor 4, as in test_gpu_head_grad.py: an fp32 chain in a different
but equally long order, with FMA contraction and the device's division and sqrt, may lose about twice the reference's bits at
each of two stages.  Against the fp32 golden itself (e_ref away from fp64) the bound is (TOL_FACTOR + 1) * e_ref."""
import copy
import types

import numpy as np
import pytest
import torch

import bertadam_cases as BC
from train_step_cases import dcmht_head as _dcmht64

pytestmark = pytest.mark.gpu

TOL_FACTOR = 4.0
STORED = [c for c, spec in BC.CASES.items() if spec.get("stored", True)]


def _tol(kind, factor=TOL_FACTOR):
    return factor * float(BC.golden()["eref_" + kind])


def _chunk():
    from xmh import _lib
    return int(_lib.lib.xmh_bertadam_chunk())


def _optimizer(tensors, params):
    from xmh.optim import BertAdam
    groups = [dict(params=[params[t] for t, s in enumerate(tensors) if s["group"] == gi],
                   **next(s["hyper"] for s in tensors if s["group"] == gi)) for gi in sorted({s["group"] for s in tensors})]
    return BertAdam(groups, lr=BC.DEFAULTS["lr"])


def _record(opt, params):
    rec = {k: [None] * len(params) for k in BC.KINDS}
    for t, p in enumerate(params):
        st = opt.state[p]
        rec["p"][t] = p.detach().cpu().numpy()
        if len(st):
            rec["m"][t], rec["v"][t] = st["next_m"].cpu().numpy(), st["next_v"].cpu().numpy()
        if p.grad is not None:
            rec["grad"][t] = p.grad.cpu().numpy()
    rec["lr"] = opt.get_lr()
    rec["count"] = [opt.state[p]["step"] if len(opt.state[p]) else None for p in params]
    return rec


def _run(case, chunk=None, skip=()):
    """the case on the GPU -> list over steps of _record; skip: tensors left out of the optimiser altogether"""
    tensors, steps, nan = BC.resolve(case, chunk)
    params = [torch.nn.Parameter(torch.tensor(BC.draw_param(case, t, s["shape"])).cuda()) for t, s in enumerate(tensors)]
    keep = [t for t in range(len(tensors)) if t not in skip]
    opt = _optimizer([tensors[t] for t in keep], [params[t] for t in keep])
    out = []
    for s in range(steps):
        for t in keep:
            g = BC.draw_grad(case, tensors, t, s, nan)
            params[t].grad = None if g is None else torch.tensor(g).cuda()
        opt.step()
        out.append(_record(opt, params))
    return out


def _check_against_f64(case, got, own, nan=None):
    report, worst = [], {k: 0.0 for k in BC.KINDS}
    for s, (a, b) in enumerate(zip(got, own)):
        assert a["count"] == b["count"], (case, s)
        assert a["lr"] == b["lr"] or np.allclose(a["lr"], b["lr"], rtol=1e-15, atol=0), (case, s)
        for kind in BC.KINDS:
            for t, (x, y) in enumerate(zip(a[kind], b[kind])):
                assert (x is None) == (y is None), (case, s, t, kind)
                if x is None:
                    continue
                assert x.shape == y.shape and x.dtype == np.float32
                if BC.poisoned(nan, s, t, kind):
                    assert np.isnan(x).all(), (case, s, t, kind)
                    continue
                assert np.isfinite(x).all(), (case, s, t, kind)
                e = BC.rel_err(x, y)
                worst[kind] = max(worst[kind], e)
                if e > _tol(kind):
                    report.append((s, t, kind, e))
    print(case, " ".join("%s %.2e/%.2e" % (k, worst[k], _tol(k)) for k in BC.KINDS))      # each figure before any assertion
    assert not report, (case, report[:5])


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", STORED)
def test_every_golden_case_step_by_step(case):
    vals, lrs = BC.unpack(case)
    tensors, steps, nan = BC.resolve(case)
    got, own = _run(case), BC.run_f64(case)
    _check_against_f64(case, got, own, nan)
    for s in range(steps):
        assert got[s]["lr"] == lrs[s][0], (case, s)                              # the get_lr() lists are equal
        assert [(-1 if c is None else c) for c in got[s]["count"]] == lrs[s][1]
        for (gs, t, kind), (_, f32) in vals.items():
            if gs != s or BC.poisoned(nan, s, t, kind):
                continue
            scale = float(np.abs(own[s][kind][t]).max()) or 1.0
            err = float(np.abs(BC.thin(got[s][kind][t]).astype(np.float64) - f32.astype(np.float64)).max()) / scale
            assert err <= _tol(kind, TOL_FACTOR + 1), (case, s, t, kind, err)
    if case == "cosine":                                                         # lr is exactly 0 at the first step of a warm-up
        for t, spec in enumerate(tensors):
            assert np.array_equal(got[0]["p"][t], BC.draw_param(case, t, spec["shape"]))


# 2 ---------------------------------------------------------------------------------------------------------------------------
def test_chunk_edges_and_their_small_neighbours():
    chunk = _chunk()
    tensors, _, _ = BC.resolve("large", chunk)
    assert [int(np.prod(s["shape"])) for s in tensors] == [chunk - 1, 1, chunk + 1, 65, 2 * chunk + 7]
    _check_against_f64("large", _run("large", chunk), BC.run_f64("large", chunk))


def test_a_gradient_just_below_and_just_above_the_clipping_norm():
    from xmh.optim import BertAdam
    rng = np.random.default_rng(5)
    gs = []
    for n, target in ((1000, 1.0 - 1e-3), (1000, 1.0 + 1e-3), (5, 1.0 - 1e-3), (5, 1.0 + 1e-3)):
        g = rng.standard_normal(n)
        gs.append((g * (target / np.sqrt((g * g).sum()))).astype(np.float32))
    params = [torch.nn.Parameter(torch.zeros(len(g), device="cuda")) for g in gs]
    opt = BertAdam(params, lr=0.01, max_grad_norm=1.0)
    for p, g in zip(params, gs):
        p.grad = torch.tensor(g).cuda()
    opt.step()
    for i, (p, g) in enumerate(zip(params, gs)):
        after = p.grad.cpu().numpy()
        if i % 2 == 0:
            assert np.array_equal(after, g)                                      # below: not a bit of the gradient changes
        else:
            norm = float(np.sqrt((after.astype(np.float64) ** 2).sum()))
            assert not np.array_equal(after, g) and abs(norm - 1.0) < 1e-5       # above: scaled back onto the ball
            assert BC.rel_err(after, g.astype(np.float64) / (np.sqrt((g.astype(np.float64) ** 2).sum()) + 1e-6)) <= _tol("grad")


# 3 ---------------------------------------------------------------------------------------------------------------------------
def test_views_at_odd_element_offsets_and_their_guards():
    from xmh.optim import BertAdam
    n, h = 70, dict(BC.DEFAULTS, lr=0.01)
    rng = np.random.default_rng(9)
    layout = [(1, 1), (2, 2), (3, 3), (0, 2), (2, 0)]                            # (parameter offset, gradient offset) in elements
    pbufs = [torch.tensor(rng.standard_normal(n + 8).astype(np.float32)).cuda() for _ in layout]
    gbufs = [torch.tensor((0.5 * rng.standard_normal(n + 8)).astype(np.float32)).cuda() for _ in layout]
    p0, g0 = [b.cpu().numpy().copy() for b in pbufs], [b.cpu().numpy().copy() for b in gbufs]
    params = [torch.nn.Parameter(b[po:po + n]) for b, (po, _) in zip(pbufs, layout)]
    for p, b, (po, _) in zip(params, pbufs, layout):
        assert p.data_ptr() == b.data_ptr() + 4 * po
    opt = BertAdam(params, lr=0.01)
    for p, b, (_, go) in zip(params, gbufs, layout):
        p.grad = b[go:go + n]
        assert p.grad.data_ptr() == b.data_ptr() + 4 * go
    opt.step()
    for i, (po, go) in enumerate(layout):
        pa, ga = pbufs[i].cpu().numpy(), gbufs[i].cpu().numpy()
        for buf, before, off in ((pa, p0[i], po), (ga, g0[i], go)):
            assert np.array_equal(buf[:off], before[:off]) and np.array_equal(buf[off + n:], before[off + n:]), i     # guards, to the bit
        z = np.zeros(n)
        wp, wm, wv, wg = BC.step_f64(p0[i][po:po + n].astype(np.float64), g0[i][go:go + n].astype(np.float64), z, z, h["lr"], h)
        st = opt.state[params[i]]
        for kind, got, want in (("p", pa[po:po + n], wp), ("m", st["next_m"].cpu().numpy(), wm), ("v", st["next_v"].cpu().numpy(), wv),
                                ("grad", ga[go:go + n], wg)):
            assert BC.rel_err(got, want) <= _tol(kind), (i, kind)
        assert not np.array_equal(ga[go:go + n], g0[i][go:go + n])              # clipped: the gradient was written through the view


# 4 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_a_nan_or_inf_gradient_stays_in_its_tensor(bad):
    tensors, steps, nan = BC.resolve("nan")
    spec = dict(BC.CASES["nan"])
    assert nan[0] == 1
    if bad != bad:
        got = _run("nan")
    else:                                                                        # the same entry holds an inf instead
        params = [torch.nn.Parameter(torch.tensor(BC.draw_param("nan", t, s["shape"])).cuda()) for t, s in enumerate(tensors)]
        opt, got = _optimizer(tensors, params), []
        for s in range(steps):
            for t, p in enumerate(params):
                g = BC.draw_grad("nan", tensors, t, s, None)
                if (t, s) == nan[:2]:
                    g.reshape(-1)[nan[2]] = bad
                p.grad = torch.tensor(g).cuda()
            opt.step()
            got.append(_record(opt, params))
    clean = _run("nan", skip=(1,))                                               # the run without the poisoned tensor
    for s in range(steps):
        for kind in BC.KINDS:
            for t in (0, 2):
                assert np.array_equal(got[s][kind][t], clean[s][kind][t]), (s, t, kind)        # bit for bit
            x = got[s][kind][1]
            if bad != bad:
                assert np.isnan(x).all() == BC.poisoned(nan, s, 1, kind), (s, kind)
            elif s == nan[1]:
                # an infinite norm gives coef = 0: inf * 0 = NaN in that entry, and IEEE carries it on as the reference does
                # (g' = 0 elsewhere, so m and v only decay there and stay finite)
                assert np.isnan(x.reshape(-1)[nan[2]]), (s, kind)
                assert np.isfinite(np.delete(x.reshape(-1), nan[2])).all(), (s, kind)
    del spec


# 5 ---------------------------------------------------------------------------------------------------------------------------
def test_a_parameter_without_a_gradient_neither_moves_nor_ages():
    tensors, steps, _ = BC.resolve("skipped")
    got = _run("skipped")
    assert got[0]["count"] == [1, 1, None] and got[0]["m"][2] is None           # no state before the first gradient
    assert np.array_equal(got[0]["p"][2], BC.draw_param("skipped", 2, tensors[2]["shape"]))
    for s in (1, 2, 4):                                                          # tensor 1 has no gradient at these steps
        for kind in ("p", "m", "v"):
            assert np.array_equal(got[s][kind][1], got[s - 1][kind][1]), (s, kind)
        assert got[s]["count"][1] == got[s - 1]["count"][1] and got[s]["grad"][1] is None
    assert got[-1]["count"] == [7, 4, 6]
    h = tensors[1]["hyper"]
    assert got[-1]["lr"] == [BC.lr_f64(h, 7), BC.lr_f64(h, 4), BC.lr_f64(h, 6)]   # its schedule lags accordingly


# 6 ---------------------------------------------------------------------------------------------------------------------------
def test_two_runs_agree_to_the_bit():
    chunk = _chunk()
    for case in ("shapes", "large"):
        a, b = _run(case, chunk)[:3], _run(case, chunk)[:3]
        for ra, rb in zip(a, b):
            for kind in BC.KINDS:
                assert all(np.array_equal(x, y) for x, y in zip(ra[kind], rb[kind])), (case, kind)


# 7 ---------------------------------------------------------------------------------------------------------------------------
def test_step_does_not_synchronise():
    chunk = _chunk()
    tensors, _, _ = BC.resolve("large", chunk)
    params = [torch.nn.Parameter(torch.tensor(BC.draw_param("large", t, s["shape"])).cuda()) for t, s in enumerate(tensors)]
    opt = _optimizer(tensors, params)
    grads = [[torch.tensor(BC.draw_grad("large", tensors, t, s)).cuda() for t in range(len(tensors))] for s in range(4)]
    for p, g in zip(params, grads[0]):
        p.grad = g.clone()
    opt.step()                                                                   # warm-up: state, the device table, staging buffers
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for p, g in zip(params, grads[1]):
            p.grad.copy_(g)
        opt.step()                                                               # same pointers, another rate
        opt.zero_grad(set_to_none=True)
        for p, g in zip(params[:-1], grads[2]):                                  # new gradient tensors, one parameter without: a new table
            p.grad = g.clone()                                                   # (clones: a clipped gradient is written in place)
        opt.step()
        for p, g in zip(params, grads[3]):
            p.grad = g.clone()
        opt.step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert [opt.state[p]["step"] for p in params] == [4, 4, 4, 4, 3]
    own = BC.run_f64("large", chunk, grads=[[None if (s == 2 and t == 4) else g.cpu().numpy() for t, g in enumerate(gr)]
                                            for s, gr in enumerate(grads)] + [[None] * 5] * 2)
    for t, p in enumerate(params):
        assert BC.rel_err(p.detach().cpu().numpy(), own[3]["p"][t]) <= _tol("p"), t


# 8 ---------------------------------------------------------------------------------------------------------------------------
def test_state_dict_round_trip_continues_to_the_bit():
    tensors, steps, nan = BC.resolve("two_groups")

    def fresh():
        params = [torch.nn.Parameter(torch.tensor(BC.draw_param("two_groups", t, s["shape"])).cuda()) for t, s in enumerate(tensors)]
        return params, _optimizer(tensors, params)

    def advance(opt, params, lo, hi):
        for s in range(lo, hi):
            for t, p in enumerate(params):
                p.grad = torch.tensor(BC.draw_grad("two_groups", tensors, t, s)).cuda()
            opt.step()

    pa, oa = fresh()
    advance(oa, pa, 0, 3)
    sd = copy.deepcopy(oa.state_dict())
    assert set(sd["state"][0]) == {"step", "next_m", "next_v"} and sd["state"][0]["step"] == 3
    pb, ob = fresh()
    with torch.no_grad():
        for a, b in zip(pa, pb):
            b.copy_(a)
    cpu_sd = {"state": {k: {n: (v.cpu() if torch.is_tensor(v) else v) for n, v in st.items()} for k, st in sd["state"].items()},
              "param_groups": sd["param_groups"]}
    ob.load_state_dict(cpu_sd)                                                   # saved on the host, as a checkpoint file is
    advance(oa, pa, 3, steps)
    advance(ob, pb, 3, steps)
    for a, b in zip(pa, pb):
        assert torch.equal(a, b) and torch.equal(oa.state[a]["next_m"], ob.state[b]["next_m"])
        assert torch.equal(oa.state[a]["next_v"], ob.state[b]["next_v"]) and oa.state[a]["step"] == ob.state[b]["step"] == steps
    assert oa.get_lr() == ob.get_lr()


# 9 ---------------------------------------------------------------------------------------------------------------------------
def _trainer(tmp_path, arch, runner, K, C, **model):
    import xmh.models  # noqa: F401
    import xmh.runners  # noqa: F401
    from xmh.common.register import registry
    from xmh.utils.config import Config
    cfg = Config({
        "model": dict({"arch": arch, "clip_path": "synthetic:1814:vision_layers=1,transformer_layers=1"}, **model),
        "dataset": {"arch": "synthetic", "name": "synth", "num_classes": C, "retrieval_num": 40, "max_word": 32, "image_resolution": 224},
        "run": {"arch": runner, "output_dim": K, "device": 0, "batch_size": 8, "num_workers": 0, "is_train": False, "query_num": 8,
                "train_num": 24, "epochs": 4, "save_dir": str(tmp_path), "log_dir": str(tmp_path), "seed": 1814},
    })
    return registry.get_runner_class(runner).from_config(cfg=cfg, autorun=False)


def _embeddings(model, B):
    from xmh.models import weights as W
    image, (ids, _) = W.synth_images(2, B), W.synth_text(2, B)
    with torch.no_grad():
        return model.backbone.encode_image(image.cuda()).float(), model.backbone.encode_text(ids.cuda()).float()


def _labels(B, C):
    g = torch.Generator().manual_seed(3)
    L = (torch.rand(B, C, generator=g) < 0.15).float()
    L[torch.arange(B), torch.randint(0, C, (B,), generator=g)] = 1.0
    return L


class _Restated:
    """the BertAdam step on float64 torch leaves, through step_f64; one hyper-parameter set"""

    def __init__(self, leaves, hyper):
        self.leaves, self.h = leaves, hyper
        self.m = [np.zeros(tuple(x.shape)) for x in leaves]
        self.v = [np.zeros(tuple(x.shape)) for x in leaves]
        self.count = 0

    def zero_grad(self):
        for x in self.leaves:
            x.grad = None

    def step(self):
        lr = BC.lr_f64(self.h, self.count)
        for i, x in enumerate(self.leaves):
            p, self.m[i], self.v[i], _ = BC.step_f64(x.detach().numpy(), x.grad.numpy(), self.m[i], self.v[i], lr, self.h)
            with torch.no_grad():
                x.copy_(torch.from_numpy(p))
        self.count += 1


# The optimiser's configuration for the two end-to-end tests.  Two biases of the BatchNorm head (atten.in_proj_bias, atten.out_proj.bias)
# have a gradient that is mathematically zero, so what backward writes there is rounding noise (|g| of 1e-9 .. 1e-6 in fp32, 1e-17 in
# float64).  Adam normalises it like any other gradient: for |g| << e the update is (1 - b1) g / e per step, for |g| >> e it is a
# full +-0.7 sign step.  With the configs' e = 1e-6 the fp32 noise therefore moves those biases by up to lr * 0.7 per step where the
# float64 restatement does not move them at all -- the reference's own class shows the same drift between its fp32 and fp64 runs on
# the CPU (3e-5 after five steps at lr 0.002, against this comparison's 5e-5) -- so no fp32 implementation can be held to float64
# there.  e = 1e-3 keeps the noise's contribution at lr * 0.1 * 1e-6 / 1e-3 = 2e-7 per step and still lets every real gradient
# (|g| of 1e-3 .. 6e-2 here) move its parameter by about 1e-3 per step, twenty times the tolerance: a wrong step shows.  The
# configs' e = 1e-6 is what every golden case above runs with.  The other keys take build_optimizer's defaults.
OPT_CFG = {"lr": 0.002, "e": 1e-3}
OPT_HYPER = dict(lr=0.002, warmup=0.1, t_total=12, schedule="warmup_cosine", b1=0.9, b2=0.98, e=1e-3, weight_decay=0.2, max_grad_norm=1.0)


def test_dcmht_heads_follow_the_restatement_behind_build_optimizer(tmp_path):
    from oracle import losses as OL
    from xmh.optim import BertAdam
    from xmh.utils.config import Config
    B, K, C = 12, 16, 10
    trainer = _trainer(tmp_path, "DCMHT", "DCMHTTrainer", K, C)
    model = trainer.model.eval()
    assert len(trainer.train_loader) * trainer.epochs == OPT_HYPER["t_total"]
    opt, sched = trainer.build_optimizer(Config(OPT_CFG))
    assert type(opt) is BertAdam and sched is None and [g["lr"] for g in opt.param_groups] == [0.00001, 0.002]
    backbone = [p.detach().clone() for p in model.backbone.parameters()]
    emb_i, emb_t = _embeddings(model, B)
    labels = _labels(B, C)
    model.hash.train()
    d = {n: p.detach().cpu().double().clone().requires_grad_(True) for n, p in model.hash.named_parameters()}
    assert len(d) == 16
    opt_d = _Restated(list(d.values()), OPT_HYPER)
    xi, xt = emb_i.cpu().double(), emb_t.cpu().double()
    losses = []
    for _ in range(5):
        opt.zero_grad()
        opt_d.zero_grad()
        hi, ht = model.hash(emb_i, emb_t)
        loss, loss_dict = model.object_function(hi, ht, labels.cuda())
        loss.backward()
        assert all(p.grad is not None for p in model.hash.parameters()) and all(p.grad is None for p in model.backbone.parameters())
        pi = _dcmht64(xi, {k[len("img_hash."):]: v for k, v in d.items() if k.startswith("img_hash.")}, True, 1e-5)[0]
        pt = _dcmht64(xt, {k[len("txt_hash."):]: v for k, v in d.items() if k.startswith("txt_hash.")}, False, 1e-5)[0]
        want = OL.our_loss(pi, pt, labels, K, vartheta=model.vartheta, threshold=model.threshold, quan_alpha=model.quan_alpha)["loss"]
        want.backward()
        print("dcmht step loss %.8f want %.8f" % (float(loss), float(want)))
        assert abs(float(loss) - float(want)) <= 5e-5 * abs(float(want)) + 1e-6
        losses.append(float(loss))
        opt.step()
        opt_d.step()
    assert losses[-1] != losses[0]
    for n, p in model.hash.named_parameters():                                   # each figure before any assertion
        print("dcmht %-36s |p - f64| %.2e  max|f64| %.2e  max|grad| %.2e" % (n, float((p.detach().cpu().double() - d[n].detach()).abs().max()),
                                                                            float(d[n].detach().abs().max()), float(p.grad.abs().max())))
    for n, p in model.hash.named_parameters():
        assert float((p.detach().cpu().double() - d[n].detach()).abs().max()) <= 5e-5 * max(1.0, float(d[n].detach().abs().max())), n
    assert all(torch.equal(a, b) for a, b in zip(backbone, model.backbone.parameters()))         # no gradient: bit-unchanged
    assert all(len(opt.state[p]) == 0 for p in model.backbone.parameters())
    lines = []
    trainer.logger, trainer.optimizer = types.SimpleNamespace(info=lines.append), opt
    trainer.print_loss_dict(loss_dict, bits=K, epoch=1, times=2)
    assert len(lines) == 1 and lines[0].endswith("lr: %.9f" % BC.lr_f64(OPT_HYPER, 5)) and "[1/4], [2/3]" in lines[0]


def test_dsph_heads_and_proxies_follow_the_restatement_behind_build_optimizer(tmp_path):
    from oracle.losses import hyp_terms
    from xmh.optim import BertAdam
    from xmh.utils.config import Config
    B, K, C = 12, 16, 10
    trainer = _trainer(tmp_path, "DSPH", "DSPHTrainer", K, C, numclass=C, alpha=0.8, threshold=0.25)
    model = trainer.model.eval()
    opt, opt_loss, sched = trainer.build_optimizer(Config(dict(OPT_CFG, hyp={"lr": 0.05, "momentum": 0.0, "weight_decay": 0.0})))
    assert type(opt) is BertAdam and type(opt_loss) is torch.optim.SGD and sched is None
    backbone = [p.detach().clone() for p in model.backbone.parameters()]
    emb_i, emb_t = _embeddings(model, B)
    labels = _labels(B, C)
    model.hash.train()
    heads = (model.hash.img_hash, model.hash.txt_hash)
    for s, h in enumerate(heads):
        h.generator = torch.Generator(device="cuda").manual_seed(100 + s)
    twin = [torch.Generator(device="cuda").manual_seed(100 + s) for s in range(2)]     # draws the same masks for the restatement
    params = list(model.hash.parameters())
    assert len(params) == 4
    d = [p.detach().cpu().double().clone().requires_grad_(True) for p in params]
    dP = model.hyp.proxies.detach().cpu().double().clone().requires_grad_(True)
    opt_d, opt_dP = _Restated(d, OPT_HYPER), torch.optim.SGD([dP], lr=0.05)
    xi, xt = emb_i.cpu().double(), emb_t.cpu().double()
    first = None
    for _ in range(5):
        for o in (opt, opt_loss, opt_d, opt_dP):
            o.zero_grad()
        hi, ht = model.hash(emb_i, emb_t)
        loss, loss_dict = model.object_function(hi, ht, labels.cuda())
        loss.backward()
        codes = []
        for s, x in enumerate((xi, xt)):
            keep = (torch.rand(B, K, device="cuda", generator=twin[s]) >= 0.2).cpu().double()
            codes.append(torch.tanh(torch.nn.functional.linear(x, d[2 * s], d[2 * s + 1]) * keep / 0.8))
        want = hyp_terms(codes[0], codes[1], dP, labels, 0.25, 0.8)["loss"]
        want.backward()
        print("dsph step loss %.8f want %.8f" % (float(loss), float(want)))
        assert abs(float(loss) - float(want)) <= 5e-5 * abs(float(want)) + 1e-6
        first = float(loss) if first is None else first
        opt.step()
        opt_loss.step()
        opt_d.step()
        opt_dP.step()
    assert float(loss) != first
    for p, q in zip(params + [model.hyp.proxies], d + [dP]):                     # each figure before any assertion
        print("dsph %s |p - f64| %.2e  max|f64| %.2e" % (tuple(p.shape), float((p.detach().cpu().double() - q.detach()).abs().max()),
                                                         float(q.detach().abs().max())))
    for p, q in zip(params + [model.hyp.proxies], d + [dP]):
        assert float((p.detach().cpu().double() - q.detach()).abs().max()) <= 5e-5 * max(1.0, float(q.detach().abs().max()))
    assert all(torch.equal(a, b) for a, b in zip(backbone, model.backbone.parameters()))
    lines = []
    trainer.logger, trainer.optimizer = types.SimpleNamespace(info=lines.append), opt
    trainer.print_loss_dict(loss_dict, bits=K, epoch=0, times=1)
    assert len(lines) == 1 and lines[0].endswith("lr: %.9f" % BC.lr_f64(OPT_HYPER, 5))


# 10 --------------------------------------------------------------------------------------------------------------------------
def test_unsupported_parameters_raise_with_their_index():
    from xmh.optim import BertAdam
    good = torch.nn.Parameter(torch.zeros(8, device="cuda"))
    good.grad = torch.ones(8, device="cuda")
    cpu = torch.nn.Parameter(torch.zeros(8))
    cpu.grad = torch.ones(8)
    half = torch.nn.Parameter(torch.zeros(8, device="cuda", dtype=torch.float16))
    half.grad = torch.ones(8, device="cuda", dtype=torch.float16)
    strided = torch.nn.Parameter(torch.zeros(8, 6, device="cuda").t())
    strided.grad = torch.ones(8, 6, device="cuda").t()
    assert not strided.is_contiguous()
    badgrad = torch.nn.Parameter(torch.zeros(6, 8, device="cuda"))
    badgrad.grad = torch.ones(8, 6, device="cuda").t()
    for bad, word in ((cpu, "cpu"), (half, "float16"), (strided, "contiguous"), (badgrad, "gradient")):
        opt = BertAdam([good, bad], lr=0.1)
        with pytest.raises(RuntimeError, match="parameter 1") as e:
            opt.step()
        assert word in str(e.value)
        assert not good.detach().any() and len(opt.state[bad]) == 0             # nothing ran
    empty = torch.nn.Parameter(torch.zeros(0, device="cuda"))
    empty.grad = torch.zeros(0, device="cuda")
    opt = BertAdam([empty, good], lr=0.1, max_grad_norm=-1, weight_decay=0.0)
    opt.step()                                                                   # zero-element parameters are skipped
    assert len(opt.state[empty]) == 0 and opt.state[good]["step"] == 1 and bool((good.detach() < 0).all())
