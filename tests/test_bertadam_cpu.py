"""BertAdam without a GPU: the float64 restatement of tests/bertadam_cases.py (which the GPU tests lean on) reproduces the
reference's own fp64 trajectories of tests/golden/bertadam.npz; the schedule functions and get_lr() equal the golden's; registry,
constructor errors, state keys; argument errors of the C entry; build_optimizer of the DCMHT and DSPH runners on stand-in models
(the runners themselves put their model on the GPU, so their construction is covered by tests/test_gpu_bertadam.py)."""
import ctypes
import logging

import numpy as np
import pytest
import torch

import bertadam_cases as BC

STORED = [c for c, spec in BC.CASES.items() if spec.get("stored", True)]


@pytest.mark.parametrize("case", STORED)
def test_float64_restatement_reproduces_the_reference(case):
    vals, lrs = BC.unpack(case)
    tensors, steps, nan = BC.resolve(case)
    own = BC.run_f64(case)
    seen = 0
    for s in range(steps):
        assert [(-1 if c is None else c) for c in own[s]["count"]] == lrs[s][1]
        assert np.allclose(own[s]["lr"], lrs[s][0], rtol=1e-15, atol=0) and len(own[s]["lr"]) == len(lrs[s][0])
        for t in range(len(tensors)):
            for kind in BC.KINDS:
                got = own[s][kind][t]
                assert (got is None) == ((s, t, kind) not in vals), (s, t, kind)
                if got is None:
                    continue
                want = vals[(s, t, kind)][0]
                if BC.poisoned(nan, s, t, kind):                                 # NaN norm -> NaN coef -> the whole tensor
                    assert np.isnan(want).all() and np.isnan(got).all(), (s, t, kind)
                else:
                    assert np.isfinite(want).all()
                    assert BC.rel_err(BC.thin(got), want) <= 1e-12, (s, t, kind)
                seen += 1
    assert seen == len(vals)


def test_first_step_of_a_warmup_does_not_move_the_parameters():
    vals, lrs = BC.unpack("cosine")
    tensors, _, _ = BC.resolve("cosine")
    for t, spec in enumerate(tensors):
        p0 = BC.draw_param("cosine", t, spec["shape"])
        assert np.array_equal(vals[(0, t, "p")][1], BC.thin(p0)) and np.array_equal(vals[(0, t, "p")][0], BC.thin(p0).astype(np.float64))
        assert np.abs(vals[(0, t, "m")][0]).max() > 0                            # the moments did move
    assert lrs[0][0][0] > 0                                                      # get_lr() after the step: the next step's rate


def test_schedules_and_get_lr_equal_the_goldens():
    import xmh  # noqa: F401
    from xmh.optim import SCHEDULES, BertAdam
    assert sorted(SCHEDULES) == ["warmup_constant", "warmup_cosine", "warmup_linear"]
    for name, f in SCHEDULES.items():
        for x in (0.0, 0.001, 0.05, 0.1, 0.5, 0.999, 1.0, 1.7):
            for w in (0.002, 0.1, 0.3):
                assert f(x, w) == BC.schedule_f64(name, x, w), (name, x, w)
        assert f(0.001) == 0.5                                                   # the default warmup is 0.002
    for case in STORED:                                                          # get_lr() from the stored counters: no step() needed
        tensors, steps, _ = BC.resolve(case)
        _, lrs = BC.unpack(case)
        params = [torch.nn.Parameter(torch.zeros(s["shape"])) for s in tensors]
        groups = [dict(params=[params[t] for t, s in enumerate(tensors) if s["group"] == gi],
                       **next(s["hyper"] for s in tensors if s["group"] == gi)) for gi in sorted({s["group"] for s in tensors})]
        opt = BertAdam(groups, lr=BC.DEFAULTS["lr"])
        for s in range(steps):
            for t, p in enumerate(params):
                p.grad = None if s in tensors[t]["none"] else torch.zeros_like(p)
                if lrs[s][1][t] >= 0:
                    opt.state[p].update(step=int(lrs[s][1][t]), next_m=torch.zeros_like(p), next_v=torch.zeros_like(p))
            assert opt.get_lr() == lrs[s][0], (case, s)


def test_registry_constructor_errors_and_state_keys():
    import xmh  # noqa: F401
    from xmh.common.register import registry
    from xmh.optim import BertAdam
    assert registry.get_optimizer_class("BertAdam") is BertAdam and issubclass(BertAdam, torch.optim.Optimizer)
    p = torch.nn.Parameter(torch.zeros(3))
    for bad in (dict(lr=-1.0), dict(lr=0.1, schedule="nope"), dict(lr=0.1, warmup=1.0), dict(lr=0.1, warmup=-0.5), dict(lr=0.1, b1=1.0),
                dict(lr=0.1, b2=-0.1), dict(lr=0.1, e=-1e-6)):
        with pytest.raises(ValueError):
            BertAdam([p], **bad)
    with pytest.raises(ValueError):
        BertAdam([p])                                                            # lr is required
    opt = BertAdam([p], lr=0.1)
    g = opt.param_groups[0]
    assert {k: g[k] for k in g if k != "params"}.items() >= dict(lr=0.1, warmup=-1, t_total=-1, schedule="warmup_linear", b1=0.9, b2=0.999,
                                                                 e=1e-6, weight_decay=0.01, max_grad_norm=1.0).items()
    assert opt.get_lr() == []                                                    # no grad anywhere
    p.grad = torch.ones(3)
    assert opt.get_lr() == [0]                                                   # a grad, no state yet
    with pytest.raises(RuntimeError, match="parameter 0"):
        opt.step()                                                               # a CPU parameter: no fallback
    assert len(opt.state[p]) == 0
    # a state dict of the reference's layout loads, and round-trips
    sd = {"state": {0: {"step": 4, "next_m": torch.full((3,), 2.0), "next_v": torch.full((3,), 3.0)}},
          "param_groups": [dict(opt.state_dict()["param_groups"][0])]}
    opt.load_state_dict(sd)
    assert set(opt.state[p]) == {"step", "next_m", "next_v"} and opt.state[p]["step"] == 4
    again = BertAdam([p], lr=0.5)
    again.load_state_dict(opt.state_dict())
    assert again.state[p]["step"] == 4 and torch.equal(again.state[p]["next_v"], torch.full((3,), 3.0)) and again.param_groups[0]["lr"] == 0.1
    assert again.get_lr() == [0.1]


def test_c_entry_reports_argument_errors_without_a_gpu():
    from oracle.fixtures import aligned_host
    from xmh import _lib
    lib = _lib.lib
    chunk = lib.xmh_bertadam_chunk()
    assert chunk > 0 and chunk % 4 == 0
    assert lib.xmh_bertadam_ws_bytes(3, 5) >= 5 * 8 and lib.xmh_bertadam_ws_bytes(3, 5) % 256 == 0
    assert lib.xmh_bertadam_ws_bytes(-1, 5) == 0 and lib.xmh_bertadam_ws_bytes(1, -5) == 0
    buf, ws = aligned_host(4096)
    tab, tabp = aligned_host(4096)
    assert lib.xmh_bertadam_step(None, 0, None, 0, None, 0, None) == 0           # nothing to do
    for args in ((None, 1, tabp, 1, ws, 4096), (tabp, 1, None, 1, ws, 4096), (tabp, 1, tabp, 1, None, 4096), (tabp, -1, tabp, 1, ws, 4096),
                 (tabp, 1, tabp, -1, ws, 4096), (tabp, 2, tabp, 1, ws, 4096), (tabp, 1, tabp, 1, ws, 0),
                 (tabp, 1, tabp, 1, ctypes.c_void_p(ws.value + 8), 2048)):
        assert lib.xmh_bertadam_step(*args, None) == -22, args
        assert b"xmh_bertadam_step" in lib.xmh_last_error()
    from xmh.optim import CHUNK_DTYPE, TENSOR_DTYPE
    assert TENSOR_DTYPE.itemsize == 72 and CHUNK_DTYPE.itemsize == 16
    del buf, tab


class _Stub:
    """what build_optimizer reads of a runner"""

    def __init__(self, runner_cls, model, loader_len, epochs):
        self.model, self.epochs, self.logger = model, epochs, logging.getLogger("bertadam-test")
        self.train_loader = None if loader_len is None else [0] * loader_len
        self._cls = runner_cls

    def build(self, cfg, parameters=None):
        return self._cls.build_optimizer(self, cfg, parameters)


class _Model(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.backbone, self.hash, self.hyp = torch.nn.Linear(4, 3), torch.nn.Linear(3, 2), torch.nn.Linear(2, 2, bias=False)


# the runners' classes need the package's own `super()` chain: bind the stub's class under them
def _runner(base):
    import xmh.runners  # noqa: F401
    from xmh.common.register import registry
    cls = registry.get_runner_class(base)
    stub_cls = type("Stub" + base, (cls,), {"__init__": lambda self, model, n, epochs: _Stub.__init__(self, cls, model, n, epochs)})
    return stub_cls


def test_build_optimizer_of_the_dcmht_and_dsph_runners():
    from xmh.optim import BertAdam
    from xmh.utils.config import Config
    model = _Model()
    r = _runner("DCMHTTrainer")(model, 7, 3)
    opt, sched = r.build_optimizer(Config({}))
    assert type(opt) is BertAdam and sched is None
    g0, g1 = opt.param_groups
    assert [id(p) for p in g0["params"]] == [id(p) for p in model.backbone.parameters()] and g0["lr"] == 0.00001
    assert [id(p) for p in g1["params"]] == [id(p) for p in model.hash.parameters()] and g1["lr"] == 0.001
    for g in (g0, g1):
        assert (g["warmup"], g["schedule"], g["b1"], g["b2"], g["e"], g["max_grad_norm"], g["weight_decay"], g["t_total"]) == \
            (0.1, "warmup_cosine", 0.9, 0.98, 0.000001, 1.0, 0.2, 21)
    opt, _ = r.build_optimizer(Config({"arch": "BertAdam", "lr": 0.01, "backbone_lr": 0.002, "warmup_proportion": 0.05, "schedule": "warmup_linear",
                                       "b2": 0.999, "weight_decay": 0.0, "max_grad_norm": -1}))
    assert [g["lr"] for g in opt.param_groups] == [0.002, 0.01] and opt.param_groups[1]["schedule"] == "warmup_linear"
    assert opt.param_groups[0]["max_grad_norm"] == -1 and opt.param_groups[0]["warmup"] == 0.05
    opt, _ = r.build_optimizer(Config({"lr": 0.5}), parameters=[{"params": list(model.hyp.parameters())}])
    assert len(opt.param_groups) == 1 and opt.param_groups[0]["lr"] == 0.5
    with pytest.raises(NotImplementedError, match="not registered"):
        r.build_optimizer(Config({"arch": "Lion"}))
    with pytest.raises(RuntimeError, match="training loader"):
        _runner("DCMHTTrainer")(model, None, 3).build_optimizer(Config({}))
    d = _runner("DSPHTrainer")(model, 5, 2)
    opt, opt_loss, sched = d.build_optimizer(Config({"hyp": {"lr": 0.03}}))
    assert type(opt) is BertAdam and sched is None and opt.param_groups[0]["t_total"] == 10
    assert type(opt_loss) is torch.optim.SGD and [id(p) for p in opt_loss.param_groups[0]["params"]] == [id(p) for p in model.hyp.parameters()]
    assert (opt_loss.param_groups[0]["lr"], opt_loss.param_groups[0]["momentum"], opt_loss.param_groups[0]["weight_decay"]) == (0.03, 0.9, 0.0005)
    _, opt_loss, _ = d.build_optimizer(Config({}))
    assert opt_loss.param_groups[0]["lr"] == 0.02


def test_train_epoch_no_longer_lists_the_optimiser_as_missing():
    from xmh.runners.base import BaseTrainer
    with pytest.raises(NotImplementedError) as e:
        BaseTrainer.train_epoch(None, 0)
    assert "BertAdam optimiser, are still missing" not in str(e.value) and "towers" in str(e.value)
