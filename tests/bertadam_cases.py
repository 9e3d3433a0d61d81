"""Shared by tools/make_golden_bertadam.py, tests/test_bertadam_cpu.py and tests/test_gpu_bertadam.py (not a test module): the
BertAdam cases (hyper-parameters, shapes, seeded parameters and gradients), a float64 restatement of the step written from its
formulas, and the error measure of the golden file.

A case is a list of parameter groups; tensor t of a case draws its initial value from rng(seed, 7, t) and its gradient of step s
from rng(seed, 1000 + s, t), scaled so that its L2 norm is about `norm` -- below, above or far above max_grad_norm.  `none`
lists the steps at which a tensor's grad is None, `nan` = (tensor, step, flat index) poisons one gradient entry.

Stored tensors of more than FULL elements keep every THIN-th flat element (`thin`); the error measure e = max|x - fp64| /
max|fp64| is always taken on whole tensors."""
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bertadam.npz")
KINDS = ("p", "m", "v", "grad")
FULL, THIN = 256, 16
SEED = 1814

DEFAULTS = dict(lr=1e-2, warmup=-1, t_total=-1, schedule="warmup_linear", b1=0.9, b2=0.999, e=1e-6, weight_decay=0.01, max_grad_norm=1.0)


def T(shape, norm=3.0, none=(), **kw):
    return dict(shape=shape if isinstance(shape, tuple) else (shape,), norm=norm, none=frozenset(none), **kw)


def G(tensors, **hyper):
    return dict(tensors=tensors, hyper=hyper)


# name -> dict(groups, steps, nan, stored).  "C" in a shape is the kernel's chunk length (resolved by `resolve`).
CASES = {
    # every shape of the issue, norms below / above / far above the clip in the same step
    "shapes": dict(steps=6, groups=[G([T(1, 0.3), T(3, 3.0), T(4, 300.0), T(5, 0.3), T(63, 3.0), T(64, 300.0), T(65, 0.3), T((257, 3), 3.0),
                                       T((1024, 5), 300.0), T(3000, 0.3)], t_total=20, warmup=0.1, schedule="warmup_cosine", b2=0.98,
                                      weight_decay=0.2)]),
    "cosine": dict(steps=6, groups=[G([T(5, 0.3), T(65, 3.0), T(3, 300.0)], t_total=10, warmup=0.3, schedule="warmup_cosine")]),
    "constant": dict(steps=6, groups=[G([T(5, 0.3), T(65, 3.0)], t_total=10, warmup=0.3, schedule="warmup_constant")]),
    "linear": dict(steps=6, groups=[G([T(5, 0.3), T(65, 3.0)], t_total=10, warmup=0.3, schedule="warmup_linear")]),
    "no_total": dict(steps=6, groups=[G([T(5, 0.3), T(65, 3.0)], t_total=-1, warmup=0.3)]),
    "two_groups": dict(steps=6, groups=[G([T(4, 3.0), T(63, 0.3)], lr=1e-5, t_total=12, warmup=0.1, schedule="warmup_cosine"),
                                        G([T(64, 3.0), T(5, 300.0)], lr=1e-3, t_total=12, warmup=0.1, schedule="warmup_cosine")]),
    "no_clip": dict(steps=6, groups=[G([T(5, 0.3), T(65, 300.0)], max_grad_norm=-1)]),
    "no_decay": dict(steps=6, groups=[G([T(5, 0.3), T(65, 3.0)], weight_decay=0.0)]),
    # step counters diverge: tensor 1 has no grad at steps 1, 2 and 4
    "skipped": dict(steps=7, groups=[G([T(5, 3.0), T(65, 3.0, none=(1, 2, 4)), T(3, 0.3, none=(0,))], t_total=10, warmup=0.3,
                                       schedule="warmup_linear")]),
    # the schedule runs out: steps 4.. lie past t_total (warmup_linear gives 0, the cosine goes on)
    "past_total": dict(steps=8, groups=[G([T(5, 3.0)], t_total=4, warmup=0.25, schedule="warmup_linear"),
                                        G([T(65, 0.3)], t_total=4, warmup=0.25, schedule="warmup_cosine")]),
    "nan": dict(steps=6, nan=(1, 2, 17), groups=[G([T(5, 3.0), T(65, 3.0), T(64, 0.3)], t_total=10, warmup=0.1)]),
    # chunk edges: only the error scalars are stored
    "large": dict(steps=6, stored=False, groups=[G([T("C-1", 3.0), T(1, 0.3), T("C+1", 300.0), T(65, 3.0), T("2C+7", 0.3)], t_total=20,
                                                  warmup=0.1, schedule="warmup_cosine", b2=0.98, weight_decay=0.2)]),
}


def resolve(case, chunk=None):
    """-> (list of per-tensor dicts with 'shape', 'norm', 'none', 'group', 'hyper'), steps, nan"""
    sym = {"C-1": lambda c: c - 1, "C+1": lambda c: c + 1, "2C+7": lambda c: 2 * c + 7}
    spec, out = CASES[case], []
    for gi, g in enumerate(spec["groups"]):
        hyper = dict(DEFAULTS, **g["hyper"])
        for t in g["tensors"]:
            shape = tuple(sym[d](chunk) if isinstance(d, str) else d for d in t["shape"])
            out.append(dict(shape=shape, norm=t["norm"], none=t["none"], group=gi, hyper=hyper))
    return out, spec["steps"], spec.get("nan")


def _rng(case, stream, t):
    return np.random.default_rng([SEED, sorted(CASES).index(case), stream, t])


def draw_param(case, t, shape):
    return (0.5 * _rng(case, 7, t).standard_normal(shape)).astype(np.float32)


def draw_grad(case, tensors, t, step, nan=None):
    """fp32 gradient of tensor t at `step`, or None"""
    spec = tensors[t]
    if step in spec["none"]:
        return None
    n = int(np.prod(spec["shape"]))
    g = (_rng(case, 1000 + step, t).standard_normal(spec["shape"]) * (spec["norm"] / math.sqrt(n))).astype(np.float32)
    if nan is not None and nan[0] == t and nan[1] == step:
        g.reshape(-1)[nan[2]] = np.nan
    return g


def poisoned(nan, step, t, kind):
    """is this tensor all NaN?  p, m and v from the poisoned step on; the gradient at that step only (later ones are fresh)"""
    return nan is not None and t == nan[0] and (step == nan[1] or (step > nan[1] and kind != "grad"))


# ---- the float64 restatement --------------------------------------------------------------------------------------------------
def schedule_f64(name, x, warmup):
    if x < warmup:
        return x / warmup
    if name == "warmup_cosine":
        return 0.5 * (1.0 + math.cos(math.pi * x))
    if name == "warmup_constant":
        return 1.0
    return max((x - 1.0) / (warmup - 1.0), 0)


def lr_f64(h, step):
    return h["lr"] * schedule_f64(h["schedule"], step / h["t_total"], h["warmup"]) if h["t_total"] != -1 else h["lr"]


def step_f64(p, g, m, v, lr, h):
    """one tensor, one step, numpy float64 -> (p, m, v, g')"""
    with np.errstate(all="ignore"):
        if h["max_grad_norm"] > 0:
            coef = h["max_grad_norm"] / (math.sqrt(float(np.sum(g * g))) + 1e-6) if not np.isnan(g).any() else float("nan")
            if not coef >= 1.0:
                g = g * coef
        m = m * h["b1"] + (1.0 - h["b1"]) * g
        v = v * h["b2"] + (1.0 - h["b2"]) * g * g
        u = m / (np.sqrt(v) + h["e"])
        if h["weight_decay"] > 0:
            u = u + h["weight_decay"] * p
        return p - lr * u, m, v, g


def run_f64(case, chunk=None, params=None, grads=None):
    """the whole trajectory: list over steps of dict(p, m, v, grad: per-tensor lists (None where the tensor has no state / no grad
    yet), lr: what get_lr() returns after the step, count: the step counters)"""
    tensors, steps, nan = resolve(case, chunk)
    p = [draw_param(case, t, s["shape"]).astype(np.float64) for t, s in enumerate(tensors)] if params is None else [x.astype(np.float64) for x in params]
    m, v, count, out = [None] * len(p), [None] * len(p), [None] * len(p), []
    for s in range(steps):
        post, lrs = [None] * len(p), []
        for t, spec in enumerate(tensors):
            g = draw_grad(case, tensors, t, s, nan) if grads is None else grads[s][t]
            if g is None:
                continue
            if count[t] is None:
                count[t], m[t], v[t] = 0, np.zeros_like(p[t]), np.zeros_like(p[t])
            p[t], m[t], v[t], post[t] = step_f64(p[t], g.astype(np.float64), m[t], v[t], lr_f64(spec["hyper"], count[t]), spec["hyper"])
            count[t] += 1
            lrs.append(lr_f64(spec["hyper"], count[t]))
        out.append(dict(p=list(p), m=list(m), v=list(v), grad=post, lr=lrs, count=list(count)))
    return out


# ---- error measure and storage ----------------------------------------------------------------------------------------------------
def rel_err(x, ref):
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(x - ref).max()) / (float(np.abs(ref).max()) or 1.0)


def thin(a):
    a = np.asarray(a).reshape(-1)
    return a if a.size <= FULL else a[::THIN]


def layout(case):
    """the (step, tensor, kind, stored size) of every tensor a stored case holds, in file order: p always, m and v once the tensor
    has had a gradient, grad where it has one at that step"""
    tensors, steps, _ = resolve(case)
    seen, out = set(), []
    for s in range(steps):
        for t, spec in enumerate(tensors):
            has = s not in spec["none"]
            if has:
                seen.add(t)
            n = int(np.prod(spec["shape"]))
            n = n if n <= FULL else len(range(0, n, THIN))
            for kind in KINDS:
                if kind == "p" or (kind == "grad" and has) or (kind in ("m", "v") and t in seen):
                    out.append((s, t, kind, n))
    return out


def pack(case, values):
    """values: (step, tensor, kind) -> (fp64 array, fp32 array), whole tensors -> the case's arrays of the golden file.  The fp32
    run is stored as its distance in units of the last place from the rounded fp64 value (int32: exact, compresses well)."""
    f64 = np.concatenate([thin(values[(s, t, k)][0]).astype(np.float64) for s, t, k, _ in layout(case)])
    f32 = np.concatenate([thin(values[(s, t, k)][1]).astype(np.float32) for s, t, k, _ in layout(case)])
    assert f64.size == sum(n for *_, n in layout(case))
    return {case + "__f64": f64, case + "__ulp": f32.view(np.int32) - f64.astype(np.float32).view(np.int32)}


_golden, _unpacked = None, {}


def golden():
    global _golden
    if _golden is None:
        _golden = dict(np.load(GOLDEN))
    return _golden


def unpack(case):
    """-> (step, tensor, kind) -> (fp64, fp32) thinned flat arrays of the reference's two runs; [step] -> (get_lr() list, counters)"""
    if case not in _unpacked:
        Gd, at, vals = golden(), 0, {}
        f64 = Gd[case + "__f64"]
        f32 = (f64.astype(np.float32).view(np.int32) + Gd[case + "__ulp"]).view(np.float32)
        for s, t, k, n in layout(case):
            vals[(s, t, k)] = (f64[at:at + n], f32[at:at + n])
            at += n
        assert at == f64.size
        tensors, steps, _ = resolve(case)
        lrs, lr_at = [], 0
        for s in range(steps):
            n = sum(1 for spec in tensors if s not in spec["none"])
            lrs.append((list(Gd[case + "__lr"][lr_at:lr_at + n]), list(Gd[case + "__count"][s])))
            lr_at += n
        _unpacked[case] = (vals, lrs)
    return _unpacked[case]
