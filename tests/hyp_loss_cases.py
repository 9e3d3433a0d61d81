"""Shared by tests/test_hyp_loss_cases_cpu.py and tests/test_gpu_hyp_loss_f64.py (not a test module): DSPH's HyP loss (reference
models/DSPH/loss/HyP.py:18-70) restated in a chosen dtype, the cases of the GPU module with their seeded inputs, the conditions those
inputs must meet, and the error measure with its yardstick.

The restatement.  `restate` runs oracle.losses.hyp_terms (which keeps the dtype it is handed) and its backward on one CPU thread:
float64 is the oracle, float32 is the yardstick's e_ref (what the reference's own expression loses at that shape).

Inputs.  One base pattern b = randn(K) per case.  Codes x_i = tanh(1.5 (s_i b + randn)) with s_i ~ U(0, 1.5), y likewise with its own
s_i; proxies P_c = (t_c b + randn) sqrt(2 / C) with t_c ~ U(-0.3, 1.2).  The shared pattern spreads the cosines over both sides of the
thresholds the reference uses (plain randn codes do not: at K = 257 a cosine of 0.25 is four sigma out).  Labels are Bernoulli(p) plus
one forced class per row; the rows a case names are then overwritten.

Conditions (on the inputs, not measurements of the port).  The five mask families are cos = n(x) n(P)^T and cos_t = n(y) n(P)^T over
the (row, proxy) entries without a label, and xx, yy, xy = n(x) n(x)^T, n(y) n(y)^T, n(x) n(y)^T over the ordered pairs of M x M with
disjoint label sets.  The gradient jumps where such an entry crosses the threshold, so an entry that fp32 puts on the other side is
another function, not a rounding error: every entry keeps GAP = 2e-5 (about 100 x the fp32 rounding of a normalised dot product)
from the threshold in float64; rows that do not are redrawn from the case's generator.  The masks of the float32 restatement equal
the float64 ones entry for entry.  There is therefore no allowance for flipped masks anywhere in these tests.

Error measure.  rel_err = max|got - fp64| / max|fp64| per kind (the eight terms as one vector, each gradient).  Rows clamped by
F.normalize's eps (row norm < 1e-12: their gradient is du / eps, 1e12 times the others) form a group of their own inside their
tensor, the split of oracle.fixtures.grads_close_rows; a kind's error is the larger of its groups'.  The yardstick per kind is
max(pool, e_ref): pool = the reference's own fp32 numbers of tests/golden/loss_dsph.npz against the float64 restatement over the seven
golden cases, e_ref = the float32 restatement against the float64 one at the case's own inputs.  At K = 1 the gradients vanish
identically and max|fp64| is rounding residue; there the errors are divided by cancel_scale (see there) instead.

Two places where the table of cases cannot hold as first written.  A pair of M x M needs two rows with two labels each and no class
in common, hence four classes: at C = 3 (b40_k1_c3) Z is 0 whatever the labels are, so that case runs K = 1 through the Z == 0 branch
and b40_k1_c4 runs K = 1 with Z > 0 and reg > 0.  The non-finite cases need three pairwise disjoint rows of M (six classes) and a class
no row carries: C = 7."""
import contextlib

import numpy as np
import torch
import torch.nn.functional as F

from oracle import losses as OL

TERMS = OL.HYP_TERMS
KINDS = ("terms", "g_x", "g_y", "g_P")
FAMILIES = ("cos", "cos_t", "xx", "yy", "xy")
SEED = 1814
ALPHA = 0.8
GAP = 2e-5
EPS = 1e-12                          # F.normalize's eps

# name -> B, K, C, threshold, p of the Bernoulli labels, share = what the active share of each of the five masks must be ("both": in
# [0.05, 0.95], "most": >= 0.9, "none": exactly 0, None: not asked), no_class = a class that no row carries, and the rows the case
# names (see _named / check_conditions)
CASES = {
    "b257_k16_c21": dict(B=257, K=16, C=21, thr=0.25, p=0.08, share="both", set_labels={256: (3, 17)}),
    "b300_k65_c33": dict(B=300, K=65, C=33, thr=0.0, p=0.05, share="both", copy_y=(7, 130),
                         set_labels={11: (), 7: (0, 1), 130: (2, 3), 20: (4, 32), 21: (5, 32)}),
    "b513_k257_c65": dict(B=513, K=257, C=65, thr=0.25, p=0.03, share="both", set_labels={512: (1, 64)}),
    "b40_k1_c3": dict(B=40, K=1, C=3, thr=0.25, p=0.3, share=None, z_zero=True),
    "b40_k1_c4": dict(B=40, K=1, C=4, thr=0.25, p=0.3, share=None, set_labels={0: (0, 1), 1: (2, 3), 2: (0, 2), 3: (1, 3)}),
    "b64_k4096_c32": dict(B=64, K=4096, C=32, thr=0.1, p=0.08, share="both", set_labels={0: (0, 31), 5: (7, 31), 9: (31,)}),
    "b33_k100_c1024": dict(B=33, K=100, C=1024, thr=-0.2, p=0.003, share="most"),
    "b1_k16_c2": dict(B=1, K=16, C=2, thr=0.25, p=0.0, share=None, z_zero=True, set_labels={0: (0,)}),
    "b48_k63_c5_off": dict(B=48, K=63, C=5, thr=1.0, p=0.2, share="none", no_class=4, set_labels={0: (0, 1), 1: (2, 3)}),
    "b96_k64_c24_clamped": dict(B=96, K=64, C=24, thr=0.25, p=0.08, share=None, zero_x=5, tiny_y=(9, 3e-13), zero_P=2,
                                set_labels={20: ()}),
}

# B = 6, K = 4, C = 7.  The rows of M are 0, 1, 3, pairwise disjoint; rows 2, 4, 5 carry one label each; no row carries class 5.
# Recorded from the float32 restatement on the CPU (tests/test_hyp_loss_cases_cpu.py asserts that they still match it): the terms that
# are NaN, and per gradient the rows that are NaN (a row is either NaN throughout or finite throughout).
NONFINITE_B, NONFINITE_K, NONFINITE_C, NONFINITE_THR = 6, 4, 7, 0.25
NONFINITE_LABELS = ((0, 1), (2, 3), (0,), (4, 6), (2,), (4,))
_CODE_IN_M = dict(nan_terms=("loss", "pos", "neg", "reg", "reg_xt"), g_x=(0, 1, 3), g_y=(0, 1, 3), g_P=(0, 1, 2, 3, 4, 5, 6))
NONFINITE = {
    "nan_unused_proxy": dict(poke="P[5, 1] = nan", nan_terms=("loss", "neg", "neg_t"), g_x=(0, 1, 2, 3, 4, 5), g_y=(0, 1, 2, 3, 4, 5),
                             g_P=(5,)),
    "nan_code_in_M": dict(poke="x[0, 2] = nan", **_CODE_IN_M),
    "inf_code_in_M": dict(poke="x[1] = inf", **_CODE_IN_M),
    # 1 / norm = 0 makes the weight of a label -0: rows 1 and 4 carry class 2, and row 2 carries class 0
    "inf_used_proxy": dict(poke="P[2, 1] = inf", nan_terms=("loss", "pos", "neg", "pos_t", "neg_t"), g_x=(0, 1, 2, 3, 4, 5),
                           g_y=(0, 1, 2, 3, 4, 5), g_P=(2,)),
    "inf_both_codes": dict(poke="x[2] = y[2] = inf", nan_terms=("loss", "pos", "neg", "pos_t", "neg_t"), g_x=(2,), g_y=(2,),
                           g_P=(0, 1, 2, 3, 4, 5, 6)),
}


# ---- the restatement ----------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


def restate(x, y, P, labels, threshold, alpha, dtype=torch.float64):
    """x, y [B, K], P [C, K] (any float dtype, taken to `dtype`), labels [B, C] 0/1 -> dict(terms [8] in TERMS order, g_x, g_y, g_P) as
    float64 numpy: the terms and the gradients of the loss as oracle.losses.hyp_terms gives them when evaluated in `dtype`"""
    a, b, p = (torch.as_tensor(v).detach().to(dtype).clone().requires_grad_(True) for v in (x, y, P))
    with one_thread():
        t = OL.hyp_terms(a, b, p, torch.as_tensor(labels), threshold, alpha)
        assert all(v.dtype == dtype for v in t.values())
        t["loss"].backward()
    return {"terms": np.array([float(t[k].detach()) for k in TERMS], dtype=np.float64), "g_x": a.grad.double().numpy(),
            "g_y": b.grad.double().numpy(), "g_P": p.grad.double().numpy()}


# ---- error measure and yardstick ----------------------------------------------------------------------------------------------
def rel_err(x, ref, floor=None):
    """floor [rows]: the least scale the error of each row is divided by (K = 1 alone, see cancel_scale)"""
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if floor is None:
        return float(np.abs(x - ref).max()) / (float(np.abs(ref).max()) or 1.0)
    return float((np.abs(x - ref).max(axis=1) / np.maximum(np.abs(ref).max(), floor)).max())


def clamped_rows(x, y, P):
    """per gradient, the rows whose input norm lies below F.normalize's eps (bool numpy)"""
    return {k: (torch.as_tensor(v).double().norm(dim=1) < EPS).numpy() for k, v in (("g_x", x), ("g_y", y), ("g_P", P))}


def errors(got, ref, clamped, floor=None):
    """floor: {gradient: per row, the least scale its error is divided by}, for K = 1 alone (see cancel_scale)"""
    e = {"terms": rel_err(got["terms"], ref["terms"])}
    for k in KINDS[1:]:
        e[k] = max(rel_err(got[k][rows], ref[k][rows], floor[k][rows] if floor else None) for rows in (clamped[k], ~clamped[k]) if rows.any())
    return e


def cancel_scale(x, y, P, labels, alpha):
    """K = 1 alone.  n(v) = +-1 whatever v is, so every gradient is exactly zero: float64 returns its own rounding residue (1e-17),
    and an error divided by that measures nothing.  The gradient of a row is (du - u (u . du)) / |v|, the difference of two equal
    terms; the error of each row of the K = 1 cases is taken relative to the size of that row's terms instead: |du| / |v| with |du| bounded by the
    sum of the row's |d loss / d cos| (1 / P_num on a label, 1 / N_num off it; every proxy and code is a unit vector) and, for a row
    of M, 3 alpha / Z per disjoint partner (x-x counted twice, x-y once)."""
    L = (torch.as_tensor(labels) != 0).double()
    B, C = L.shape
    pn, nn = float(L.sum()), float(B * C - L.sum())
    w = L / pn + ((1 - L) / nn if nn else 0.0)
    pairs = pairs_of(labels)[1].double()
    du = w.sum(1) + (3 * alpha * pairs.sum(1) / float(pairs.sum()) if pairs.any() else 0.0)
    inv = lambda v: 1.0 / torch.as_tensor(v).double().norm(dim=1).clamp_min(EPS)       # noqa: E731
    return {"g_x": (du * inv(x)).numpy(), "g_y": (du * inv(y)).numpy(), "g_P": (w.sum(0) * inv(P)).numpy()}


_pool = None


def golden_pool():
    """per kind: the largest error of the reference's own fp32 run (the golden file) against the float64 restatement.  The file keeps
    the loss alone of the eight terms; it is the largest of them, so its error is measured as the terms' is."""
    global _pool
    if _pool is None:
        worst = {k: 0.0 for k in KINDS}
        for name in OL.HYP_CASES:
            x, y, P, labels, threshold, alpha, loss, (gx, gy, gP) = OL.load_hyp(name)
            labels = np.eye(x.shape[0]) if labels is None else labels
            ref = restate(x, y, P, labels, threshold, alpha)
            got = {"terms": np.array([loss]), "g_x": gx, "g_y": gy, "g_P": gP}
            e = errors(got, dict(ref, terms=ref["terms"][:1]), clamped_rows(x, y, P))
            worst = {k: max(worst[k], e[k]) for k in KINDS}
        _pool = worst
    return dict(_pool)


def yardstick(e_ref):
    pool = golden_pool()
    return {k: max(pool[k], e_ref[k]) for k in KINDS}


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def _gen(name):
    return torch.Generator().manual_seed(SEED * 1000 + sorted(list(CASES) + list(NONFINITE)).index(name))


def _code_rows(g, n, base):
    return torch.tanh(1.5 * (1.5 * torch.rand(n, 1, generator=g) * base + torch.randn(n, base.numel(), generator=g)))


def _proxies(g, C, base):
    t = 1.5 * torch.rand(C, 1, generator=g) - 0.3
    return (t * base + torch.randn(C, base.numel(), generator=g)) * (2.0 / C) ** 0.5


def _labels(g, B, C, p, set_labels=None, no_class=None):
    L = (torch.rand(B, C, generator=g) < p).float()
    L[torch.arange(B), torch.randint(0, C - (no_class is not None), (B,), generator=g)] = 1.0
    if no_class is not None:
        assert no_class == C - 1
        L[:, no_class] = 0.0
    for row, classes in (set_labels or {}).items():
        L[row] = 0.0
        L[row, list(classes)] = 1.0
    return L


def _named(spec, x, y, P):
    """the rows a case names, applied to copies of the drawn tensors"""
    x, y, P = x.clone(), y.clone(), P.clone()
    if "copy_y" in spec:
        y[spec["copy_y"][1]] = y[spec["copy_y"][0]]
    if "zero_x" in spec:
        x[spec["zero_x"]] = 0.0
    if "tiny_y" in spec:
        r, norm = spec["tiny_y"]
        y[r] = y[r] * (norm / float(y[r].double().norm()))
    if "zero_P" in spec:
        P[spec["zero_P"]] = 0.0
    return x, y, P


def pairs_of(labels):
    """-> (M [B] bool, pairs [B, B] bool: both rows in M and no class in common; ordered, as the reference counts Z)"""
    L = (torch.as_tensor(labels) != 0).double()
    M = L.sum(1) > 1
    return M, M[:, None] & M[None, :] & ((L @ L.T) == 0)


def families(x, y, P, labels, dtype=torch.float64):
    """-> {family: (values, valid)}: the similarities that decide a mask, evaluated in `dtype` as the reference does (F.normalize and
    a matrix product), and the entries that enter the loss through a relu"""
    with one_thread():
        nx, ny, nP = (F.normalize(torch.as_tensor(v).to(dtype), p=2, dim=1) for v in (x, y, P))
        off = torch.as_tensor(labels) == 0
        pairs = pairs_of(labels)[1]
        return {"cos": (nx @ nP.T, off), "cos_t": (ny @ nP.T, off), "xx": (nx @ nx.T, pairs), "yy": (ny @ ny.T, pairs),
                "xy": (nx @ ny.T, pairs)}


def _too_close(x, y, P, labels, thr):
    """-> (bad_x [B], bad_y [B], count): rows with a mask entry within GAP of the threshold; xy entries count against their x row"""
    f = families(x, y, P, labels)
    near = {k: ((v - thr).abs() < GAP) & valid for k, (v, valid) in f.items()}
    bad_x = near["cos"].any(1) | near["xx"].any(1) | near["xy"].any(1)
    bad_y = near["cos_t"].any(1) | near["yy"].any(1)
    return bad_x, bad_y, sum(int(v.sum()) for v in near.values())


_built = {}


def build(name):
    """-> dict(spec, x, y [B, K], P [C, K] fp32, labels [B, C] fp32, redrawn = mask entries that lay within GAP of the threshold before
    rows were redrawn, floor = cancel_scale at K = 1, else None); the same tensors at every call"""
    if name not in _built:
        spec, g = CASES[name], _gen(name)
        B, K, C = spec["B"], spec["K"], spec["C"]
        base = torch.randn(K, generator=g)
        x0, y0, P0 = _code_rows(g, B, base), _code_rows(g, B, base), _proxies(g, C, base)
        labels = _labels(g, B, C, spec["p"], spec.get("set_labels"), spec.get("no_class"))
        first = None
        for _ in range(200):
            x, y, P = _named(spec, x0, y0, P0)
            bad_x, bad_y, n = _too_close(x, y, P, labels, spec["thr"])
            first = n if first is None else first
            if n == 0:
                break
            if "copy_y" in spec and bad_y[spec["copy_y"][1]]:
                bad_y[spec["copy_y"][0]] = True                    # the copy follows its source
            for rows, t in ((bad_x, x0), (bad_y, y0)):
                idx = torch.nonzero(rows).flatten()
                if idx.numel():
                    t[idx] = _code_rows(g, idx.numel(), base)
        else:
            raise AssertionError("%s: no draw keeps every mask entry %g away from the threshold" % (name, GAP))
        _built[name] = dict(spec, name=name, x=x, y=y, P=P, labels=labels, redrawn=first,
                            floor=cancel_scale(x, y, P, labels, ALPHA) if K == 1 else None)
    return _built[name]


def build_nonfinite(name):
    """-> (x, y [6, 4], P [7, 4] fp32 with the poke applied, labels [6, 7], threshold, alpha)"""
    g = _gen(name)
    base = torch.randn(NONFINITE_K, generator=g)
    x, y = _code_rows(g, NONFINITE_B, base), _code_rows(g, NONFINITE_B, base)
    P = _proxies(g, NONFINITE_C, base)
    labels = _labels(g, NONFINITE_B, NONFINITE_C, 0.0, dict(enumerate(NONFINITE_LABELS)))
    if name == "nan_unused_proxy":
        P[5, 1] = float("nan")
    elif name == "nan_code_in_M":
        x[0, 2] = float("nan")
    elif name == "inf_code_in_M":
        x[1] = float("inf")
    elif name == "inf_used_proxy":
        P[2, 1] = float("inf")
    else:
        x[2] = y[2] = float("inf")
    return x, y, P, labels, NONFINITE_THR, ALPHA


def nan_pattern(r):
    """-> (names of the NaN terms, {gradient: NaN rows}) of a result of restate or of the port; a gradient row is NaN throughout or not
    at all (asserted)"""
    rows = {}
    for k in KINDS[1:]:
        bad = np.isnan(r[k])
        assert np.array_equal(bad.any(1), bad.all(1)) and not np.isinf(r[k]).any(), (k, bad)
        rows[k] = tuple(int(i) for i in np.nonzero(bad.all(1))[0])
    assert not np.isinf(r["terms"]).any()
    return tuple(t for t, v in zip(TERMS, r["terms"]) if np.isnan(v)), rows


# ---- the conditions on the inputs ---------------------------------------------------------------------------------------------
def measure(c):
    """what the conditions are about, from float64 on the CPU: per mask family the number of entries, the smallest distance from the
    threshold and the active share; Z, and the number of entries where the float32 masks differ from the float64 ones"""
    f64 = families(c["x"], c["y"], c["P"], c["labels"])
    f32 = families(c["x"], c["y"], c["P"], c["labels"], dtype=torch.float32)
    out = {"Z": int(pairs_of(c["labels"])[1].sum()), "fp32_mask_differs": 0}
    for k in FAMILIES:
        v, valid = f64[k]
        n = int(valid.sum())
        out["fp32_mask_differs"] += int((((v > c["thr"]) != (f32[k][0] > c["thr"])) & valid).sum())
        out[k] = dict(n=n, gap=float((v - c["thr"]).abs()[valid].min()) if n else float("inf"),
                      active=float((v > c["thr"])[valid].double().mean()) if n else float("nan"))
    return out


def check_conditions(name):
    """asserts what the case promises of its inputs and returns the measurements; called by the CPU test, and by the GPU test before
    it compares anything"""
    c = build(name)
    x, y, P, L = c["x"], c["y"], c["P"], c["labels"]
    B, K, C = c["B"], c["K"], c["C"]
    assert x.shape == y.shape == (B, K) and P.shape == (C, K) and L.shape == (B, C)
    assert all(t.dtype == torch.float32 and bool(torch.isfinite(t).all()) for t in (x, y, P, L))
    assert bool(((L == 0) | (L == 1)).all())
    m = measure(c)
    assert K < 4096 or GAP >= 4 * K ** 0.5 * 2.0 ** -24
    for k in FAMILIES:
        assert m[k]["gap"] >= GAP, (name, k, m[k])
        if m[k]["n"] and c["share"] == "both":
            assert 0.05 <= m[k]["active"] <= 0.95, (name, k, m[k])
        if m[k]["n"] and c["share"] == "most":
            assert m[k]["active"] >= 0.9, (name, k, m[k])
        if c["share"] == "none":
            assert m[k]["n"] > 0 and m[k]["active"] == 0.0, (name, k, m[k])
    assert m["fp32_mask_differs"] == 0, (name, m)
    M, pairs = pairs_of(L)
    ref = restate(x, y, P, L, c["thr"], ALPHA)["terms"]
    reg = ref[5:]
    if c.get("z_zero"):                                   # fewer than four classes, or a single row: no pair can be disjoint
        assert m["Z"] == 0 and (C < 4 or B == 1) and (reg == 0).all()
    else:
        assert m["Z"] > 0 and all(m[k]["n"] == m["Z"] for k in ("xx", "yy", "xy"))
        assert (reg == 0).all() if c["share"] == "none" else (reg > 0).all(), (name, reg)
    if c["share"] == "none":
        assert ref[2] == 0 and ref[4] == 0 and ref[1] > 0 and ref[3] > 0
    if c.get("no_class") is not None:                     # a class no row carries: its proxy meets the hinge alone
        assert not L[:, c["no_class"]].any() and int((L != 0).any(0).sum()) == C - 1
    for row, classes in c.get("set_labels", {}).items():
        assert sorted(torch.nonzero(L[row]).flatten().tolist()) == sorted(classes), (name, row)
    _check_named(name, c, M, pairs)
    return m


def _check_named(name, c, M, pairs):
    x, y, P, L = c["x"], c["y"], c["P"], c["labels"]
    Lb = L != 0
    for last in range(255, c["B"], 256):                 # the last row of a full partner chunk is in M and has partners in every chunk
        assert bool(M[last]) and all(int(pairs[last, lo:lo + 256].sum()) > 0 for lo in range(0, c["B"], 256)), (name, last)
    if name == "b257_k16_c21":                            # the second partner chunk holds one row, and it takes part
        assert bool(M[256]) and int(pairs[256, :256].sum()) > 0 and int(pairs[:256, 256].sum()) > 0
    if name == "b300_k65_c33":
        assert not Lb[11].any()
        src, dst = c["copy_y"]
        assert torch.equal(y[src], y[dst]) and bool(pairs[src, dst])
        assert abs(float(families(x, y, P, L)["yy"][0][src, dst]) - 1.0) <= 2.0 ** -50        # sim 1: one rounding of the float64 product
        shared = Lb[:, None, :] & Lb[None, :, :]                     # [B, B, C]
        only32 = M[:, None] & M[None, :] & shared[:, :, 32] & ~shared[:, :, :32].any(-1)
        only32.fill_diagonal_(False)
        assert bool(only32.any())                                    # the only shared class lies in the second label word
        word0 = ~Lb[:, 32]
        assert bool((pairs & Lb[:, 32][:, None] & word0[None, :]).any())   # disjoint: one carries class 32, the other none of word 1
        assert int(pairs[256:, :256].sum()) > 0 and int(M[256:].sum()) > 1
    if name == "b513_k257_c65":
        assert all(int(M[lo:lo + 256].sum()) > 0 for lo in (0, 256, 512)) and bool(Lb[:, 64].any())
        assert int(pairs[512].sum()) > 0
    if name == "b64_k4096_c32":
        assert int(Lb[:, 31].sum()) >= 3 and bool((M & Lb[:, 31]).any()) and bool(pairs[Lb[:, 31] & M].any())
    if name == "b33_k100_c1024":
        assert bool(Lb[:, 992:].any()) and bool(Lb[:, 32:64].any())        # the last of the 32 label words is in use
    if name == "b96_k64_c24_clamped":
        assert not x[5].any() and not P[2].any() and not Lb[20].any()
        assert 0.0 < float(y[9].double().norm()) < EPS and bool(Lb[5].any()) and bool(Lb[:, 2].any())
        cl = clamped_rows(x, y, P)
        assert [int(v.sum()) for v in cl.values()] == [1, 1, 1]


def describe(m):
    head = "Z %d  fp32 masks differ at %d" % (m["Z"], m["fp32_mask_differs"])
    return head + "  " + "  ".join("%s[n %d gap %.3g active %.3f]" % (k, m[k]["n"], m[k]["gap"], m[k]["active"]) for k in FAMILIES)
