"""Shared by tests/test_mith_loss_cases_cpu.py and tests/test_gpu_mith_loss_f64.py (not a test module): MITH's training objective
(reference models/MITH/MITH.py:116-232) restated in a chosen dtype, the cases of the GPU module with their seeded inputs, the
conditions those inputs must meet, and the error measure with its yardstick and comparison.

The restatement.  `restate` runs oracle.losses.mith_terms (which keeps the dtype it is handed) and its backward on one CPU thread:
float64 is the oracle, float32 is the yardstick's e_ref (what the reference's own expression loses at that shape).  Results are kept
per (case, weights, dtype), so the tests that need a reference share one.

Inputs (families).  soft: what tests/test_gpu_mith_loss.py draws (codes and buffer tanh(1.5 randn), normalised features).  trained: one
+-1 base pattern of K bits; every row of Y and of the four codes is the base with each bit flipped with a per-row probability
p ~ U(0, 1) (stratified over the B rows of a code), times magnitudes U(0.8, 1); at K >= 128 a large share of the dot products lies beyond the clamp at +-64.  pm1: exact +-1
codes and buffer; row q of code q is +-base and the buffer rows at the first and last row of every chunk are the base with a chosen
number of flips, so that Y.x = K - 2 flips is exactly +-64, +-62, +-66, 0 or +-K there, and S is chosen at those entries so that
S - sigma(s) is +-1 (the clamp mask alone decides whether that row's gradient passes).  raw: the codes of soft with unnormalised
1.5 randn features (logits in the hundreds, softmax rows nearly one-hot).  In every case the buffer rows `idx` hold tokens_hash_t, as
the buffer does after a step's row write.

Conditions (on the inputs, not measurements of the port), check_conditions.  The clamp and its mask jump at +-64, so a pair that
fp32 puts on the other side is another function, not a rounding error: in float64 every Y[n].x of the soft, trained and raw cases
keeps GAP = 1e-2 from +-64 (above the worst-case fp32 error of a 256-term dot product of entries <= 1, 256 * 2^-24 * 256 = 4e-3);
buffer rows that do not are redrawn from the case's generator (`redrawn`, at most 2 % of the rows).  pm1 products are exact integers
in fp32 and need no gap.  Cases with `beyond` have at least 5 % of their pairs beyond the clamp in each likelihood.  For cases with
`edges`, dropping the first or last row of any chunk of the likelihood grid (lik_grid, a copy of the kernel's) or the last row of N
moves each of the four likelihood terms and code gradients by at least 10 x the bound the GPU test applies (likelihood-only weights).

Error measure.  rel_err = max|got - fp64| / max|fp64| per kind: the ten terms as one vector, then each of the eight gradients.  A
gradient whose float64 reference is identically zero (the cls features at B = 1, the token features at K = 1: softmax_row +
softmax_col - 2 = 0; every feature gradient when hyper_info_nce = 0) is checked exactly instead: anything but zeros counts as an
infinite error, for the port and for the float32 restatement alike.  The yardstick per kind is max(pool, e_ref): pool = the reference's
own fp32 numbers of tests/golden/loss_mith.npz against the float64 restatement over the six golden cases, e_ref = the float32
restatement against the float64 one at the case's own inputs.  `compare` prints the figures and asserts e <= TOL_FACTOR * yardstick."""
import contextlib

import numpy as np
import torch
import torch.nn.functional as F

from oracle import losses as OL

TERMS = OL.MITH_TERMS
INPUTS = OL.MITH_INPUTS
WEIGHTS = OL.MITH_WEIGHTS
KINDS = ("terms",) + tuple("g_" + k for k in INPUTS)
CODES = (2, 3, 4, 5)                 # img_cls_hash, txt_cls_hash, tokens_hash_i, tokens_hash_t in the input order
LIK_OF = {2: 4, 3: 3, 4: 1, 5: 2}    # input -> the likelihood term it enters: t2i(c_i), i2t(c_t), intra_i(t_i), intra_t(t_t)
SEED = 1814
GAP = 1e-2
CLAMP = 64.0
TOL_FACTOR = 4.0
TILE, LIK_TARGET = 64, 1024          # xmh_mith_loss.hip: kTile, kLikTarget

DEFAULT = dict(zip(WEIGHTS, (1.0, 1.0, 50.0, 10.0, 8.0, 0.01, 0.99)))
WSETS = {
    "default": DEFAULT,
    "golden": dict(zip(WEIGHTS, (0.5, 2.0, 3.0, 0.25, 1.5, 0.0, 0.7))),         # the golden case `weights` (asserted on the CPU)
    "lik_only": dict(DEFAULT, hyper_quan=0.0, hyper_distill=0.0, hyper_info_nce=0.0),
}

EDGE_ROWS = (0, 63, 64, 127, 128, 129)
# name -> N, B, K, D, family; beyond: at least 5 % of the pairs of each likelihood lie beyond the clamp; edges: the edge-row condition
# holds; dots (pm1): Y[row].base at EDGE_ROWS; zero: the gradients whose float64 reference vanishes identically
CASES = {
    "n130_b17_k65_d17": dict(N=130, B=17, K=65, D=17, family="soft", edges=True, grid=(2, 3, 64)),
    "n2100_b1024_k16_d16": dict(N=2100, B=1024, K=16, D=16, family="soft", edges=True, grid=(64, 11, 192)),
    "n4200_b256_k15_d33": dict(N=4200, B=256, K=15, D=33, family="soft", edges=True, grid=(16, 33, 128)),
    "n200_b5_k256_d48": dict(N=200, B=5, K=256, D=48, family="trained", beyond=True),
    "n200_b9_k192_d40": dict(N=200, B=9, K=192, D=40, family="trained", beyond=True),
    # B = 20, not more: the rows the gap redraws grow with the 4 B N pairs (about 1e-4 of them fall within GAP of the clamp at this K),
    # the cap on them with N alone
    "n300_b20_k129_d65": dict(N=300, B=20, K=129, D=65, family="trained", beyond=True),
    "n70_b1_k1_d1": dict(N=70, B=1, K=1, D=1, family="soft", zero=("g_res_img_cls", "g_res_txt_cls", "g_trans_tokens_i", "g_trans_tokens_t")),
    "n64_b4_k16_d2048": dict(N=64, B=4, K=16, D=2048, family="soft"),
    "n129_b3_k100_d63_raw": dict(N=129, B=3, K=100, D=63, family="raw"),
    "n130_b4_k256_d32_pm1": dict(N=130, B=4, K=256, D=32, family="pm1", edges=True, dots=(64, 66, -64, 62, 0, 256)),
    "n130_b4_k192_d32_pm1": dict(N=130, B=4, K=192, D=32, family="pm1", edges=True, dots=(62, -64, -66, 64, -192, 0)),
    "n4194304_b2_k3_d1": dict(N=1 << 22, B=2, K=3, D=1, family="soft", grid=(1, 1024, 4096)),
}
EXTRA_WEIGHTS = ("n130_b17_k65_d17", "n4200_b256_k15_d33", "n200_b5_k256_d48")
RUNS = [(n, "default") for n in CASES] + [(n, w) for n in EXTRA_WEIGHTS for w in ("golden", "lik_only")]

# Non-finite inputs: fixed small tensors (soft family), N = 70 so that the poisoned row 66 lies in the second chunk.  Recorded from the
# float64 and float32 restatements on the CPU (tests/test_mith_loss_cases_cpu.py asserts that both still give them): the terms that
# are NaN, and per gradient the NaN entries -- "all", ("col", k) = column k of every row, ("entry", (b, k)) = that entry alone;
# gradients not named are finite throughout.
NF_N, NF_B, NF_K, NF_D, NF_ROW = 70, 3, 8, 8, 66
_LIK4 = ("loss", "intra_i", "intra_t", "i2t", "t2i")
NONFINITE = {
    "nan_buffer_entry": dict(poke="Y[66, 2] = nan", nan_terms=_LIK4, grads={"g_" + INPUTS[i]: ("col", 2) for i in CODES}),
    "nan_code_entry": dict(poke="img_cls_hash[1, 3] = nan", nan_terms=("loss", "t2i", "quan_i", "distillation"),
                           grads={"g_img_cls_hash": ("entry", (1, 3)), "g_tokens_hash_i": ("entry", (1, 3))}),
    "nan_feature_entry": dict(poke="res_img_cls[1, 3] = nan", nan_terms=("loss", "nce_cls"),
                              grads={"g_res_img_cls": "all", "g_res_txt_cls": "all"}),
    "inf_buffer_row": dict(poke="Y[66] = +inf", nan_terms=_LIK4, grads={"g_" + INPUTS[i]: "all" for i in CODES}),
}


# ---- the likelihood grid (a copy of lik_grid in csrc/xmh_mith_loss.hip) ---------------------------------------------------------
def lik_grid(N, B):
    """-> (ctiles, P, rows): column tiles of the 4B stacked code columns, the number of N chunks, and the rows of a chunk"""
    ctiles = (4 * B + TILE - 1) // TILE
    ntiles = (N + TILE - 1) // TILE
    P = max(1, min((LIK_TARGET + ctiles - 1) // ctiles, ntiles))
    per = (ntiles + P - 1) // P
    return ctiles, (ntiles + per - 1) // per, per * TILE


def edge_rows(N, B):
    """the first and the last row of every chunk, and the last row of N"""
    _, P, rows = lik_grid(N, B)
    out = set()
    for p in range(P):
        out.update((p * rows, min(N, (p + 1) * rows) - 1))
    out.add(N - 1)
    return sorted(out)


# ---- the restatement ----------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


def _result(t, leaves):
    return dict({"g_" + k: x.grad.double().numpy() for k, x in zip(INPUTS, leaves)},
                terms=np.array([float(v.detach()) for v in t], dtype=np.float64))


def restate(xs, Y, S, w, dtype=torch.float64):
    """xs the eight inputs, Y [N, K] the buffer after the row write, S [N, B], w the weights -> dict(terms [10] in TERMS order, one
    g_<input> per input) as float64 numpy: oracle.losses.mith_terms and its backward evaluated in `dtype`"""
    leaves = [torch.as_tensor(x).detach().to(dtype).clone().requires_grad_(True) for x in xs]
    with one_thread():
        t = OL.mith_terms(leaves, torch.as_tensor(Y).to(dtype), torch.as_tensor(S).to(dtype), w)
        assert all(v.dtype == dtype for v in t)
        t[0].backward()
    return _result(t, leaves)


def restate_broken(xs, Y, S, w, drop_row=None, open_mask=False, dtype=torch.float32):
    """the restatement with a defect a kernel could have, for showing that `compare` notices it: drop_row = that buffer row is left out
    of the four likelihood sums (still divided by N B); open_mask = the clamp's gradient passes on the open interval |d| < 64 only"""
    leaves = [torch.as_tensor(x).detach().to(dtype).clone().requires_grad_(True) for x in xs]
    Y, S = torch.as_tensor(Y).to(dtype), torch.as_tensor(S).to(dtype)
    keep = torch.ones(Y.shape[0], dtype=torch.bool)
    if drop_row is not None:
        keep[drop_row] = False

    def bayes(b):
        d = Y @ b.T
        s = 0.5 * d.clamp(min=-CLAMP, max=CLAMP)
        if open_mask:
            s = torch.where(d.abs() < CLAMP, s, s.detach())
        return -(S * s - torch.log(1 + torch.exp(s)))[keep].sum() / (Y.shape[0] * b.shape[0])

    with one_thread():
        t = OL.mith_terms(leaves, Y, S, w)
        for i in CODES:
            t[LIK_OF[i]] = bayes(leaves[i])
        t[0] = (w["hyper_tokens_intra"] * (t[1] + t[2]) + w["hyper_cls_inter"] * (t[3] + t[4]) + w["hyper_quan"] * (t[5] + t[6])
                + w["hyper_info_nce"] * (t[7] + w["hyper_alpha"] * t[8]) + t[9])
        t[0].backward()
    return _result(t, leaves)


# ---- error measure, yardstick and the comparison ------------------------------------------------------------------------------
def rel_err(x, ref):
    """max|x - ref| / max|ref|; a reference that is identically zero is met by exact zeros alone (error 0, else inf)"""
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    scale = float(np.abs(ref).max())
    if scale == 0.0:
        return 0.0 if not x.any() else float("inf")
    return float(np.abs(x - ref).max()) / scale


def errors(got, ref):
    return {k: rel_err(got[k], ref[k]) for k in KINDS}


_pool = None


def golden_pool():
    """per kind: the largest error of the reference's own fp32 run (the golden file) against the float64 restatement"""
    global _pool
    if _pool is None:
        worst = {k: 0.0 for k in KINDS}
        for name in OL.MITH_CASES:
            _, _, _, _, w, _, steps = OL.load_mith(name)
            for st in steps:
                ref = restate(st["inputs"], st["buf"], st["label_sim"], w)
                got = dict({"g_" + k: g for k, g in zip(INPUTS, st["grads"])}, terms=st["terms"])
                e = errors(got, ref)
                worst = {k: max(worst[k], e[k]) for k in KINDS}
        _pool = worst
    return dict(_pool)


def yardstick(e_ref):
    pool = golden_pool()
    return {k: max(pool[k], e_ref[k]) for k in KINDS}


def compare(what, got, ref, r32, kinds=KINDS):
    """prints e_ref, the yardstick, the error of `got`, their ratio and the bound per kind, then asserts that `got` is finite and that
    e <= TOL_FACTOR * max(pool, e_ref); -> the errors"""
    e_ref, e = errors(r32, ref), errors(got, ref)
    yard = yardstick(e_ref)
    for k in kinds:
        print("%s %-16s e_ref %.2e  yardstick %.2e  e_port %.2e  e_port/e_ref %.2f  bound %.2e%s" %
              (what, k, e_ref[k], yard[k], e[k], e[k] / e_ref[k] if e_ref[k] else float("inf"), TOL_FACTOR * yard[k],
               "  (exact zeros)" if not np.asarray(ref[k]).any() else ""))
    for k in kinds:
        assert np.isfinite(got[k]).all(), (what, k)
        if not np.asarray(ref[k]).any():
            assert e_ref[k] == 0.0, (what, k, "the float32 restatement does not vanish where float64 does")
        assert e[k] <= TOL_FACTOR * yard[k], (what, k, e[k], yard[k])
    return e


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def _gen(name):
    return torch.Generator().manual_seed(SEED * 1000 + sorted(list(CASES) + list(NONFINITE)).index(name))


def batch_rows(N, B):
    """the buffer rows of the batch: spread over N, never row 0, never the last rows"""
    return 1 + np.arange(B, dtype=np.int64) * ((N - 2) // B)


def _soft_codes(g, n, K, base=None):
    return torch.tanh(torch.randn(n, K, generator=g) * 1.5)


def _trained_codes(g, n, K, base, stratified=False):
    """stratified: one p from each n-th of (0, 1), in random order (the few rows of a code then cover both ends at every draw)"""
    p = torch.rand(n, 1, generator=g)
    if stratified:
        p = (torch.randperm(n, generator=g).float()[:, None] + p) / n
    flip = (torch.rand(n, K, generator=g) < p).float()
    return base * (1.0 - 2.0 * flip) * (0.8 + 0.2 * torch.rand(n, K, generator=g))


def _pm1_codes(g, n, K, base=None):
    return torch.where(torch.rand(n, K, generator=g) < 0.5, -1.0, 1.0)


def _features(g, B, K, D, raw):
    f = [torch.randn(B, D, generator=g), torch.randn(B, D, generator=g), torch.randn(K, B, D, generator=g),
         torch.randn(K, B, D, generator=g)]
    return [1.5 * t for t in f] if raw else [F.normalize(t, dim=-1) for t in f]


def _flipped(base, flips):
    """the base with its first `flips` bits negated"""
    row = base.clone()
    row[:flips] = -row[:flips]
    return row


PM1_SIGNS = (1.0, -1.0, 1.0, -1.0)   # row q of code q (input order c_i, c_t, t_i, t_t) is PM1_SIGNS[q] * base


def dots64(xs, Y):
    """[N, 4B] float64: Y[n] . x for the rows x of the four codes, stacked in the input order"""
    with one_thread():
        return torch.as_tensor(Y).double() @ torch.cat([torch.as_tensor(xs[i]).double() for i in CODES]).T


_built = {}


def build(name):
    """-> dict(spec, xs = the eight inputs, Y [N, K], S [N, B] (all fp32), idx = the batch's buffer rows (Y[idx] == tokens_hash_t),
    redrawn = buffer rows redrawn for the gap, base = the pattern of the trained and pm1 families); the same tensors at every call"""
    if name in _built:
        return _built[name]
    spec, g = CASES[name], _gen(name)
    N, B, K, D, fam = spec["N"], spec["B"], spec["K"], spec["D"], spec["family"]
    base = torch.where(torch.randn(K, generator=g) < 0, -1.0, 1.0)
    rows_of = {"soft": _soft_codes, "raw": _soft_codes, "trained": _trained_codes, "pm1": _pm1_codes}[fam]
    f = _features(g, B, K, D, raw=(fam == "raw"))
    codes = [_trained_codes(g, B, K, base, stratified=True) if fam == "trained" else rows_of(g, B, K, base) for _ in range(4)]
    Y = rows_of(g, N, K, base)
    S = (torch.rand(N, B, generator=g) < 0.1).float()
    idx = batch_rows(N, B)
    if fam == "pm1":
        assert B == 4 and not set(idx.tolist()) & set(EDGE_ROWS)
        for q in range(4):
            codes[q][q] = PM1_SIGNS[q] * base
        for row, d in zip(EDGE_ROWS, spec["dots"]):
            assert (K - d) % 2 == 0
            Y[row] = _flipped(base, (K - d) // 2)
            for q in range(4):                      # S - sigma(s) = +-1 at the designed entries: the clamp mask alone decides
                S[row, q] = 1.0 if PM1_SIGNS[q] * d < 0 else 0.0
    xs = [f[0], f[1], *codes, f[2], f[3]]
    Y[idx] = xs[5]
    redrawn = 0
    if fam != "pm1" and K >= CLAMP:                 # entries are at most 1 in size: below K = 64 no product comes near the clamp
        batch = set(idx.tolist())
        for _ in range(100):
            near = ((dots64(xs, Y).abs() - CLAMP).abs() < GAP).any(1)
            bad = torch.nonzero(near).flatten().tolist()
            if not bad:
                break
            redrawn += len(bad)
            for n in bad:
                Y[n] = rows_of(g, 1, K, base)[0]
                if n in batch:                      # a batch row holds tokens_hash_t: the code row follows
                    xs[5][int(np.nonzero(idx == n)[0][0])] = Y[n]
        else:
            raise AssertionError("%s: no draw keeps every dot product %g away from the clamp" % (name, GAP))
    _built[name] = dict(spec, name=name, xs=xs, Y=Y, S=S, idx=idx, redrawn=redrawn, base=base)
    return _built[name]


def with_edge_S(c, value):
    """case 10's S with the rows EDGE_ROWS set to `value` across the batch"""
    S = c["S"].clone()
    S[list(EDGE_ROWS)] = value
    return S


def build_nonfinite(name):
    """-> (xs, Y [70, 8], S [70, 3], idx) fp32 with the poke applied; the poisoned buffer row is none of the batch's"""
    g = _gen(name)
    f = _features(g, NF_B, NF_K, NF_D, raw=False)
    codes = [_soft_codes(g, NF_B, NF_K) for _ in range(4)]
    Y = _soft_codes(g, NF_N, NF_K)
    S = (torch.rand(NF_N, NF_B, generator=g) < 0.1).float()
    idx = batch_rows(NF_N, NF_B)
    assert NF_ROW not in idx.tolist()
    xs = [f[0], f[1], *codes, f[2], f[3]]
    Y[idx] = xs[5]
    if name == "nan_buffer_entry":
        Y[NF_ROW, 2] = float("nan")
    elif name == "nan_code_entry":
        xs[2][1, 3] = float("nan")
    elif name == "nan_feature_entry":
        xs[0][1, 3] = float("nan")
    else:
        Y[NF_ROW] = float("inf")
    return xs, Y, S, idx


def nan_mask(spec, shape):
    m = np.zeros(shape, dtype=bool)
    if spec == "all":
        m[...] = True
    elif spec is not None and spec[0] == "col":
        m[:, spec[1]] = True
    elif spec is not None:
        m[spec[1]] = True
    return m


def nan_pattern(r):
    """-> (names of the NaN terms, {gradient: bool mask of its NaN entries}) of a result of restate or of the port; no inf anywhere
    (asserted)"""
    assert not any(np.isinf(r[k]).any() for k in KINDS), [k for k in KINDS if np.isinf(r[k]).any()]
    return tuple(t for t, v in zip(TERMS, r["terms"]) if np.isnan(v)), {k: np.isnan(r[k]) for k in KINDS[1:]}


def recorded_pattern(name, r):
    """the recorded pattern of a NONFINITE entry in the form nan_pattern returns (r gives the shapes)"""
    spec = NONFINITE[name]
    return tuple(spec["nan_terms"]), {k: nan_mask(spec["grads"].get(k), r[k].shape) for k in KINDS[1:]}


def same_pattern(a, b):
    return a[0] == b[0] and all(np.array_equal(a[1][k], b[1][k]) for k in KINDS[1:])


# ---- shared references --------------------------------------------------------------------------------------------------------
_refs = {}


def reference(name, wname="default", dtype=torch.float64):
    """restate of a case under a weight set, computed once and handed out read-only"""
    key = (name, wname, dtype)
    if key not in _refs:
        c = build(name)
        r = restate(c["xs"], c["Y"], c["S"], WSETS[wname], dtype)
        for v in r.values():
            v.setflags(write=False)
        _refs[key] = r
    return _refs[key]


# ---- the conditions on the inputs ---------------------------------------------------------------------------------------------
def row_effect(c, n, w):
    """float64, closed form: what leaving buffer row n out of the likelihood sums changes -> (|change| of the four likelihood terms
    in the input order of CODES, max|change| of the four code gradients)"""
    N, B = c["N"], c["B"]
    y = c["Y"][n].double()
    S = c["S"][n].double()
    dt, dg = [], []
    for i in CODES:
        d = c["xs"][i].double() @ y                                             # [B]
        s = 0.5 * d.clamp(-CLAMP, CLAMP)
        dt.append(abs(float((S * s - torch.log(1 + torch.exp(s))).sum())) / (N * B))
        wq = w["hyper_tokens_intra"] if i in (4, 5) else w["hyper_cls_inter"]
        m = ((d >= -CLAMP) & (d <= CLAMP)).double()
        dg.append(float((wq * 0.5 / (N * B) * (S - torch.sigmoid(s)) * m).abs().max() * y.abs().max()))
    return dt, dg


def check_conditions(name):
    """asserts what the case promises of its inputs and returns the measurements; called by the CPU test, and by the GPU test before
    it compares anything"""
    c = build(name)
    N, B, K, D, fam = c["N"], c["B"], c["K"], c["D"], c["family"]
    xs, Y, S, idx = c["xs"], c["Y"], c["S"], c["idx"]
    assert [tuple(t.shape) for t in xs] == [(B, D)] * 2 + [(B, K)] * 4 + [(K, B, D)] * 2 and Y.shape == (N, K) and S.shape == (N, B)
    assert all(t.dtype == torch.float32 and bool(torch.isfinite(t).all()) for t in xs + [Y, S])
    assert len(set(idx.tolist())) == B and torch.equal(Y[idx], xs[5])
    if "grid" in c:
        assert lik_grid(N, B) == c["grid"], (name, lik_grid(N, B))
    assert all(float(t.abs().max()) <= 1.0 for t in xs[2:6] + [Y])
    if K >= CLAMP:
        d = dots64(xs, Y)
        out = dict(redrawn=c["redrawn"], gap=float((d.abs() - CLAMP).abs().min()),
                   beyond=[float((d[:, q * B:(q + 1) * B].abs() > CLAMP).double().mean()) for q in range(4)])
    else:                                             # |Y[n] . x| <= K
        out = dict(redrawn=c["redrawn"], gap=CLAMP - K, beyond=[0.0] * 4)
    assert c["redrawn"] <= 0.02 * N, (name, c["redrawn"])
    if fam == "pm1":
        assert all(bool(((t == 1) | (t == -1)).all()) for t in xs[2:6] + [Y])
        seen = set()
        for q in range(4):
            assert torch.equal(xs[2 + q][q], PM1_SIGNS[q] * c["base"])
            col = d[list(EDGE_ROWS), q * B + q]
            assert col.tolist() == [PM1_SIGNS[q] * v for v in c["dots"]], (name, q, col)
            seen.update(int(v) for v in col.tolist())
            for row, v in zip(EDGE_ROWS, col.tolist()):
                assert float(S[row, q]) == (1.0 if v < 0 else 0.0)
        assert {64, -64, 62, -62, 66, -66, 0, K, -K} <= seen, (name, sorted(seen))
        assert list(EDGE_ROWS) == edge_rows(N, B)
    else:
        assert out["gap"] >= GAP, (name, out["gap"])
    if c.get("beyond"):
        assert min(out["beyond"]) >= 0.05, (name, out["beyond"])
    if c.get("edges"):
        w = WSETS["lik_only"]
        ref, r32 = reference(name, "lik_only"), reference(name, "lik_only", torch.float32)
        bound = {k: TOL_FACTOR * v for k, v in yardstick(errors(r32, ref)).items()}
        tmax = float(np.abs(ref["terms"]).max())
        worst = float("inf")
        for n in edge_rows(N, B):
            dt, dg = row_effect(c, n, w)
            for i, t, gmax in zip(CODES, dt, dg):
                k = "g_" + INPUTS[i]
                worst = min(worst, t / tmax / bound["terms"], gmax / float(np.abs(ref[k]).max()) / bound[k])
                assert t / tmax >= 10 * bound["terms"], (name, n, TERMS[LIK_OF[i]], t / tmax, bound["terms"])
                assert gmax / float(np.abs(ref[k]).max()) >= 10 * bound[k], (name, n, k, gmax, bound[k])
        out["edge_rows"], out["edge_least"] = len(edge_rows(N, B)), worst
    return out


def describe(m):
    s = "redrawn %d  gap %.3g  beyond the clamp %s" % (m["redrawn"], m["gap"], " ".join("%.3f" % v for v in m["beyond"]))
    if "edge_rows" in m:
        s += "  %d edge rows, the least effect of one is %.0f x the bound" % (m["edge_rows"], m["edge_least"])
    return s
