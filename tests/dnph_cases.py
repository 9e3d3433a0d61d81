"""Cases and restatement of DNPH's training objective (reference models/DNPH/loss/loss.py:12-33, models/DNPH/DNPH.py:72-99) and of
its head, shared by tests/test_dnph_cpu.py, tests/test_gpu_dnph_loss.py, tests/test_gpu_dnph_train.py and tools/make_golden_dnph.py;
and the edge cases (EDGE_CASES, NONFINITE, at the end) of tests/test_dnph_cases_cpu.py and tests/test_gpu_dnph_loss_f64.py.

The restatement is written from the reference's expressions, in torch on the CPU with torch's autograd for the gradients, with the
dtype as a parameter: float64 is the truth the GPU tests compare with, float32 on the same inputs is the yardstick (e_ref).

  objective   u = normalize(cat(f_img, f_txt)), q = normalize(P); D = sum_k (u - q)^2 (a sum of squared differences, as the kernel
              forms it; the reference's torch.cdist ** 2 is the same number) + mrg on the rows' own classes;
              p_loss = mean_n sum_c -l log_softmax(-D); d_loss_m = CE(p_m, argmax l); noise_m = mean_b sum_k f_m noise_m;
              loss = p_loss + d_loss_img + d_loss_txt - noise_alpha (noise_img + noise_txt)
              -> terms [6] (loss, p_loss, d_loss_img, d_loss_txt, noise_img, noise_txt) and the gradients of up * loss
  head        tanh(keep * (x W^T + b) / (1 - p)) and x Wp^T + bp per modality, then the objective (chain)

Error rule (tests/test_gpu_tower_grad.py's): per tensor e = max|got - f64| / max|f64|; the port must stay within TOL_FACTOR *
max(pool, e_ref), e_ref the float32 restatement's e on the same inputs and pool the largest e_ref of that tensor kind over CASES."""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

TOL_FACTOR = 4.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dnph.npz")
GOLDEN_CASES = {"small": dict(B=7, K=16, C=5, Cp=80, seed=5201), "mid": dict(B=37, K=48, C=33, Cp=80, seed=5202)}

# name -> B, K, C (proxies), Cp (class logits), mrg, noise_alpha, upstream.  B = 1, 37, 65, 257: one row, less than a wave of rows, a
# wave and one, more than one 256-row chunk of the proxy blocks (2B = 514: three chunks); K = 16, 48, 130: less than a wave of
# columns, not a multiple of 64, more than two lanes' worth; C = 1, 24, 32, 33, 80: one class, label-word edges; Cp = C and 80 > C.
# zero: row 2 of the image codes is all zero (F.normalize's eps branch: its gradient is du / 1e-12).
CASES = {
    "b1_k16_c1": dict(B=1, K=16, C=1, Cp=1, mrg=1.0, alpha=0.1, up=1.0, seed=5101),
    "b37_k48_c24": dict(B=37, K=48, C=24, Cp=80, mrg=1.0, alpha=0.1, up=0.37, seed=5102),
    "b65_k130_c32": dict(B=65, K=130, C=32, Cp=32, mrg=1.0, alpha=1.0, up=2.5, seed=5103),
    "b37_k16_c33": dict(B=37, K=16, C=33, Cp=80, mrg=0.5, alpha=0.1, up=1.0, seed=5104),
    "b257_k48_c80": dict(B=257, K=48, C=80, Cp=80, mrg=1.0, alpha=0.1, up=1.0, seed=5105),
    "b65_k16_c33_zero": dict(B=65, K=16, C=33, Cp=33, mrg=1.0, alpha=0.1, up=1.0, seed=5106, zero=True),
    "b37_k48_c24_mrg50": dict(B=37, K=48, C=24, Cp=80, mrg=50.0, alpha=0.1, up=1.0, seed=5107),
}
TERMS = ("loss", "p_loss", "d_loss_img", "d_loss_txt", "noise_img", "noise_txt")
GRADS = ("g_f_img", "g_f_txt", "g_p_img", "g_p_txt", "g_P")
KINDS = ("term", "g_f", "g_p", "g_P", "nz_f")        # nz_f: a code gradient with the eps-branch row zeroed on both sides
ZERO_ROW = 2


def rel_err(got, want):
    """max|got - want| / max|want| (absolute where the reference tensor is identically zero)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = np.abs(want).max() if want.size else 0.0
    return float(np.abs(got - want).max() / (scale if scale > 0 else 1.0)) if want.size else 0.0


# ---- restatement -------------------------------------------------------------------------------------------------------------------
def objective_terms(f_img, f_txt, p_img, p_txt, P, labels, mrg, alpha, noise_img=None, noise_txt=None, stash=None):
    """torch tensors of one dtype (labels: 0 / 1 of any dtype) -> the six terms, a tensor with a graph.  stash: a dict that receives the
    normalised rows u [2B, K] and q [C, K] with retain_grad set, so that the gradient arriving at them can be read after backward"""
    dtype = f_img.dtype
    lab = (torch.as_tensor(labels) == 1).to(dtype)
    u = F.normalize(torch.cat((f_img, f_txt), 0), p=2, dim=-1)
    q = F.normalize(P, p=2, dim=-1)
    if stash is not None:
        u.retain_grad()
        q.retain_grad()
        stash["u"], stash["q"] = u, q
    D = ((u[:, None, :] - q[None, :, :]) ** 2).sum(-1)
    l2 = torch.cat((lab, lab), 0)
    D = D + mrg * l2
    p_loss = torch.sum(-l2 * F.log_softmax(-D, 1), -1).mean()
    t = torch.argmax(lab, -1)
    d_img, d_txt = F.cross_entropy(p_img, t), F.cross_entropy(p_txt, t)
    zero = torch.zeros((), dtype=dtype)
    n_img = zero if noise_img is None else (f_img * noise_img.to(dtype)).sum(-1).mean()
    n_txt = zero if noise_txt is None else (f_txt * noise_txt.to(dtype)).sum(-1).mean()
    loss = p_loss + (d_img + d_txt) - alpha * (n_img + n_txt)
    return torch.stack([loss, p_loss, d_img, d_txt, n_img, n_txt])


def objective(c, dtype, mrg=None, alpha=None, up=None, noise=True, stash=None):
    """case dict (numpy inputs) -> {terms..., g_*: gradients of up * loss} as float64 numpy, computed in `dtype`.  stash: see
    objective_terms; after the call stash["u"].grad and stash["q"].grad hold what arrives at the normalised rows"""
    leaves = {k: torch.tensor(c[k]).to(dtype).requires_grad_(True) for k in ("f_img", "f_txt", "p_img", "p_txt", "P")}
    ns = [torch.tensor(c[k]) if noise else None for k in ("noise_img", "noise_txt")]
    terms = objective_terms(*[leaves[k] for k in ("f_img", "f_txt", "p_img", "p_txt", "P")], torch.tensor(c["labels"]),
                            c["mrg"] if mrg is None else mrg, c["alpha"] if alpha is None else alpha, *ns, stash=stash)
    (terms[0] * (c["up"] if up is None else up)).backward()
    out = {k: terms[i].detach().double().numpy().reshape(1) for i, k in enumerate(TERMS)}
    for g, k in zip(GRADS, ("f_img", "f_txt", "p_img", "p_txt", "P")):
        out[g] = leaves[k].grad.double().numpy()
    return expand(c, out)


def expand(c, vals):
    """what is compared: every term and gradient as it is and, in a case with the all-zero image row, g_f_img again with that row
    zeroed (nz_f_img): the row's du / 1e-12 sets the whole tensor's scale, the other rows are then checked at their own"""
    out = dict(vals)
    if c.get("zero") and vals.get("g_f_img") is not None:
        nz = np.array(vals["g_f_img"], np.float64)
        nz[ZERO_ROW] = 0
        out["nz_f_img"] = nz
    return {k: v for k, v in out.items() if v is not None}


def kind_of(key):
    return "term" if key in TERMS else next(k for k in KINDS if key.startswith(k))


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def draw(B, K, C, Cp, seed, zero=False, density=0.15, **rest):
    """float32 / integer numpy inputs.  Rows by design (where B allows): row 0 has no label, row 1 every label; with `zero`, row 2 of
    the image codes is all zero.  The codes are tanh outputs, the logits of unit-ish scale, the proxies randn / 8 as constructed."""
    rng = np.random.default_rng(seed)
    labels = (rng.random((B, C)) < density).astype(np.int64)
    labels[np.arange(B), rng.integers(0, C, B)] = 1
    if B >= 3:
        labels[0] = 0
        labels[1] = 1
    f = {m: np.tanh(rng.standard_normal((B, K)) * 1.5).astype(np.float32) for m in ("img", "txt")}
    if zero:
        f["img"][ZERO_ROW] = 0.0
    p = {m: (rng.standard_normal((B, Cp)) * 2.0).astype(np.float32) for m in ("img", "txt")}
    P = (rng.standard_normal((C, K)) / 8.0).astype(np.float32)
    noise = {m: (rng.integers(0, 2, (B, K)) * 2 - 1).astype(np.float32) for m in ("img", "txt")}
    return dict(rest, B=B, K=K, C=C, Cp=Cp, seed=seed, zero=zero, labels=labels, f_img=f["img"], f_txt=f["txt"], p_img=p["img"], p_txt=p["txt"],
                P=P, noise_img=noise["img"], noise_txt=noise["txt"])


@functools.lru_cache(maxsize=None)
def build(name):
    return dict(draw(**CASES[name]), name=name)


@functools.lru_cache(maxsize=None)
def reference(name, dtype=torch.float64):
    return objective(build(name), dtype)


@functools.lru_cache(maxsize=None)
def e_ref(name):
    """per tensor: the float32 restatement's error against the float64 one"""
    r64, r32 = reference(name, torch.float64), reference(name, torch.float32)
    return {k: rel_err(r32[k], r64[k]) for k in r64}


@functools.lru_cache(maxsize=None)
def pool():
    """per tensor kind, the largest e_ref over CASES"""
    out = {k: 0.0 for k in KINDS}
    for name in CASES:
        for key, e in e_ref(name).items():
            out[kind_of(key)] = max(out[kind_of(key)], e)
    return out


def compare(what, got, ref64, own):
    """prints e, the yardstick and their ratio for every tensor of `got`, then asserts e <= TOL_FACTOR * max(pool, e_ref) -> worst ratio"""
    rows = []
    for key, g in got.items():
        yard = max(pool().get(kind_of(key), 0.0), own.get(key, 0.0))
        e = rel_err(g, ref64[key])
        rows.append((key, e, yard))
        print("%-22s %-11s e %.3e  yardstick %.3e  ratio %.2f  bound %.3e" % (what, key, e, yard, e / yard if yard else float("inf"),
                                                                               TOL_FACTOR * yard))
    for key, e, yard in rows:
        assert np.asarray(got[key]).shape == ref64[key].shape, (what, key)
        assert e <= TOL_FACTOR * yard, (what, key, e, yard)
    return max((e / yard if yard else float("inf")) for _, e, yard in rows)


# ---- the chain head -> objective ------------------------------------------------------------------------------------------------------
HEAD_PARAMS = ("hash_w", "hash_b", "pre_w", "pre_b")
HEAD_KEYS = {"hash_w": "%s_hash.fc.weight", "hash_b": "%s_hash.fc.bias", "pre_w": "%s_pre.fc.weight", "pre_b": "%s_pre.fc.bias"}
MOD = {"img": "image", "txt": "text"}


def draw_head(seed, K, E, Cp=80):
    """parameters of one modality's two layers away from their initial values, float32"""
    rng = np.random.default_rng(seed)
    u = lambda shape, a: ((rng.random(shape) * 2.0 - 1.0) * a).astype(np.float32)      # noqa: E731
    a = 1.0 / np.sqrt(E)
    return {"hash_w": u((K, E), 1.5 * a), "hash_b": u((K,), 0.1), "pre_w": u((Cp, E), 2.0 * a), "pre_b": u((Cp,), 0.1)}


def chain(x, Pm, keep, P, labels, noises, mrg, alpha, p_drop, dtype):
    """x / Pm / keep / noises: {"img" / "txt": embeddings [B, E] / head parameters / keep mask [B, K] / assigned noise [B, K]}, numpy.
    The whole chain in `dtype` with torch's autograd -> dict: loss, g_x_<m>, g_<param>_<m>, g_P (float64 numpy)"""
    xs = {m: torch.tensor(x[m]).to(dtype).requires_grad_(True) for m in x}
    Ps = {m: {k: torch.tensor(v).to(dtype).requires_grad_(True) for k, v in Pm[m].items()} for m in Pm}
    Pt = torch.tensor(P).to(dtype).requires_grad_(True)
    f, p = {}, {}
    for m in ("img", "txt"):
        z = xs[m] @ Ps[m]["hash_w"].T + Ps[m]["hash_b"]
        f[m] = torch.tanh(z * torch.tensor(keep[m]).to(dtype) / (1.0 - p_drop))
        p[m] = xs[m] @ Ps[m]["pre_w"].T + Ps[m]["pre_b"]
    terms = objective_terms(f["img"], f["txt"], p["img"], p["txt"], Pt, torch.tensor(labels), mrg, alpha, torch.tensor(noises["img"]),
                            torch.tensor(noises["txt"]))
    terms[0].backward()
    out = {"loss": terms[0].detach().reshape(1), "g_P": Pt.grad}
    for m in ("img", "txt"):
        out["g_x_" + m] = xs[m].grad
        for k in HEAD_PARAMS:
            out["g_%s_%s" % (k, m)] = Ps[m][k].grad
    out = {k: v.double().numpy() for k, v in out.items()}
    out["f_img"], out["f_txt"] = f["img"].detach().double().numpy(), f["txt"].detach().double().numpy()
    return out


# ---- edge cases: tests/test_dnph_cases_cpu.py (their conditions) and tests/test_gpu_dnph_loss_f64.py (the port) ------------------------
# A table of its own: pool() stays the maximum over CASES, so nothing here loosens a bound of tests/test_gpu_dnph_loss.py.
# The inputs are draw's (tanh codes, randn / 8 proxies, +-1 noise, one generator per case), then the overrides the case names:
#   set_labels   row -> its classes ("all": every class), written over the drawn row
#   eye          labels = eye(B), as DNPH.object_function builds them without labels (C = B)
#   density      of the drawn labels (0.15 unless given)
#   zero_img / tiny_txt / tiny_P / zero_P   a row all zero, or rescaled to the given norm (non-zero, below F.normalize's eps)
#   logit_scale  both logit matrices times it
# What each reaches in xmh_dnph.hip (256 threads, kSlots = 16 column slots of 256, label words of 32 classes, 256-row chunks):
#   b5_k257_c33           slot 1 with one live thread; class 32 alone in word 1: rows with (32,), (31,), (31, 32), none, all
#   b3_k4096_c5           the K limit: all 16 slots, the largest LDS
#   b9_k100_c1024         the C and Cp limit, 32 label words, four class strides; lowest labels in word 15, word 16, word 31, at bit 31
#   b6_k63_c257           one class past a stride, Cp no multiple of 64, K one short of a wave
#   b129_k65_c65          2B = 258: a full chunk across the image / text boundary and two rows; class 64 alone in word 2
#   b128_k128_c80         2B = 256: exactly one chunk; K exactly two columns a lane; the shipped 128-bit COCO shape
#   b4096_k16_c2          the B limit: 32 strides of k_dnph_finalize, 32 chunks of a proxy block
#   b97_k16_c97_eye       identity labels: the lowest label at every bit of every word
#   b40_k1_c3             K = 1: every gradient through F.normalize is an exact zero formed as a difference (see cancel_floor); row 0
#                         carries a label and the proxies have both signs, so that every row's parts are non-zero.  (Its seed is the
#                         first of 5309.. at which that holds and the float32 restatement's g_P is not 0.0 in every entry: with three
#                         proxies it often is, and then there is no float32 error to take a yardstick from.)
#   b33_k64_c24_clamped   the eps branch of F.normalize with a zero and a non-zero row, codes and proxies
#   b37_k48_c24_logits    logits whose exp overflows float32 unless the maximum is subtracted
EPS = 1e-12                          # F.normalize's eps
EDGE_CASES = {
    "b5_k257_c33": dict(B=5, K=257, C=33, Cp=33, mrg=1.0, alpha=0.1, up=2.5, seed=5301,
                        set_labels={0: (), 1: "all", 2: (32,), 3: (31,), 4: (31, 32)}),
    "b3_k4096_c5": dict(B=3, K=4096, C=5, Cp=80, mrg=1.0, alpha=1.0, up=1.0, seed=5302),
    "b9_k100_c1024": dict(B=9, K=100, C=1024, Cp=1024, mrg=0.5, alpha=0.1, up=0.37, seed=5303, density=0.003,
                          set_labels={0: (), 2: (1023,), 3: (992,), 4: (512, 1023), 5: (511, 700)}),
    "b6_k63_c257": dict(B=6, K=63, C=257, Cp=300, mrg=1.0, alpha=0.1, up=1.0, seed=5304, set_labels={2: (256,)}),
    "b129_k65_c65": dict(B=129, K=65, C=65, Cp=65, mrg=1.0, alpha=0.1, up=2.5, seed=5305,
                         set_labels={2: (64,), 3: (31, 64), 128: (64,)}),
    "b128_k128_c80": dict(B=128, K=128, C=80, Cp=80, mrg=1.0, alpha=1.0, up=1.0, seed=5306),
    "b4096_k16_c2": dict(B=4096, K=16, C=2, Cp=2, mrg=1.0, alpha=0.1, up=1.0, seed=5307),
    "b97_k16_c97_eye": dict(B=97, K=16, C=97, Cp=97, mrg=1.0, alpha=0.1, up=0.37, seed=5308, eye=True),
    "b40_k1_c3": dict(B=40, K=1, C=3, Cp=3, mrg=1.0, alpha=0.1, up=1.0, seed=5312, set_labels={0: (2,)}),
    "b33_k64_c24_clamped": dict(B=33, K=64, C=24, Cp=80, mrg=1.0, alpha=0.1, up=1.0, seed=5310, zero_img=5, tiny_txt=(9, 3e-13),
                                tiny_P=(7, 3e-13), zero_P=2),
    "b37_k48_c24_logits": dict(B=37, K=48, C=24, Cp=80, mrg=0.5, alpha=0.1, up=1.0, seed=5311, logit_scale=45.0),
}
CODE_OF = {"g_f_img": "f_img", "g_f_txt": "f_txt", "g_P": "P"}          # the gradients that pass through F.normalize, and their inputs


def _rescaled(row, norm):
    return (row.astype(np.float64) * (norm / np.linalg.norm(row.astype(np.float64)))).astype(np.float32)


def _override(spec, c):
    c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    if spec.get("eye"):
        assert spec["B"] == spec["C"]
        c["labels"] = np.eye(spec["B"], dtype=np.int64)
    for row, classes in spec.get("set_labels", {}).items():
        c["labels"][row] = 0
        c["labels"][row, list(range(spec["C"])) if classes == "all" else list(classes)] = 1
    if "zero_img" in spec:
        c["f_img"][spec["zero_img"]] = 0.0
    if "tiny_txt" in spec:
        c["f_txt"][spec["tiny_txt"][0]] = _rescaled(c["f_txt"][spec["tiny_txt"][0]], spec["tiny_txt"][1])
    if "tiny_P" in spec:
        c["P"][spec["tiny_P"][0]] = _rescaled(c["P"][spec["tiny_P"][0]], spec["tiny_P"][1])
    if "zero_P" in spec:
        c["P"][spec["zero_P"]] = 0.0
    if "logit_scale" in spec:
        c["p_img"], c["p_txt"] = c["p_img"] * np.float32(spec["logit_scale"]), c["p_txt"] * np.float32(spec["logit_scale"])
    return c


@functools.lru_cache(maxsize=None)
def build_edge(name):
    spec = EDGE_CASES[name]
    return dict(_override(spec, draw(**spec)), name=name)


def row_norms(c):
    """float64 norm of every code row and proxy, keyed by the gradient that passes through its F.normalize"""
    return {g: np.linalg.norm(np.asarray(c[k], np.float64), axis=1) for g, k in CODE_OF.items()}


def clamped_rows(c):
    """per gradient, the rows whose input norm lies below F.normalize's eps: their gradient is du / eps, 1e10 here"""
    return {g: n < EPS for g, n in row_norms(c).items()}


def restate(c, dtype):
    """-> (objective(c, dtype), du): du per gradient of CODE_OF, what arrives at the normalised rows (of up * loss, float64 numpy)"""
    stash = {}
    vals = objective(c, dtype, stash=stash)
    du_u, B = stash["u"].grad.double().numpy(), c["B"]
    return vals, {"g_f_img": du_u[:B], "g_f_txt": du_u[B:], "g_P": stash["q"].grad.double().numpy()}


def normalize_part(c, vals):
    """the part of each gradient of CODE_OF that came through F.normalize: the whole of g_P, g_f less the noise term's
    -up alpha noise / B (formed in float64)"""
    w = c["up"] * c["alpha"] / c["B"]
    return {"g_f_img": vals["g_f_img"] + w * np.asarray(c["noise_img"], np.float64),
            "g_f_txt": vals["g_f_txt"] + w * np.asarray(c["noise_txt"], np.float64), "g_P": vals["g_P"]}


def cancel_floor(c, du64):
    """K = 1 alone, after hyp_loss_cases.cancel_scale.  n(v) = +-1 whatever v is, so the gradient through F.normalize,
    (du - u (u . du)) / |v|, is exactly zero: float64 returns rounding residue (g_P: 4e-16 at most), and an error divided by that
    measures nothing.  The error of a row is taken relative to the size of the two equal parts that cancel instead, |du| / |v|, du
    the float64 gradient that arrives at the normalised row: per row the floor of the scale its error is divided by."""
    n = row_norms(c)
    return {g: np.abs(du64[g]).max(1) / np.maximum(n[g], EPS) for g in CODE_OF}


def edge_errors(c, vals, ref64, floor=None):
    """-> {key: e}, e = max|got - f64| / max|f64| per tensor, with two refinements.  Rows clamped by eps form a group of their own
    (key + "_clamped", as hyp_loss_cases.errors): each group on its own scale.  With floor (K = 1) the error of each row of a
    gradient of CODE_OF is divided by max(max|f64 tensor|, floor[row])."""
    out, cl = {}, clamped_rows(c)
    for key, want in ref64.items():
        got = np.asarray(vals[key], np.float64)
        if key in cl and cl[key].any():
            out[key], out[key + "_clamped"] = rel_err(got[~cl[key]], want[~cl[key]]), rel_err(got[cl[key]], want[cl[key]])
        elif floor is not None and key in floor:
            out[key] = float((np.abs(got - want).max(1) / np.maximum(np.abs(want).max(), floor[key])).max())
        else:
            out[key] = rel_err(got, want)
    return out


@functools.lru_cache(maxsize=None)
def edge_reference(name):
    """-> (float64 values, float32 values, floor or None, e_ref per key) of an edge case, computed once"""
    c = build_edge(name)
    (r64, du64), (r32, _) = restate(c, torch.float64), restate(c, torch.float32)
    floor = cancel_floor(c, du64) if c["K"] == 1 else None
    return r64, r32, floor, edge_errors(c, r32, r64, floor)


def edge_table(what, e, own):
    """e, own: {key: error} of the port and of the float32 restatement.  Prints e, the yardstick max(pool, e_ref), their ratio and
    the bound for every key -> [(key, e, yardstick)]"""
    rows = [(key, e[key], max(pool().get(kind_of(key), 0.0), own.get(key, 0.0))) for key in e]
    for key, v, yard in rows:
        print("%-24s %-16s e %.3e  e_ref %.3e  yardstick %.3e  ratio %.2f  bound %.3e" %
              (what, key, v, own.get(key, 0.0), yard, v / yard if yard else float("inf"), TOL_FACTOR * yard))
    return rows


def assert_within(what, rows):
    """asserts e <= TOL_FACTOR * yardstick for every row of edge_table -> worst ratio"""
    for key, v, yard in rows:
        assert v <= TOL_FACTOR * yard, (what, key, v, yard)
    return max((v / yard if yard else float("inf")) for _, v, yard in rows)


# ---- non-finite inputs ---------------------------------------------------------------------------------------------------------------
# 6 x 4 codes, C = Cp = 7 (row 0 without a label, row 1 with every one), one poke each.  `want`: what is not finite in the result, as
# recorded from the float32 and float64 restatements on the CPU (tests/test_dnph_cases_cpu.py asserts that both still give it): a term
# "nan" / "+inf" / "-inf"; a gradient ("rows", r...) NaN in exactly those rows, throughout, "all", or ("entry", b, k).  Everything not
# named is finite.  `t` below is the target of the poked row (its lowest label), `o` = (t + 1) % 7 a class off the target.
NONFINITE_SHAPE = dict(B=6, K=4, C=7, Cp=7, mrg=1.0, alpha=0.1, up=1.0, seed=5401)
NONFINITE = {
    "nan_logit": dict(poke="p_img[2, o] = nan", want={"loss": "nan", "d_loss_img": "nan", "g_p_img": ("rows", 2)}),
    "posinf_logit": dict(poke="p_txt[3, o] = +inf", want={"loss": "nan", "d_loss_txt": "nan", "g_p_txt": ("rows", 3)}),
    "neginf_logit_off_target": dict(poke="p_img[2, o] = -inf", want={}),
    "neginf_logit_on_target": dict(poke="p_img[2, t] = -inf", want={"loss": "+inf", "d_loss_img": "+inf"}),
    "inf_code": dict(poke="f_img[3, 1] = +inf", want={"loss": "nan", "p_loss": "nan", "noise_img": "sign of noise_img[3, 1]",
                                                       "g_f_img": ("rows", 3), "g_P": "all"}),
    "nan_noise": dict(poke="noise_txt[4, 2] = nan", want={"loss": "nan", "noise_txt": "nan", "g_f_txt": ("entry", 4, 2)}),
}
FINITE, NAN, PINF, NINF = 0, 1, 2, 3


def nonfinite_target(c, row):
    t = int(np.argmax(c["labels"][row]))
    return t, (t + 1) % c["Cp"]


@functools.lru_cache(maxsize=None)
def build_nonfinite(name, poke=True):
    c = dict(draw(**NONFINITE_SHAPE), name=name)
    if not poke:
        return c
    for k in ("f_img", "p_img", "p_txt", "noise_txt"):
        c[k] = c[k].copy()
    if name == "nan_logit":
        c["p_img"][2, nonfinite_target(c, 2)[1]] = np.nan
    elif name == "posinf_logit":
        c["p_txt"][3, nonfinite_target(c, 3)[1]] = np.inf
    elif name == "neginf_logit_off_target":
        c["p_img"][2, nonfinite_target(c, 2)[1]] = -np.inf
    elif name == "neginf_logit_on_target":
        c["p_img"][2, nonfinite_target(c, 2)[0]] = -np.inf
    elif name == "inf_code":
        c["f_img"][3, 1] = np.inf
    else:
        assert name == "nan_noise"
        c["noise_txt"][4, 2] = np.nan
    return c


def classes(vals):
    """{key: per entry FINITE / NAN / PINF / NINF}"""
    out = {}
    for k, v in vals.items():
        v = np.asarray(v, np.float64)
        out[k] = np.where(np.isnan(v), NAN, np.where(v == np.inf, PINF, np.where(v == -np.inf, NINF, FINITE))).astype(np.int8)
    return out


def recorded_classes(name):
    """NONFINITE[name]["want"] written out entry for entry, in the shapes of objective's result"""
    c, s = build_nonfinite(name), NONFINITE_SHAPE
    shapes = dict({k: (1,) for k in TERMS}, g_f_img=(s["B"], s["K"]), g_f_txt=(s["B"], s["K"]), g_p_img=(s["B"], s["Cp"]),
                  g_p_txt=(s["B"], s["Cp"]), g_P=(s["C"], s["K"]))
    out = {k: np.full(shape, FINITE, np.int8) for k, shape in shapes.items()}
    for k, w in NONFINITE[name]["want"].items():
        if w == "all":
            out[k][:] = NAN
        elif isinstance(w, tuple) and w[0] == "rows":
            out[k][list(w[1:])] = NAN
        elif isinstance(w, tuple):
            out[k][w[1], w[2]] = NAN
        elif w.startswith("sign of"):
            out[k][:] = PINF if c["noise_img"][3, 1] > 0 else NINF
        else:
            out[k][:] = {"nan": NAN, "+inf": PINF, "-inf": NINF}[w]
    return out


def finite_errors(vals, ref64):
    """e per tensor over the entries that are finite in float64 (a tensor without one is left out)"""
    out = {}
    for k, want in ref64.items():
        keep = np.isfinite(want)
        if keep.any():
            out[k] = rel_err(np.asarray(vals[k], np.float64)[keep], want[keep])
    return out
