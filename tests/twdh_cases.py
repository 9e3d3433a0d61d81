"""Cases and restatement of TwDH's training objective (reference models/TwDH/TwDH.py:125-230) and of its short-code transforms, shared
by tests/test_twdh_cpu.py, tests/test_gpu_twdh_loss.py, tests/test_gpu_twdh_train.py and tools/make_golden_twdh_loss.py.

The restatement is written from the reference's expressions, in torch on the CPU, with the dtype as a parameter: float64 is the
truth the GPU tests compare with, float32 on the same inputs is the yardstick (e_ref).  A stream is one code length, the long one
first; `lens` lists them, the target bits of all streams stand side by side ([B, K_tot]), the short probabilities likewise
([B, 2 (K_tot - lens[0])]).

  targets        hash_convert(hash_center_multilables(labels, centre)) as bits: sign of the integer sum of the set labels' centres,
                 the tie vector where the sum is zero, 0 for a row without a label (the reference's NaN mean, checked against it in
                 the golden)
  loss           nn.BCELoss (mean, logs clamped at -100) and 1 - mean((2 p - 1)^2) per modality and stream, the modality means and
                 the total, in the layout of xmh_twdh_loss's output: [total, (m, s, term)..., (s, term) means...]
  loss_grad      what autograd returns for BCELoss, (p - t) / max(p (1 - p), 1e-12) / n, plus -4 (2 p - 1) / n, weighted
  short_forward  pair_softmax(long @ T_cat);  short_backward: g_z = p (g - sum_pair(g p)), g_long = g_z @ T_cat^T
  head / chain   the DCMHT hash layer in train mode (as oracle/heads_train.py, here with the dtype as a parameter and torch's
                 autograd for the gradients), then the transforms, then the objective

Error rule (tests/test_gpu_tower_grad.py's): per tensor e = max|got - f64| / max|f64|; the port must stay within TOL_FACTOR *
max(pool, e_ref), e_ref the float32 restatement's e on the same inputs and pool the largest e_ref of that tensor kind over CASES."""
import functools
import os

import numpy as np
import torch

TOL_FACTOR = 4.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "twdh_loss.npz")

# name -> B, C (label width), lens (long, shorts...), quan_alpha, low_rate, upstream.  B = 1, 3, 65, 130: wave and block edges of the
# row chunks (32 rows) and of the 256-thread blocks; K_tot = 44 and 624: not multiples of 32; C = 1, 33, 80: label-word edges.
CASES = {
    "b1_c1": dict(B=1, C=1, lens=(32, 4, 8), quan_alpha=0.5, low_rate=0.3, up=1.0, seed=4101),
    "b3_c33": dict(B=3, C=33, lens=(32, 4, 8), quan_alpha=0.0, low_rate=0.3, up=0.37, seed=4102),
    "b65_c80": dict(B=65, C=80, lens=(32, 4, 8), quan_alpha=0.5, low_rate=0.3, up=2.5, seed=4103),
    "b130_c80": dict(B=130, C=80, lens=(512, 16, 32, 64), quan_alpha=0.5, low_rate=0.3, up=1.0, seed=4104),
    "b130_c80_lr0": dict(B=130, C=80, lens=(512, 16, 32, 64), quan_alpha=0.5, low_rate=0.0, up=1.0, seed=4105),
}
GOLDEN_CASES = ("small", "coco16")
# tensor kinds of the comparison.  Every scalar of the terms vector is compared on its own (the clamped BCE means would otherwise set
# the scale for the quantisation terms), and every gradient twice: whole (d_*: the saturated entries, 0.5 / 1e-12 / n, set the scale
# and are what is checked) and with the entries of saturated probabilities zeroed (ord_*: every ordinary entry, at its own scale)
KINDS = ("term_total", "term_bce", "term_quan", "d_long", "d_short", "ord_long", "ord_short", "p_short", "g_long")


def rel_err(got, want):
    """max|got - want| / max|want| (absolute where the reference tensor is identically zero)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = np.abs(want).max() if want.size else 0.0
    return float(np.abs(got - want).max() / (scale if scale > 0 else 1.0)) if want.size else 0.0


# ---- restatement -------------------------------------------------------------------------------------------------------------------
def targets(labels, centres, ties):
    """labels [B, C] (set = 1), centres: list of [C', K_s] +-1 with C' >= C, ties: list of [K_s] +-1 -> bits [B, K_tot] uint8"""
    lab = (np.asarray(labels) == 1)
    cen = np.concatenate([np.asarray(c) for c in centres], 1).astype(np.int64)[:lab.shape[1]]
    tie = np.concatenate([np.asarray(t).reshape(-1) for t in ties]).astype(np.int64)
    s = lab.astype(np.int64) @ cen
    bits = (s > 0) | ((s == 0) & (tie > 0)[None, :])
    return (bits & (lab.sum(1) > 0)[:, None]).astype(np.uint8)


def pack_bits(bits):
    """[B, K_tot] 0 / 1 -> uint32 [B, ceil(K_tot / 32)], bit k in word k >> 5 at position k & 31"""
    B, K = bits.shape
    Tw = (K + 31) // 32
    padded = np.zeros((B, Tw * 32), np.uint64)
    padded[:, :K] = bits
    return (padded.reshape(B, Tw, 32) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)


def pair_targets(bits, dtype):
    """hash_convert: bit b -> the pair (1, 0) for 0 and (0, 1) for 1: [B, K] -> [B, 2K]"""
    b = torch.as_tensor(np.asarray(bits)).to(dtype)
    return torch.stack([1 - b, b], -1).reshape(b.shape[0], -1)


def _split(lens, long, short):
    """the [B, 2 K_s] matrix of every stream"""
    out, at = [long], 0
    for k in lens[1:]:
        out.append(short[:, at:at + 2 * k])
        at += 2 * k
    return out


def loss(img_long, img_short, txt_long, txt_short, bits, lens, quan_alpha, low_rate, dtype=torch.float64):
    """-> the terms vector [1 + 6 n] of xmh_twdh_loss, in `dtype`"""
    n = len(lens)
    offs = np.concatenate([[0], np.cumsum(lens)])
    per = []
    for long, short in ((img_long, img_short), (txt_long, txt_short)):
        ps = _split(lens, torch.as_tensor(long).to(dtype), None if short is None else torch.as_tensor(short).to(dtype))
        for s, p in enumerate(ps):
            t = pair_targets(bits[:, offs[s]:offs[s + 1]], dtype)
            bce = -(t * torch.log(p).clamp(min=-100) + (1 - t) * torch.log(1 - p).clamp(min=-100)).mean()
            per += [bce, 1 - ((2 * p - 1) ** 2).mean()]
    means = []
    for s in range(n):
        means += [(per[2 * s] + per[2 * (n + s)]) / 2, (per[2 * s + 1] + per[2 * (n + s) + 1]) / 2]
    total = means[0] + quan_alpha * means[1]
    for s in range(1, n):
        total = total + low_rate * means[2 * s]
    for s in range(1, n):
        total = total + low_rate * means[2 * s + 1]
    return torch.stack([total] + per + means)


def loss_grad(long, short, bits, lens, quan_alpha, low_rate, up, dtype=torch.float64):
    """d total / d (long, short) of one modality, times `up`: the formula autograd's BCELoss backward evaluates"""
    offs = np.concatenate([[0], np.cumsum(lens)])
    ps = _split(lens, torch.as_tensor(long).to(dtype), None if short is None else torch.as_tensor(short).to(dtype))
    out = []
    for s, p in enumerate(ps):
        t = pair_targets(bits[:, offs[s]:offs[s + 1]], dtype)
        n = p.numel()
        wb, wq = (0.5, 0.5 * quan_alpha) if s == 0 else (0.5 * low_rate, 0.5 * low_rate)
        floor = torch.full_like(p, 1e-12)
        g = up * wb * (p - t) / torch.maximum((1 - p) * p, floor) / n + up * wq * (-4 * (2 * p - 1) / n)
        out.append(g)
    return out[0], (torch.cat(out[1:], 1) if len(out) > 1 else None)


def pair_softmax(z):
    zp = z.reshape(z.shape[0], -1, 2)
    e = torch.exp(zp - zp.max(-1, keepdim=True).values)
    return (e / e.sum(-1, keepdim=True)).reshape(z.shape)


def short_forward(long, T, dtype=torch.float64):
    return pair_softmax(torch.as_tensor(long).to(dtype) @ torch.as_tensor(T).to(dtype))


def short_backward(g, p, T, dtype=torch.float64):
    g, p = torch.as_tensor(g).to(dtype).reshape(p.shape[0], -1, 2), torch.as_tensor(p).to(dtype).reshape(p.shape[0], -1, 2)
    gz = (p * (g - (g * p).sum(-1, keepdim=True))).reshape(p.shape[0], -1)
    return gz @ torch.as_tensor(T).to(dtype).T


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def _probs(rng, B, K, scale=3.0):
    z = torch.tensor((rng.standard_normal((B, 2 * K)) * scale).astype(np.float32))
    return pair_softmax(z).numpy()


@functools.lru_cache(maxsize=None)
def build(name):
    """the inputs of a case, float32 / integer numpy arrays: labels, centres, ties, bits, the four probability matrices, the transform
    T_cat with its upstream.  Rows by design (where B allows): row 0 has no label, row 1 every label, rows 2.. at least some with an
    even number of labels (zero sums); row 2 of every probability matrix holds exact 0 / 1 pairs on and off target."""
    c = CASES[name]
    rng = np.random.default_rng(c["seed"])
    B, C, lens = c["B"], c["C"], c["lens"]
    labels = (rng.random((B, C)) < 0.1).astype(np.int64)
    labels[np.arange(B), rng.integers(0, C, B)] = 1
    if B >= 3:
        labels[0] = 0
        labels[1] = 1
        for r in range(2, B, 2):                                 # exactly two labels: every bit where the two centres differ is a tie
            labels[r] = 0
            labels[r, rng.choice(C, 2, replace=False) if C > 1 else [0]] = 1
    centres = [(rng.integers(0, 2, (C, k)) * 2 - 1).astype(np.int8) for k in lens]
    ties = [(rng.integers(0, 2, k) * 2 - 1).astype(np.int8) for k in lens]
    bits = targets(labels, centres, ties)
    ktot, S = sum(lens), sum(lens[1:])
    # logits of unit scale: every drawn probability lies within a few per cent of 0 and 1, so that in the ord_* tensors the quantisation
    # part (up to 4 w / n) is a few per cent of the largest BCE entry and an error in it, its weight or its upstream is far above rounding
    P = {k: _probs(rng, B, n, scale=1.0) for k, n in (("img_long", lens[0]), ("img_short", S), ("txt_long", lens[0]), ("txt_short", S))}
    row = 2 if B >= 3 else 0
    offs = np.concatenate([[0], np.cumsum(lens)])
    for m in ("img", "txt"):
        for s, k in enumerate(lens):
            mat, base = (P[m + "_long"], 0) if s == 0 else (P[m + "_short"], 2 * (offs[s] - lens[0]))
            for j in range(min(4, k)):                               # 0: on target, 1: off target, 2: (0, 1), 3: (1, 0)
                b = int(bits[row, offs[s] + j])
                on = {0: b, 1: 1 - b, 2: 1, 3: 0}[j]
                mat[row, base + 2 * j:base + 2 * j + 2] = (0.0, 1.0) if on else (1.0, 0.0)
    L2 = 2 * lens[0]
    T = (rng.standard_normal((L2, 2 * S)) * L2 ** -0.5).astype(np.float32)
    at = 0
    for k in lens[1:]:           # the first two pairs of every short length: logits 160 apart (the long pairs sum to 1: +160 / L per row)
        T[:, at] += 160.0 / lens[0]                                  # pair 0 -> (1, 0)
        T[:, at + 3] += 160.0 / lens[0]                              # pair 1 -> (0, 1)
        at += 2 * k
    g_short = rng.standard_normal((B, 2 * S)).astype(np.float32)
    return dict(c, name=name, labels=labels, centres=centres, ties=ties, bits=bits, ktot=ktot, T=T, g_short=g_short, **P)


def reference(name, dtype):
    """the restatement of everything the loss test compares, in `dtype`: terms, d_long / d_short per modality, p_short and g_long of
    the transform (of the image's long probabilities, with the case's upstream)"""
    c = build(name)
    out = {"terms": loss(c["img_long"], c["img_short"], c["txt_long"], c["txt_short"], c["bits"], c["lens"], c["quan_alpha"], c["low_rate"], dtype)}
    for m in ("img", "txt"):
        out["d_long_" + m], out["d_short_" + m] = loss_grad(c[m + "_long"], c[m + "_short"], c["bits"], c["lens"], c["quan_alpha"], c["low_rate"],
                                                            c["up"], dtype)
    out["p_short"] = short_forward(c["img_long"], c["T"], dtype)
    out["g_long"] = short_backward(c["g_short"], out["p_short"], c["T"], dtype)
    return expand(name, {k: v.double().numpy() for k, v in out.items()})


def composed(name, dtype):
    """the transforms feeding the objective: both modalities' short codes are pair_softmax(long @ T) -- with the pairs the offset
    columns saturate -- and the gradient reaches the long probabilities through both ways: terms, d_long_img, d_long_txt"""
    c = build(name)
    p = {m: short_forward(c[m + "_long"], c["T"], dtype) for m in ("img", "txt")}
    out = {"terms": loss(c["img_long"], p["img"], c["txt_long"], p["txt"], c["bits"], c["lens"], c["quan_alpha"], c["low_rate"], dtype)}
    for m in ("img", "txt"):
        dl, ds = loss_grad(c[m + "_long"], p[m], c["bits"], c["lens"], c["quan_alpha"], c["low_rate"], c["up"], dtype)
        out["d_long_" + m] = dl + short_backward(ds, p[m], c["T"], dtype)
    return expand(name, {k: v.double().numpy() for k, v in out.items()})


def term_key(i):
    """the name of scalar i of the terms vector: the total, a BCE mean (odd i) or a quantisation term (even i)"""
    return "term_total" if i == 0 else "term_%s_%02d" % ("bce" if i % 2 else "quan", i)


def saturated(p):
    """the entries of a probability matrix at which the BCE gradient's 1e-12 floor is hit (exact 0 / 1, or 1e-30)"""
    p = np.asarray(p, np.float64)
    return p * (1 - p) < 1e-12


def expand(name, vals):
    """what is compared, from the tensors of one evaluation of case `name` (restatement or port; None = not there): every scalar of
    `terms` under its own key (term_key), every gradient d_<which>_<m> as it is and, as ord_<which>_<m>, with the entries zeroed
    whose input probability is saturated"""
    c = build(name)
    out = {}
    for k, v in vals.items():
        if v is None:
            continue
        if k == "terms":
            v = np.asarray(v, np.float64)
            out.update({term_key(i): v[i:i + 1] for i in range(len(v))})
            continue
        out[k] = v
        if k.startswith("d_"):
            which, m = k[2:].split("_")
            out["ord" + k[1:]] = np.where(saturated(c["%s_%s" % (m, which)]), 0.0, v)
    return out


def kind_of(key):
    return next(k for k in KINDS if key.startswith(k))


@functools.lru_cache(maxsize=None)
def e_ref(name):
    """per tensor of `reference`: the float32 restatement's error against the float64 one"""
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


def compare(name, got, ref64=None, own=None):
    """prints e, the yardstick and their ratio for every tensor of `got`, then asserts e <= TOL_FACTOR * max(pool, e_ref) -> worst ratio"""
    ref64 = reference(name, torch.float64) if ref64 is None else ref64
    own = e_ref(name) if own is None else own
    rows = []
    for key, g in got.items():
        yard = max(pool().get(kind_of(key), 0.0), own.get(key, 0.0))
        e = rel_err(g, ref64[key])
        rows.append((key, e, yard))
        print("%-14s %-12s e %.3e  yardstick %.3e  ratio %.2f  bound %.3e" % (name, key, e, yard, e / yard if yard else float("inf"),
                                                                                TOL_FACTOR * yard))
    for key, e, yard in rows:
        assert np.asarray(got[key]).shape == ref64[key].shape, (name, key)
        assert e <= TOL_FACTOR * yard, (name, key, e, yard)
    return max((e / yard if yard else float("inf")) for _, e, yard in rows)


# ---- the chain head -> transforms -> objective ---------------------------------------------------------------------------------------
HEAD_PARAMS = ("in_w", "in_b", "out_w", "out_b", "norm_w", "norm_b", "w2", "b2")
HEAD_KEYS = {"in_w": "atten.in_proj_weight", "in_b": "atten.in_proj_bias", "out_w": "atten.out_proj.weight", "out_b": "atten.out_proj.bias",
             "norm_w": "norm.weight", "norm_b": "norm.bias", "w2": "fc2.weight", "b2": "fc2.bias"}
EPS32 = float(np.finfo(np.float32).eps)
TIE_FACTOR = 8.0                     # oracle/heads_train.py's near-tie band of a relu input: |z64| <= TIE_FACTOR eps32 |n| |w2|


def draw_head(seed, K, bn, e):
    """parameters of one modality head away from their initial values, float32 (the recipe of oracle/heads_train.py:draw_dcmht)"""
    rng = np.random.default_rng(seed)
    u = lambda shape, a: ((rng.random(shape) * 2.0 - 1.0) * a).astype(np.float32)      # noqa: E731
    a = 1.0 / np.sqrt(e)
    return {"in_w": u((3 * e, e), 1.5 * a), "in_b": u((3 * e,), 0.1), "out_w": u((e, e), 1.5 * a), "out_b": u((e,), 0.1),
            "norm_w": 1.0 + u((e,), 0.3), "norm_b": u((e,), 0.2), "w2": u((2 * K, e), 2.0 * a), "b2": u((2 * K,), 0.1)}


def head(x, P, bn, dtype, mask=None, eps=1e-5):
    """the DCMHT modality head in train mode (batch statistics) on torch tensors with a graph -> (probs, z, tie band, relu mask)"""
    e = x.shape[1]
    v = x @ P["in_w"][2 * e:].T + P["in_b"][2 * e:]
    o = v @ P["out_w"].T + P["out_b"]
    ax = 0 if bn else 1
    mu = o.mean(ax, keepdim=True)
    var = ((o - mu) ** 2).mean(ax, keepdim=True)
    n = (o - mu) / torch.sqrt(var + eps) * P["norm_w"] + P["norm_b"]
    z = n @ P["w2"].T + P["b2"]
    tie = TIE_FACTOR * EPS32 * n.detach().norm(dim=1)[:, None] * P["w2"].detach().norm(dim=1)[None, :]
    m = (z.detach() > 0) if mask is None else torch.as_tensor(mask)
    f = torch.where(m, z, torch.zeros_like(z))
    return pair_softmax(f), z.detach(), tie, m


def chain(x, P, T, bits, lens, quan_alpha, low_rate, dtype, masks=None):
    """x / P: {"img" / "txt": embeddings [B, e] / head parameters}, float32 numpy.  The whole chain in `dtype` with torch's autograd ->
    dict: loss, terms, g_x_<m>, g_<param>_<m>, and z / tie / mask per modality for the near-tie rule"""
    xs = {m: torch.tensor(x[m]).to(dtype).requires_grad_(True) for m in x}
    Ps = {m: {k: torch.tensor(v).to(dtype).requires_grad_(True) for k, v in P[m].items()} for m in P}
    Tt = torch.tensor(T).to(dtype)
    out, longs, shorts = {}, {}, {}
    for m in ("img", "txt"):
        longs[m], out["z_" + m], out["tie_" + m], out["mask_" + m] = head(xs[m], Ps[m], m == "img", dtype, None if masks is None else masks[m])
        shorts[m] = pair_softmax(longs[m] @ Tt)
    offs = np.concatenate([[0], np.cumsum(lens)])
    total = 0
    for s in range(len(lens)):
        for term in range(2):
            v = 0
            for m in ("img", "txt"):
                p = longs[m] if s == 0 else shorts[m][:, 2 * (offs[s] - lens[0]):2 * (offs[s + 1] - lens[0])]
                if term == 0:
                    # BCELoss with the backward torch gives it: a custom Function keeps the (p - t) / max(p (1 - p), 1e-12) form
                    v = v + _BCE.apply(p, pair_targets(bits[:, offs[s]:offs[s + 1]], dtype))
                else:
                    v = v + (1 - ((2 * p - 1) ** 2).mean())
            w = (1.0 if term == 0 else quan_alpha) if s == 0 else low_rate
            total = total + w * v / 2
    total.backward()
    out["loss"] = total.detach()
    for m in ("img", "txt"):
        out["g_x_" + m] = xs[m].grad
        for k in HEAD_PARAMS:
            out["g_%s_%s" % (k, m)] = Ps[m][k].grad
    return {k: (v.double().numpy() if v.dtype != torch.bool else v.numpy()) for k, v in out.items()}


class _BCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p, t):
        ctx.save_for_backward(p, t)
        return -(t * torch.log(p).clamp(min=-100) + (1 - t) * torch.log(1 - p).clamp(min=-100)).mean()

    @staticmethod
    def backward(ctx, g):
        p, t = ctx.saved_tensors
        return g * (p - t) / torch.maximum((1 - p) * p, torch.full_like(p, 1e-12)) / p.numel(), None
