"""Cases, seeded draws and float64 restatements of UMoED (reference models/UMoED): the soft-MoE decoder head (hash/hash_moe.py,
hash/block/transformer.py, hash/block/SoftMoe.py, models/common/hash.py) and the pairwise objective (UMoED.py similarity_loss with
distance/__init__.py pairwise_distance and DIMCH's loss/triplet_loss.py), shared by tests/test_umoed_cpu.py, tests/test_gpu_umoed_head.py,
tests/test_gpu_umoed_loss.py and tools/make_golden_umoed.py.

The restatements are written from the formulas, in torch on the CPU with the dtype as a parameter and torch's autograd
for the gradients: float64 is the truth the GPU tests compare with, float32 on the same inputs is the yardstick.  Parameters and
inputs are never stored: they are drawn here from a seed (``head_params``, ``head_case``, ``loss_case``), and the golden file holds
what the unmodified reference made of the same draws.

Error rule: per tensor e = max|got - f64| / max|f64| <= TOL_FACTOR * max(e_ref, pool), e_ref the float32 restatement's (or the
reference's) e on the same inputs, pool the largest e_ref of that tensor kind over the cases.

Guards.  Head: a case is redrawn until, in float64, every row's two largest logits are at least 1e-3 of the row's largest |logit| apart
(linear_subspace), so that every code bit can be compared.  Objective: redrawn until no hinge argument of a live triplet and no
similarity under the clamp lies within 1e-5 of zero."""
import functools
import math
import os
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

TOL_FACTOR = 4.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "umoed.npz")
HEAD_GAP = 1e-3

# ---- the head ----------------------------------------------------------------------------------------------------------------------------
# B, T, E, d, heads, M, layers, n x p, F, V, moe, hash_func + merge_func.  "fusion": the tokens of 5 image and 4 text rows stacked along T.
HEAD_CASES = {
    "golden": dict(B=2, T=5, E=128, d=128, heads=2, M=3, layers=2, n=2, p=2, F=2048, V=2, moe=True, hash_func="linear_subspace", seed=7101),
    "odd_slots": dict(B=1, T=50, E=128, d=128, heads=2, M=64, layers=1, n=3, p=5, F=2048, V=16, moe=True, hash_func="linear_subspace", seed=7102),
    "depth": dict(B=37, T=32, E=128, d=128, heads=2, M=8, layers=6, n=8, p=8, F=96, V=2, moe=True, hash_func="linear_subspace", seed=7103),
    "workload_slice": dict(B=2, T=50, E=512, d=512, heads=8, M=64, layers=2, n=8, p=8, F=2048, V=2, moe=True, hash_func="linear_subspace",
                           seed=7104),
    "fusion": dict(B=2, T=9, T_img=5, E=128, d=128, heads=2, M=3, layers=2, n=2, p=2, F=2048, V=2, moe=True, hash_func="linear_subspace",
                   seed=7105),
    "plain": dict(B=2, T=5, E=192, d=128, heads=2, M=3, layers=2, n=0, p=0, F=2048, V=16, moe=False, hash_func="tanh", seed=7106),
}
GOLDEN_HEAD_CASES = ("golden", "fusion", "plain")             # F = 2048 and a route the reference has: it can build these
MERGE_OF = {"linear_subspace": "concatenate", "tanh": "mean", "softmax": "mean"}
# the two module configurations whose state-dict keys and shapes the golden file records: (constructor arguments of HashLayer)
STATE_CONFIGS = {
    "moe_fusion": dict(visual_tokens=50, txt_tokens=32, img_feature_size=512, txt_feature_size=512, outputDim=2, setDim=64, decoder_heads=8,
                       decoder_layers=2, num_experts=8, slots_per_expert=8, MoE=True, fusion=True, hidden_dim=512, hash_func_="linear_subspace",
                       merge_func_="concatenate"),
    "plain_split": dict(visual_tokens=50, txt_tokens=32, img_feature_size=512, txt_feature_size=512, outputDim=16, setDim=8, decoder_heads=4,
                        decoder_layers=2, MoE=False, fusion=False, hidden_dim=256, hash_func_="tanh", merge_func_="mean"),
}


def rel_err(got, want):
    """max|got - want| / max|want| (absolute where the reference tensor is identically zero)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = np.abs(want).max() if want.size else 0.0
    return float(np.abs(got - want).max() / (scale if scale > 0 else 1.0)) if want.size else 0.0


def head_shapes(c):
    """TokenHash's state-dict names -> shapes, in the reference's order"""
    d, E, F_, M, V = c["d"], c["E"], c["F"], c["M"], c["V"]
    out = OrderedDict()
    out["decoder_learned_parameters"] = (M, d)
    for i in range(c["layers"]):
        pre = "decoder.layers.%d." % i
        attn = lambda nm: [(pre + nm + ".in_proj_weight", (3 * d, d)), (pre + nm + ".in_proj_bias", (3 * d,)),           # noqa: E731
                           (pre + nm + ".out_proj.weight", (d, d)), (pre + nm + ".out_proj.bias", (d,))]
        norm = lambda nm: [(pre + nm + ".weight", (d,)), (pre + nm + ".bias", (d,))]                                      # noqa: E731
        if c["moe"]:
            items = norm("norm1") + attn("self_attn") + norm("norm2") + attn("multihead_attn") + norm("norm3") + [
                (pre + "linear.weight", (F_, d)), (pre + "linear.bias", (F_,)), (pre + "moe.phi", (F_, c["n"], c["p"])),
                (pre + "moe.experts.weight", (c["n"], F_, d)), (pre + "moe.experts.bias", (c["n"], d))]
        else:
            items = attn("self_attn") + attn("multihead_attn") + [
                (pre + "linear1.weight", (F_, d)), (pre + "linear1.bias", (F_,)), (pre + "linear2.weight", (d, F_)), (pre + "linear2.bias", (d,))
            ] + norm("norm1") + norm("norm2") + norm("norm3")
        out.update(items)
    if d != E:
        out["first_layer.weight"], out["first_layer.bias"] = (d, E), (d,)
    out["classifier.weight"], out["classifier.bias"] = (V, d), (V,)
    return out


def head_params(c, seed):
    """name -> float32 array, drawn from `seed` in the order of head_shapes: weights N(0, 1 / fan_in) (the experts' and phi's fan-in is
    F), biases 0.1 N(0, 1), LayerNorm gains 1 + 0.1 N(0, 1), the learned rows N(0, 1)"""
    rng = np.random.default_rng(seed)
    P = OrderedDict()
    for name, shape in head_shapes(c).items():
        z = rng.standard_normal(shape).astype(np.float32)
        if name == "decoder_learned_parameters":
            P[name] = z
        elif ".norm" in name and name.endswith("weight"):
            P[name] = (1 + np.float32(0.1) * z).astype(np.float32)
        elif name.endswith("bias"):
            P[name] = np.float32(0.1) * z
        elif name.endswith("moe.phi"):
            P[name] = z * np.float32(1 / math.sqrt(shape[0]))
        elif name.endswith("experts.weight"):
            P[name] = z * np.float32(1 / math.sqrt(shape[1]))
        else:
            P[name] = z * np.float32(1 / math.sqrt(shape[-1]))
    return P


def _mha(q_in, kv_in, in_w, in_b, out_w, out_b, heads):
    d = q_in.shape[-1]
    dh = d // heads
    q = q_in @ in_w[:d].t() + in_b[:d]
    k = kv_in @ in_w[d:2 * d].t() + in_b[d:2 * d]
    v = kv_in @ in_w[2 * d:].t() + in_b[2 * d:]
    split = lambda t: t.reshape(t.shape[0], t.shape[1], heads, dh).transpose(1, 2)            # noqa: E731
    s = (split(q) / math.sqrt(dh)) @ split(k).transpose(-1, -2)
    o = (torch.softmax(s, dim=-1) @ split(v)).transpose(1, 2).reshape(q.shape)
    return o @ out_w.t() + out_b


def linear_subspace_bits(embeds):
    """[B, M, V] -> [B, M log2 V]: the argmax (first index on a tie) as bits, most significant first, 1 -> +1, 0 -> -1"""
    B, M, V = embeds.shape
    bits = int(math.log2(V))
    idx = torch.argmax(embeds, dim=-1)
    sh = torch.arange(bits - 1, -1, -1)
    return (((idx.unsqueeze(-1) >> sh) & 1).to(embeds.dtype) * 2 - 1).reshape(B, M * bits)


def head(tokens, P, c, dtype):
    """the head of one modality in torch on the CPU: tokens [B, T, E], P head_params -> {"embeds" [B, M, V], "code"} float64 numpy,
    computed in `dtype`"""
    W = {k: torch.tensor(np.asarray(v)).to(dtype) for k, v in P.items()}
    mem = torch.tensor(np.asarray(tokens)).to(dtype)
    d, eps = c["d"], 1e-5
    if "first_layer.weight" in W:
        mem = F.relu(mem @ W["first_layer.weight"].t() + W["first_layer.bias"])
    x = W["decoder_learned_parameters"].unsqueeze(0).repeat(mem.shape[0], 1, 1)
    for i in range(c["layers"]):
        g = lambda nm: W["decoder.layers.%d.%s" % (i, nm)]                                    # noqa: E731
        ln = lambda t, nm: F.layer_norm(t, (d,), g(nm + ".weight"), g(nm + ".bias"), eps)     # noqa: E731
        at = lambda nm, q, kv: _mha(q, kv, g(nm + ".in_proj_weight"), g(nm + ".in_proj_bias"), g(nm + ".out_proj.weight"),      # noqa: E731
                                    g(nm + ".out_proj.bias"), c["heads"])
        x = ln(x + at("self_attn", x, x), "norm1")
        x = ln(x + at("multihead_attn", x, mem), "norm2")
        if c["moe"]:
            h = F.relu(x @ g("linear.weight").t() + g("linear.bias"))                          # [B, M, F]
            S = c["n"] * c["p"]
            logits = h @ g("moe.phi").reshape(-1, S)                                          # [B, M, S]
            Dw, Cw = torch.softmax(logits, dim=1), torch.softmax(logits, dim=2)
            Xs = Dw.transpose(1, 2) @ h                                                       # [B, S, F]
            Xs = Xs.reshape(Xs.shape[0], c["n"], c["p"], -1)
            Ys = torch.einsum("bnpf,nfd->bnpd", Xs, g("moe.experts.weight")) + g("moe.experts.bias")[None, :, None, :]
            x = ln(x + Cw @ Ys.reshape(Ys.shape[0], S, d), "norm3")
        else:
            h = F.relu(x @ g("linear1.weight").t() + g("linear1.bias"))
            x = ln(x + h @ g("linear2.weight").t() + g("linear2.bias"), "norm3")
    embeds = x @ W["classifier.weight"].t() + W["classifier.bias"]
    if c["hash_func"] == "linear_subspace":
        code = linear_subspace_bits(embeds)
    else:
        pooled = embeds.mean(1)
        code = torch.tanh(pooled) if c["hash_func"] == "tanh" else torch.softmax(pooled.reshape(pooled.shape[0], -1, 2), dim=-1).reshape(pooled.shape)
    return {"embeds": embeds.double().numpy(), "code": code.double().numpy()}


def head_gap(embeds):
    """the smallest (top-1 - top-2) / max|logit| over the rows of embeds [B, M, V]"""
    e = np.asarray(embeds, np.float64)
    top = np.sort(e, axis=-1)
    return float(((top[..., -1] - top[..., -2]) / np.abs(e).max(-1)).min())


@functools.lru_cache(maxsize=None)
def head_case(name):
    """the drawn inputs of HEAD_CASES[name]: {"P", "x", "gap", "seed", ...spec}; redrawn (seed + 1000, ...) until head_gap >= HEAD_GAP for
    the linear_subspace route"""
    spec = HEAD_CASES[name]
    for attempt in range(40):
        seed = spec["seed"] + 1000 * attempt
        P = head_params(spec, seed)
        x = np.random.default_rng(seed + 500).standard_normal((spec["B"], spec["T"], spec["E"])).astype(np.float32)
        gap = head_gap(head(x, P, spec, torch.float64)["embeds"])
        if spec["hash_func"] != "linear_subspace" or gap >= HEAD_GAP:
            return dict(spec, name=name, seed=seed, P=P, x=x, gap=gap)
    raise AssertionError("no guarded draw for %r" % (spec,))


@functools.lru_cache(maxsize=None)
def head_reference(name, dtype=torch.float64):
    c = head_case(name)
    return head(c["x"], c["P"], c, dtype)


@functools.lru_cache(maxsize=None)
def head_pool():
    """the largest float32-against-float64 error of the restatement's embeds (and of a tanh / softmax code) over HEAD_CASES"""
    out = {"embeds": 0.0, "code": 0.0}
    for name in HEAD_CASES:
        r64, r32 = head_reference(name), head_reference(name, torch.float32)
        out["embeds"] = max(out["embeds"], rel_err(r32["embeds"], r64["embeds"]))
        if HEAD_CASES[name]["hash_func"] != "linear_subspace":
            out["code"] = max(out["code"], rel_err(r32["code"], r64["code"]))
    return out


# ---- the objective -----------------------------------------------------------------------------------------------------------------------
# configs/UMoED/config.yaml of the reference
CONFIG = dict(extreme=True, extreme_T=0.3, token_triplet_margin=0.1, triplet_alpha=1.0, unif_alpha=0.8)
CONST_KEYS = tuple(CONFIG)
TERMS = ("loss", "T_i2t", "T_t2i", "U_img", "U_txt")
INPUTS = ("e_img", "e_txt")
GRADS = ("g_e_img", "g_e_txt")
KINDS = ("loss", "T", "U", "g_e")
# name -> B, M, V, C, overrides of CONFIG, upstream.  (7, 5, 2, 4) with and without the softmax; (20, 8, 16, 6); (9, 64, 2, 5): the
# configuration's set size and vocabulary; (6, 1, 2, 3): sets of one, U = 0; same_set: sample 2's text set is its image set and its token
# row 1 a copy of row 0 (D[2][2] = 0 without the softmax, a squared distance of exactly 0 in U); (258, 3, 2, 1): more columns of an anchor
# row than threads, with C = 1 (no negative: the triplet terms are 0) and the softmax on, so that no similarity is near the clamp.
LOSS_CASES = {
    "b7_m5_v2_extreme": dict(B=7, M=5, V=2, C=4, up=1.0, seed=7201),
    "b7_m5_v2_plain": dict(B=7, M=5, V=2, C=4, up=1.0, seed=7202, extreme=False),
    "b20_m8_v16": dict(B=20, M=8, V=16, C=6, up=0.37, seed=7203),
    "b9_m64_v2": dict(B=9, M=64, V=2, C=5, up=1.0, seed=7204),
    "b6_m1_v2": dict(B=6, M=1, V=2, C=3, up=1.0, seed=7205, extreme=False),
    "b7_m5_v4_same_set": dict(B=7, M=5, V=4, C=4, up=2.5, seed=7206, extreme=False, same_set=True),
    "b258_m3_v2_c1": dict(B=258, M=3, V=2, C=1, up=1.0, seed=7207),
}
SAME_ROW = 2
GOLDEN_LOSS_CASES = {
    "g_extreme": dict(B=7, M=5, V=2, C=4, seed=7301),
    "g_plain": dict(B=7, M=5, V=2, C=4, seed=7302, extreme=False),
    "g_v16": dict(B=20, M=8, V=16, C=6, seed=7303),
    "g_m64": dict(B=9, M=64, V=2, C=5, seed=7304),
}


def consts(c):
    return {k: c.get(k, CONFIG[k]) for k in CONST_KEYS}


def triplet_term(D, labels, margin, probe=None):
    """T(D, m): c = label overlap, sim = c > 0, Z[a] = sum_j (2^c_(j) - 1) / log2(j + 2) over row a sorted descending, w = (2^c - 1) / Z,
    t[a][p][n] = (w[a][p] - w[a][n]) sim[a][p] (1 - sim[a][n]) (D[a][p] - D[a][n] + m), T = sum max(t, 0) / (#{t > 1e-16} + 1e-16).
    probe: receives the smallest |hinge argument| of a live triplet"""
    B = D.shape[0]
    so = labels @ labels.t()
    sim = (so > 0).to(D.dtype)
    ideal = torch.sort(so, dim=1, descending=True)[0]
    th = torch.log2(torch.arange(0.0, B) + 2).repeat(B, 1)          # float32 logarithms in every dtype, as the reference's
    Z = ((2 ** ideal - 1) / th).sum(1).reshape(-1, 1)
    w = (2 ** so - 1) / Z
    t = D.unsqueeze(2) - D.unsqueeze(1) + margin
    mask = sim.unsqueeze(2) * (1 - sim.unsqueeze(1))
    weight = w.unsqueeze(2) - w.unsqueeze(1)
    if probe is not None:
        live = (mask > 0) & (weight.detach() != 0)
        if live.any():
            probe["hinge"] = min(probe.get("hinge", np.inf), float(t.detach()[live].abs().min()))
    t = (weight * mask * t).clamp(0)
    return t.sum() / (t.gt(1e-16).to(D.dtype).sum() + 1e-16)


def objective_terms(e_img, e_txt, labels, cst, probe=None):
    """torch tensors of one dtype -> the five TERMS, a tensor with a graph"""
    dtype, M = e_img.dtype, e_img.shape[1]
    lab = torch.as_tensor(labels).to(dtype)
    x, y = F.normalize(e_img, dim=-1), F.normalize(e_txt, dim=-1)
    a, b = (torch.softmax(x / cst["extreme_T"], dim=-1), torch.softmax(y / cst["extreme_T"], dim=-1)) if cst["extreme"] else (x, y)
    dots = torch.einsum("btl,ktl->btk", a, b)
    if probe is not None:
        probe["clamp"] = float(dots.detach().abs().min())
    D = (1 - dots.clamp(min=0)).mean(dim=1)
    T_i2t = triplet_term(D, lab, cst["token_triplet_margin"], probe)
    T_t2i = triplet_term(D.t(), lab, cst["token_triplet_margin"], probe)

    def unif(u):
        if M == 1:
            return torch.zeros((), dtype=dtype)
        q = (u.unsqueeze(2) - u.unsqueeze(1)).pow(2).sum(-1)       # [B, M, M] squared distances
        return (torch.exp(-20 * q).triu(1).sum((1, 2)) / (M * (M - 1) * 0.5)).mean()
    U_i, U_t = unif(x), unif(y)
    loss = cst["triplet_alpha"] * ((T_i2t + T_t2i) / 4) + cst["unif_alpha"] * ((U_i + U_t) / 3)
    return torch.stack([loss, T_i2t, T_t2i, U_i, U_t])


def objective(c, dtype, up=None, probe=None, **over):
    """case dict (numpy inputs) -> {terms..., g_*: gradients of up * loss} as float64 numpy, computed in `dtype`"""
    leaves = {k: torch.tensor(c[k]).to(dtype).requires_grad_(True) for k in INPUTS}
    terms = objective_terms(leaves["e_img"], leaves["e_txt"], torch.tensor(c["labels"]), dict(consts(c), **over), probe)
    (terms[0] * (c.get("up", 1.0) if up is None else up)).backward()
    out = {k: terms[i].detach().double().numpy().reshape(1) for i, k in enumerate(TERMS)}
    for g, k in zip(GRADS, INPUTS):
        out[g] = leaves[k].grad.double().numpy()
    return out


def kind_of(key):
    return "loss" if key == "loss" else ("g_e" if key.startswith("g_") else key[0])


def _draw_loss(B, M, V, C, seed, same_set=False, density=0.3, **rest):
    rng = np.random.default_rng(seed)
    labels = (rng.random((B, C)) < density).astype(np.int64)
    labels[np.arange(B), rng.integers(0, C, B)] = 1              # every row has a label: one without makes the loss NaN
    e = {m: rng.standard_normal((B, M, V)).astype(np.float32) for m in ("img", "txt")}
    if same_set:
        e["img"][SAME_ROW, 1] = e["img"][SAME_ROW, 0]
        e["txt"][SAME_ROW] = e["img"][SAME_ROW]
    return dict(rest, B=B, M=M, V=V, C=C, seed=seed, same_set=same_set, labels=labels, e_img=e["img"], e_txt=e["txt"])


def guards(c):
    """-> {"hinge", "clamp"}: the float64 distances from the kinks; "hinge" is absent where no triplet is live"""
    probe = {}
    objective(c, torch.float64, probe=probe)
    return probe


def guarded(probe):
    return probe.get("hinge", np.inf) >= 1e-5 and probe["clamp"] >= 1e-5


def draw_loss(seed, **spec):
    for attempt in range(40):
        c = _draw_loss(seed=seed + 1000 * attempt, **spec)
        if guarded(guards(c)):
            return c
    raise AssertionError("no guarded draw for %r" % (spec,))


@functools.lru_cache(maxsize=None)
def loss_case(name):
    return dict(draw_loss(**LOSS_CASES[name]), name=name)


@functools.lru_cache(maxsize=None)
def loss_reference(name, dtype=torch.float64):
    return objective(loss_case(name), dtype)


@functools.lru_cache(maxsize=None)
def loss_e_ref(name):
    r64, r32 = loss_reference(name, torch.float64), loss_reference(name, torch.float32)
    return {k: rel_err(r32[k], r64[k]) for k in r64}


@functools.lru_cache(maxsize=None)
def loss_pool():
    out = {k: 0.0 for k in KINDS}
    for name in LOSS_CASES:
        for key, e in loss_e_ref(name).items():
            out[kind_of(key)] = max(out[kind_of(key)], e)
    return out


def compare(what, got, ref64, own, pool):
    """prints e, the yardstick max(pool of the tensor's kind, own e_ref) and their ratio for every tensor of `got`, then asserts
    e <= TOL_FACTOR * yardstick -> worst ratio.  pool: kind (or key) -> float"""
    rows = []
    for key, g in got.items():
        yard = max(pool.get(kind_of(key), pool.get(key, 0.0)), own.get(key, 0.0))
        e = rel_err(g, ref64[key])
        rows.append((key, e, yard))
        print("%-24s %-8s e %.3e  yardstick %.3e  ratio %.2f  own e_ref %.3e" % (what, key, e, yard, e / yard if yard else float("inf"), own.get(key, 0.0)))
    for key, e, yard in rows:
        assert np.asarray(got[key]).shape == np.asarray(ref64[key]).shape, (what, key)
        assert e <= TOL_FACTOR * yard, (what, key, e, yard)
    return max((e / yard if yard else float("inf")) for _, e, yard in rows)
