"""Cases and restatement of DIMCH's training objective (reference models/DIMCH/DIMCH.py:152-234, distance/distance.py,
loss/triplet_loss.py:16-88) and, at the end, of its token-set head (models/DIMCH/hash/hash.py), shared by tests/test_dimch_cpu.py,
tests/test_gpu_dimch_loss.py, tests/test_gpu_dimch_head.py, tools/make_golden_dimch.py and tools/bench_dimch_step.py.

The restatement is written from the reference's expressions, in torch on the CPU with torch's autograd for the gradients, with the
dtype as a parameter: float64 is the truth the GPU tests compare with, float32 on the same inputs is the yardstick (e_ref).  It never
builds the reference's [N, N, N] tensor: batchwise_uniformity_loss on the flattened [N, K] rows evaluates to the strict upper
triangle of exp(-20 cdist^2) over M (M - 1) / 2, and that is what is written here.  Distances are torch.cdist's, as the reference's,
so that the float64 numbers are the reference's to rounding.

Error rule (tests/test_gpu_dnph_loss.py's): per tensor e = max|got - f64| / max|f64|; the port must stay within TOL_FACTOR *
max(pool, e_ref), e_ref the float32 restatement's e on the same inputs and pool the largest e_ref of that tensor kind over CASES.

Every case of the pool is drawn until, in float64, every hinge argument of a masked triplet and every 1 - s is at least 1e-5 from
zero and, in chamfer and max mode, the two largest entries behind every maximum are at least 1e-4 apart (guards): nearer than that
a float32 evaluation may legitimately land on the other side of a kink."""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

TOL_FACTOR = 4.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dimch.npz")
MODES = ("smooth_chamfer", "chamfer", "max", "avg")
HASH_FUNCS = ("tanh", "softmax")
# configs/DIMCH/config.yaml of the reference
CONFIG = dict(mode="smooth_chamfer", denominator=2.0, temperature=16.0, temperature_txt_scale=1.0, token_triplet_margin=0.3,
              triplet_margin=0.3, mmd_gamma=0.5, triplet_alpha=50.0, mmd_alpha=1.0, unif_alpha=0.3, hash_triplet_alpha=50.0, quan_alpha=1.0,
              hash_func="tanh")
CONST_KEYS = tuple(CONFIG)

TERMS = ("loss", "T_i2t", "T_t2i", "mmd", "unif", "Th_i2t", "Th_t2i", "Q_img", "Q_txt")
INPUTS = ("e_img", "e_txt", "h_img", "h_txt")
GRADS = ("g_e_img", "g_e_txt", "g_h_img", "g_h_txt")
KINDS = ("loss", "T", "mmd", "unif", "Q", "g_e", "g_h")          # T: the four triplet terms, Q: the two quantisation terms

# name -> B, M, K (Kh = K), C, overrides of CONFIG, upstream.  (3, 1, 16): sets of one, U = 0; (7, 5, 6): odd everything, all four
# modes; (20, 8, 16): the configuration's shape; (9, 64, 32): M at the tile edge; (33, 8, 64): B past one wave's half; (65, 3, 130): N
# and K off every multiple, two label words.  C = 1 (no negative anywhere: every triplet term is 0), 24, 80, 127.
# (5, 4, 100): two 64-column slots of K a thread; (258, 2, 8): more columns of an anchor row than threads, the owner's loop in one part; with C = 1, because among the
# millions of live triplets of such a batch some hinge argument always lies within 1e-5 of zero.
# clamp: sample 2's text tokens are its image tokens, so s > 1 there and clamp(1 - s, 0) is active.
CASES = {
    "b3_m1_k16": dict(B=3, M=1, K=16, C=24, up=1.0, seed=6101),
    "b7_m5_k6_smooth": dict(B=7, M=5, K=6, C=24, up=1.0, seed=6102),
    "b7_m5_k6_chamfer": dict(B=7, M=5, K=6, C=24, up=1.0, seed=6103, mode="chamfer"),
    "b7_m5_k6_max": dict(B=7, M=5, K=6, C=24, up=1.0, seed=6104, mode="max"),
    "b7_m5_k6_avg": dict(B=7, M=5, K=6, C=24, up=1.0, seed=6105, mode="avg"),
    "b20_m8_k16": dict(B=20, M=8, K=16, C=80, up=1.0, seed=6106),
    "b9_m64_k32": dict(B=9, M=64, K=32, C=24, up=0.37, seed=6107),
    "b33_m8_k64": dict(B=33, M=8, K=64, C=127, up=1.0, seed=6108),
    "b65_m3_k130": dict(B=65, M=3, K=130, C=80, up=2.5, seed=6109),
    "b7_m5_k6_c1": dict(B=7, M=5, K=6, C=1, up=1.0, seed=6110),
    "b20_m8_k16_softmax": dict(B=20, M=8, K=16, C=24, up=1.0, seed=6111, hash_func="softmax"),
    "b20_m8_k16_sigma": dict(B=20, M=8, K=16, C=24, up=1.0, seed=6112, temperature_txt_scale=0.6),
    "b7_m5_k6_clamp": dict(B=7, M=5, K=6, C=24, up=1.0, seed=6113, clamp=True, temperature=4.0),
    "b5_m4_k100": dict(B=5, M=4, K=100, C=24, up=1.0, seed=6114),
    "b258_m2_k8_c1": dict(B=258, M=2, K=8, C=1, up=1.0, seed=6115),
}
CLAMP_ROW = 2
GOLDEN_CASES = {
    "g_smooth": dict(B=7, M=5, K=6, C=24, seed=6201),
    "g_chamfer": dict(B=7, M=5, K=6, C=24, seed=6202, mode="chamfer"),
    "g_max": dict(B=7, M=5, K=6, C=24, seed=6203, mode="max"),
    "g_avg": dict(B=7, M=5, K=6, C=24, seed=6204, mode="avg"),
    "g_config": dict(B=20, M=8, K=16, C=80, seed=6205),
    "g_m64": dict(B=9, M=64, K=32, C=24, seed=6206),
    "g_softmax": dict(B=7, M=5, K=6, C=24, seed=6207, hash_func="softmax"),
}


def rel_err(got, want):
    """max|got - want| / max|want| (absolute where the reference tensor is identically zero)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = np.abs(want).max() if want.size else 0.0
    return float(np.abs(got - want).max() / (scale if scale > 0 else 1.0)) if want.size else 0.0


def consts(c):
    """the constants of a case: CONFIG with the case's overrides"""
    return {k: c.get(k, CONFIG[k]) for k in CONST_KEYS}


# ---- restatement -------------------------------------------------------------------------------------------------------------------
def _trace(probe, key, value):
    """a probe that holds a dict under "trace" receives, per key, the list of every array behind the probe's minima (float64 numpy, in
    call order; NaN where a triplet is not live): tests/dimch_train_step_cases.py compares them between two dtypes"""
    if probe.get("trace") is not None:
        probe["trace"].setdefault(key, []).append(value.double().numpy().copy())


def set_similarity(u, v, M, cst, probe=None):
    """u, v [N, K] normalised -> s(u, v) [B, B].  probe: a dict that receives the smallest top-2 gap behind a maximum"""
    N = u.shape[0]
    B = N // M
    G = (u @ v.t()).view(B, M, B, M)                             # [i, a, j, b]
    mode, den = cst["mode"], cst["denominator"]
    if "smooth" in mode:
        t1 = cst["temperature"]
        ts = t1 * cst["temperature_txt_scale"]
        right = torch.logsumexp(ts * G, dim=3).sum(1)
        left = torch.logsumexp(t1 * G, dim=1).sum(2)
        return (right / (M * ts) + left / (M * t1)) / den
    if "chamfer" in mode:
        if probe is not None and M > 1:
            for d in (3, 1):
                top = torch.topk(G.detach(), 2, dim=d).values
                probe["gap"] = min(probe.get("gap", np.inf), float((top.select(d, 0) - top.select(d, 1)).min()))
                _trace(probe, "gap", top.select(d, 0) - top.select(d, 1))
        return (G.max(dim=3).values.sum(1) / M + G.max(dim=1).values.sum(2) / M) / den
    flat = G.permute(0, 2, 1, 3).reshape(B, B, M * M)
    if "max" in mode:
        if probe is not None and M > 1:
            top = torch.topk(flat.detach(), 2, dim=2).values
            probe["gap"] = min(probe.get("gap", np.inf), float((top[..., 0] - top[..., 1]).min()))
        return flat.max(dim=2).values
    return torch.sigmoid(flat).mean(2)


def triplet_term(D, labels, margin, probe=None):
    """the reference's TripletLoss(reduction="mean") with _get_triplet_mask.  probe: receives the smallest |hinge argument| of a
    masked triplet with a non-zero weight"""
    B = D.shape[0]
    so = labels @ labels.t()
    sim = (so > 0).to(D.dtype)
    ideal = torch.sort(so, dim=1, descending=True)[0]
    th = torch.log2(torch.arange(0.0, B, device=D.device) + 2).repeat(B, 1)   # float32 logarithms in every dtype, as the reference's;
                                                                              # made on D's device: no host copy inside a timed step
    Z = ((2 ** ideal - 1) / th).sum(1).reshape(-1, 1)
    w = (2 ** so - 1) / Z
    t = D.unsqueeze(2) - D.unsqueeze(1) + margin
    mask = sim.unsqueeze(2) * (1 - sim.unsqueeze(1))
    weight = w.unsqueeze(2) - w.unsqueeze(1)
    if probe is not None:
        live = (mask > 0) & (weight.detach() != 0)
        if live.any():
            probe["hinge"] = min(probe.get("hinge", np.inf), float(t.detach()[live].abs().min()))
        _trace(probe, "hinge", torch.where(live, t.detach(), torch.full_like(t.detach(), float("nan"))))
    t = (weight * mask * t).clamp(0)
    if probe is not None:
        _trace(probe, "live", t.detach().gt(1e-16).sum())
    return t.sum() / (t.gt(1e-16).to(D.dtype).sum() + 1e-16)


def objective_terms(e_img, e_txt, h_img, h_txt, labels, cst, probe=None):
    """torch tensors of one dtype (labels: 0 / 1 of any dtype) -> the nine TERMS, a tensor with a graph"""
    dtype = e_img.dtype
    M = e_img.shape[1]
    lab = torch.as_tensor(labels).to(dtype)
    x = F.normalize(e_img.reshape(-1, e_img.shape[-1]), dim=-1)
    y = F.normalize(e_txt.reshape(-1, e_txt.shape[-1]), dim=-1)
    s_xy, s_yx = set_similarity(x, y, M, cst, probe), set_similarity(y, x, M, cst, probe)
    if probe is not None:
        probe["one_minus_s"] = min(float((1 - s_xy.detach()).abs().min()), float((1 - s_yx.detach()).abs().min()))
        _trace(probe, "one_minus_s", torch.stack([1 - s_xy.detach(), 1 - s_yx.detach()]))
    T_i2t = triplet_term(torch.clamp(1 - s_xy, 0), lab, cst["token_triplet_margin"], probe)
    T_t2i = triplet_term(torch.clamp(1 - s_yx, 0), lab, cst["token_triplet_margin"], probe)
    g = cst["mmd_gamma"]
    rbf = lambda p, q: torch.exp(-g * torch.cdist(p, q))        # noqa: E731
    mmd = rbf(x, x).mean() - 2 * rbf(x, y).mean() + rbf(y, y).mean()
    if M == 1:
        unif = torch.zeros((), dtype=dtype)
    else:
        uni = lambda p: torch.exp(-20 * torch.cdist(p, p).pow(2)).triu(1).sum() / (M * (M - 1) * 0.5)        # noqa: E731
        unif = uni(x) + uni(y)
    cosd = lambda p, q: torch.clamp(1 - F.cosine_similarity(p.unsqueeze(1), q, dim=-1), 0)                   # noqa: E731
    Th_i2t = triplet_term(cosd(h_img, h_txt), lab, cst["triplet_margin"], probe)
    Th_t2i = triplet_term(cosd(h_txt, h_img), lab, cst["triplet_margin"], probe)
    if cst["hash_func"] == "softmax":
        Q = [1 - torch.pow(2 * h - 1, 2).mean() for h in (h_img, h_txt)]
    else:
        Q = [F.mse_loss(h, torch.sign(h.detach())) for h in (h_img, h_txt)]
    loss = (T_i2t + T_t2i) / 2 * cst["triplet_alpha"] + cst["mmd_alpha"] * mmd + cst["unif_alpha"] * unif \
        + (Th_i2t + Th_t2i) / 2 * cst["hash_triplet_alpha"] + (Q[0] + Q[1]) / 2 * cst["quan_alpha"]
    return torch.stack([loss, T_i2t, T_t2i, mmd, unif, Th_i2t, Th_t2i, Q[0], Q[1]])


def objective(c, dtype, up=None, probe=None, **over):
    """case dict (numpy inputs) -> {terms..., g_*: gradients of up * loss} as float64 numpy, computed in `dtype`.  over: constants to
    replace (a wrong margin, a weight 1 % off)"""
    leaves = {k: torch.tensor(c[k]).to(dtype).requires_grad_(True) for k in INPUTS}
    terms = objective_terms(*[leaves[k] for k in INPUTS], torch.tensor(c["labels"]), dict(consts(c), **over), probe)
    (terms[0] * (c.get("up", 1.0) if up is None else up)).backward()
    out = {k: terms[i].detach().double().numpy().reshape(1) for i, k in enumerate(TERMS)}
    for g, k in zip(GRADS, INPUTS):
        out[g] = leaves[k].grad.double().numpy()
    return out


def kind_of(key):
    if key in ("loss", "mmd", "unif"):
        return key
    return key[0] if key in TERMS else key[:3]


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def _draw(B, M, K, C, seed, clamp=False, density=0.15, unlabelled=False, **rest):
    rng = np.random.default_rng(seed)
    labels = (rng.random((B, C)) < density).astype(np.int64)
    labels[np.arange(B), rng.integers(0, C, B)] = 1              # every row has a label: one without makes the loss NaN
    if unlabelled:
        labels[0] = 0
    e = {m: rng.standard_normal((B, M, K)).astype(np.float32) for m in ("img", "txt")}
    if clamp:
        e["txt"][CLAMP_ROW] = e["img"][CLAMP_ROW]
    if rest.get("hash_func", "tanh") == "softmax":               # softmax_hash: pairs that sum to one
        z = {m: rng.standard_normal((B, K // 2, 2)) * 1.5 for m in ("img", "txt")}
        h = {m: (np.exp(z[m]) / np.exp(z[m]).sum(-1, keepdims=True)).reshape(B, K).astype(np.float32) for m in z}
    else:
        h = {m: np.tanh(rng.standard_normal((B, K)) * 1.5).astype(np.float32) for m in ("img", "txt")}
    return dict(rest, B=B, M=M, K=K, C=C, seed=seed, clamp=clamp, labels=labels, e_img=e["img"], e_txt=e["txt"], h_img=h["img"], h_txt=h["txt"])


def guards(c):
    """-> {"hinge", "one_minus_s", "gap"}: the float64 distances from the kinks (see the module text); absent where there is none"""
    probe = {}
    objective(c, torch.float64, probe=probe)
    return probe


def guarded(probe, clamp=False):
    return probe.get("hinge", np.inf) >= 1e-5 and probe.get("one_minus_s", np.inf) >= 1e-5 and probe.get("gap", np.inf) >= 1e-4


def draw(seed, **spec):
    """_draw, redrawn with seed + 1000, + 2000, ... until the guards hold"""
    for attempt in range(20):
        c = _draw(seed=seed + 1000 * attempt, **spec)
        if guarded(guards(c)):
            return c
    raise AssertionError("no guarded draw for %r" % (spec,))


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
        # the pool's loss and g_e entries come from the one case without a triplet term (C = 1, the loss is the MMD's cancellation); the
        # last column says how far the port is from the case's OWN float32 error, so that nothing hides behind the pool
        print("%-22s %-8s e %.3e  yardstick %.3e  ratio %.2f  bound %.3e  own e_ref %.3e  e / own %.2f"
              % (what, key, e, yard, e / yard if yard else float("inf"), TOL_FACTOR * yard, own.get(key, 0.0),
                 e / own[key] if own.get(key) else float("inf")))
    for key, e, yard in rows:
        assert np.asarray(got[key]).shape == ref64[key].shape, (what, key)
        assert e <= TOL_FACTOR * yard, (what, key, e, yard)
    return max((e / yard if yard else float("inf")) for _, e, yard in rows)


# ---- the token-set head (reference models/DIMCH/hash/hash.py:18-52) ----------------------------------------------------------------
HEAD_PARAMS = ("conv_w", "conv_b", "w1", "b1", "w2", "b2")
HEAD_KEYS = {"conv_w": "%s_token_hash.token_layer.weight", "conv_b": "%s_token_hash.token_layer.bias",
             "w1": "%s_token_hash.hash_layer.0.weight", "b1": "%s_token_hash.hash_layer.0.bias",
             "w2": "%s_token_hash.hash_layer.3.weight", "b2": "%s_token_hash.hash_layer.3.bias"}
HEAD_GUARD = 64 * 2.0 ** -24          # see draw_head_case
# B, T, E, M, K, hash_func, dropout p (0: no keep mask).  Every value of T in {5, 50, 32}, E in {64, 512}, M in {1, 3, 8, 64},
# K in {6, 16, 128} and B in {1, 2, 37} occurs; M = 64 > the convolution's 8 set members a thread, E = 512 two blocks of columns.
HEAD_CASES = {
    "b1_t5_e64_m1_k6": dict(B=1, T=5, E=64, M=1, K=6, hash_func="tanh", p=0.0, seed=6301),
    "b2_t5_e64_m3_k6_keep": dict(B=2, T=5, E=64, M=3, K=6, hash_func="tanh", p=0.3, seed=6302),
    "b37_t5_e64_m3_k16_softmax": dict(B=37, T=5, E=64, M=3, K=16, hash_func="softmax", p=0.3, seed=6303),
    "b2_t50_e512_m8_k16_keep": dict(B=2, T=50, E=512, M=8, K=16, hash_func="tanh", p=0.3, seed=6304),
    "b2_t32_e512_m64_k128": dict(B=2, T=32, E=512, M=64, K=128, hash_func="tanh", p=0.0, seed=6305),
    "b37_t32_e64_m8_k6_keep": dict(B=37, T=32, E=64, M=8, K=6, hash_func="softmax", p=0.5, seed=6306),
}


def head_forward(x, P, keep, p, hash_func):
    """the head on torch tensors of one dtype, with a graph: x [B, T, E], P the six parameters, keep [B M, E / 2] 0 / 1 of that dtype or
    None -> (embeds [B, M, K], code [B, K], the pre-activations of the two relus [B, M, E] and [B, M, E / 2])"""
    c_pre = F.conv1d(x, P["conv_w"], P["conv_b"], padding=1)                              # [B, M, E]
    a_pre = F.linear(F.relu(c_pre), P["w1"], P["b1"])                                     # [B, M, H]
    a = F.relu(a_pre)
    if keep is not None:
        a = a * keep.reshape(a.shape) / (1.0 - p)
    embeds = F.linear(a, P["w2"], P["b2"])                                                # [B, M, K]
    pooled = embeds.mean(1)
    code = torch.tanh(pooled) if hash_func == "tanh" else torch.softmax(pooled.reshape(pooled.shape[0], -1, 2), dim=-1).reshape(pooled.shape)
    return embeds, code, c_pre, a_pre


def head(x, P, keep, p, hash_func, dtype, g_embeds=None, g_hash=None, probe=None):
    """the head of one modality in torch on the CPU: x [B, T, E], P the six parameters (HEAD_PARAMS), keep [B M, E / 2] 0 / 1 or None
    -> {"embeds", "hash"} and, with upstreams, the gradients of sum(embeds g_embeds) + sum(hash g_hash): "g_x" and "g_<parameter>";
    float64 numpy, computed in `dtype`.  probe: receives "relu", the smallest |pre-activation| / max |pre-activation| of both relus"""
    leaves = {k: torch.tensor(np.asarray(v)).to(dtype).requires_grad_(True) for k, v in dict(P, x=x).items()}
    embeds, code, c_pre, a_pre = head_forward(leaves["x"], leaves, None if keep is None else torch.tensor(np.asarray(keep)).to(dtype), p, hash_func)
    if probe is not None:
        probe["relu"] = min(float((z.detach().abs() / z.detach().abs().max()).min()) for z in (c_pre, a_pre))
    out = {"embeds": embeds.detach().double().numpy(), "hash": code.detach().double().numpy()}
    if g_embeds is not None or g_hash is not None:
        tot = sum((t * torch.tensor(np.asarray(g)).to(dtype)).sum() for t, g in ((embeds, g_embeds), (code, g_hash)) if g is not None)
        tot.backward()
        out.update({"g_" + k: v.grad.double().numpy() for k, v in leaves.items()})
    return out


def _draw_head_case(B, T, E, M, K, hash_func, p, seed):
    rng = np.random.default_rng(seed)
    H = E // 2
    f = lambda *shape: rng.standard_normal(shape).astype(np.float32)      # noqa: E731
    P = {"conv_w": f(M, T, 3) * np.float32(np.sqrt(2.0 / (3 * T))), "conv_b": f(M) * np.float32(0.1),
         "w1": f(H, E) * np.float32(np.sqrt(2.0 / E)), "b1": f(H) * np.float32(0.1),
         "w2": f(K, H) * np.float32(np.sqrt(2.0 / H)), "b2": f(K) * np.float32(0.1)}
    keep = (rng.random((B * M, H)) >= p).astype(np.uint8) if p > 0 else None
    return dict(B=B, T=T, E=E, M=M, K=K, hash_func=hash_func, p=p, seed=seed, P=P, keep=keep, x=f(B, T, E), g_embeds=f(B, M, K), g_hash=f(B, K))


@functools.lru_cache(maxsize=None)
def head_case(name):
    """the inputs of HEAD_CASES[name], redrawn (seed + 1000, ...) until in float64 no pre-activation of either relu is nearer to zero
    than HEAD_GUARD = 64 eps (eps = 2^-24) times the largest: the relu's gradient jumps there, and a float32 dot product of a few
    hundred terms of that scale carries an error of some tens of eps, so nearer than that float32 may take the other side"""
    spec = HEAD_CASES[name]
    for attempt in range(40):
        c = _draw_head_case(**dict(spec, seed=spec["seed"] + 1000 * attempt))
        probe = {}
        head(c["x"], c["P"], c["keep"], c["p"], c["hash_func"], torch.float64, probe=probe)
        if probe["relu"] >= HEAD_GUARD:
            return dict(c, name=name, relu=probe["relu"])
    raise AssertionError("no guarded draw for %r" % (spec,))


@functools.lru_cache(maxsize=None)
def head_reference(name, dtype=torch.float64, through="both"):
    """through: "both", "embeds" or "hash" -- which outputs carry an upstream gradient"""
    c = head_case(name)
    return head(c["x"], c["P"], c["keep"], c["p"], c["hash_func"], dtype, c["g_embeds"] if through != "hash" else None,
                c["g_hash"] if through != "embeds" else None)


@functools.lru_cache(maxsize=None)
def head_pool():
    """per tensor, the largest float32-against-float64 error of the restatement over HEAD_CASES (gradients through both outputs)"""
    out = {}
    for name in HEAD_CASES:
        r64, r32 = head_reference(name), head_reference(name, torch.float32)
        for k in r64:
            out[k] = max(out.get(k, 0.0), rel_err(r32[k], r64[k]))
    return out


def head_compare(what, got, ref64, ref32):
    """prints e, the yardstick max(head_pool, e_ref) and their ratio for every tensor of `got`, then asserts e <= TOL_FACTOR * yardstick
    -> worst ratio"""
    rows = []
    for key, g in got.items():
        yard = max(head_pool()[key], rel_err(ref32[key], ref64[key]))
        e = rel_err(g, ref64[key])
        rows.append((key, e, yard))
        print("%-30s %-9s e %.3e  yardstick %.3e  ratio %.2f" % (what, key, e, yard, e / yard))
    for key, e, yard in rows:
        assert np.asarray(got[key]).shape == ref64[key].shape, (what, key)
        assert e <= TOL_FACTOR * yard, (what, key, e, yard)
    return max(e / yard for _, e, yard in rows)
