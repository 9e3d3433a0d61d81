"""Shared by tools/make_golden_mith_head_grad.py, tests/test_mith_head_grad_cpu.py and tests/test_gpu_mith_head_grad.py (not a test
module): the cases of MITH's training head (shapes, seeded parameters, inputs, masks and upstream gradients), a torch restatement
of one modality of the reference's HashLayer.encode_img / encode_txt (models/MITH/hash/hash.py:231-247) that runs in float32 and in
float64 with the parameters and the two inputs as autograd leaves, and the error measure of the golden file.

The reference's own HashLayer cannot serve as the float64 side (its transformer's LayerNorm casts to fp32); its fp32 run in
.train() mode is what tests/golden/mith_head_grad.npz stores, and the fp32 run of the restatement equals it to the bit at the
committed cases (asserted by the generator).  Runs here use one CPU thread, so the fp32 bits do not depend on the machine.

Selection.  The LTA keep-set (score > 0, and >= the token's top_k-th score) is discontinuous.  `run_restatement(..., keep=...)`
evaluates the head with a GIVEN keep-set [L, B, K] instead of its own, which is how the GPU tests compare (the keep-set the forward
stored); `selection` returns the restatement's own set and every entry's margin to its nearest threshold.

Tensor kinds: the four outputs, g_cls, g_tokens, g_concept, g_hash_w, g_hash_b, g_proj_w, g_proj_b, g_mlp_<field> (pooled over the
residual MLPs) and g_blk_<field> (pooled over the blocks).  Stored tensors of more than FULL elements keep every THIN-th flat
element (`thin`); the error measure e = max|x - fp64| / max|fp64| is always taken on whole tensors."""
import math
import os
import zlib

import numpy as np
import torch
import torch.nn.functional as F

import block_grad_cases as BC
from oracle import encode as enc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mith_head_grad.npz")
FULL, THIN = 256, 16
SEED = 2718

MLP_FIELDS = ("ln_w", "ln_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b")
OUTPUTS = ("res_cls", "cls_hash", "tokens_hash", "trans_tokens")

# name -> (D, heads, lct layers, res_mlp_layers, K, top_k, L, B, modality, mask): mask "pad" = a padding mask (text), "pad_all" = the
# same with every token of sample 1 masked
CASES = {
    "k8_top8_l7_r2_img": (64, 1, 1, 2, 8, 8, 7, 2, "img", None),                 # top_k = K, two residual MLPs
    "k20_top8_l50_r1_txt_allmasked": (64, 1, 2, 1, 20, 8, 50, 3, "txt", "pad_all"),   # K no multiple of 16, L = 50, a sample without tokens
    "k72_top1_l7_r0_img": (64, 1, 1, 0, 72, 1, 7, 2, "img", None),               # the second 64-stride group, top_k = 1, no MLP: empty concepts
    "k128_top8_l1_r2_img": (64, 1, 1, 2, 128, 8, 1, 2, "img", None),             # the K limit, one token
    "d128_k16_top8_l7_r2_txt": (128, 2, 2, 2, 16, 8, 7, 3, "txt", "pad"),        # two heads, two blocks
}
# cases in which some (sample, concept) has no positive score (the NaN -> 0 route); asserted by the generator and the GPU test
EMPTY_CONCEPT_CASES = ("k72_top1_l7_r0_img", "k128_top8_l1_r2_img", "k20_top8_l50_r1_txt_allmasked")


def case_seed(name):
    return SEED + 10 * sorted(CASES).index(name)


def positional_encoding(D, K):
    """PositionalEncoding.pe (models/MITH/hash/hash.py:52-60) -> [K, 1, D] fp32, as the module's buffer holds it"""
    pe = torch.zeros(K, D)
    position = torch.arange(0, K, dtype=torch.float).unsqueeze(1)
    div_term = torch.exp(torch.arange(0, D, 2).float() * (-math.log(10000.0) / D))
    pe[:, 0::2] = torch.sin(position * div_term)
    pe[:, 1::2] = torch.cos(position * div_term)
    return (pe.unsqueeze(0).transpose(0, 1) / (D ** 0.5)).numpy()


def draw_params(seed, D, layers, R, K):
    """the parameters of one modality under modality-free names: mlp<i>.<field>, concept, blk.resblocks.<i>.<key>, hash_w [K, D],
    hash_b [K], proj_w, proj_b.  LayerNorm weights around 1, matrices sigma 0.05 (the concept embedding 0.1), vectors sigma 0.1."""
    sd = {}
    for i in range(R):
        for t, f in enumerate(MLP_FIELDS):
            rng = np.random.default_rng([seed, 3, i, t])
            shape = {"ln_w": (D,), "ln_b": (D,), "fc1_w": (4 * D, D), "fc1_b": (4 * D,), "fc2_w": (D, 4 * D), "fc2_b": (D,)}[f]
            v = 0.05 * rng.standard_normal(shape) if len(shape) == 2 else 0.1 * rng.standard_normal(shape) + (1.0 if f == "ln_w" else 0.0)
            sd["mlp%d.%s" % (i, f)] = v.astype(np.float32)
    rng = np.random.default_rng([seed, 5])
    sd["concept"] = (0.1 * rng.standard_normal((K, D))).astype(np.float32)
    sd["hash_w"] = (0.1 * rng.standard_normal((K, D))).astype(np.float32)
    sd["hash_b"] = (0.1 * rng.standard_normal((K,))).astype(np.float32)
    sd["proj_w"] = (0.05 * rng.standard_normal((D, D))).astype(np.float32)
    sd["proj_b"] = (0.1 * rng.standard_normal((D,))).astype(np.float32)
    for k, v in BC.draw_params(seed, D, layers).items():
        sd["blk." + k] = v
    return sd


def draw_batch(seed, B, L, D, K):
    """cls [B, D], tokens [L, B, D] (LND) and the four upstream gradients in the outputs' shapes"""
    rng = np.random.default_rng([seed, 11])
    f = lambda *s: rng.standard_normal(s).astype(np.float32)      # noqa: E731
    return f(B, D), f(L, B, D), (f(B, D), f(B, K), f(B, K), f(K, B, D))


def draw_mask(seed, B, L, kind):
    """[B, L] bool, True = the token is ignored: caption lengths from 1 to L; "pad_all": every token of sample 1"""
    if kind is None:
        return None
    rng = np.random.default_rng([seed, 13])
    m = np.zeros((B, L), dtype=bool)
    for b in range(B):
        m[b, int(rng.integers(1, L + 1)):] = True
    m[0, max(L // 2, 1):] = True
    if kind == "pad_all":
        m[1, :] = True
    return m


def case_inputs(name):
    D, heads, layers, R, K, top_k, L, B, mod, mk = CASES[name]
    seed = case_seed(name)
    cls, tok, ups = draw_batch(seed, B, L, D, K)
    return draw_params(seed, D, layers, R, K), cls, tok, draw_mask(seed, B, L, mk), ups


def checksum(arrays):
    c = 0
    for a in arrays:
        c = zlib.crc32(np.ascontiguousarray(a).tobytes(), c)
    return float(c)


def inputs_checksum(sd, cls, tok, mask, ups):
    return checksum([sd[k] for k in sorted(sd)] + [cls, tok, *ups] + ([] if mask is None else [mask.astype(np.uint8)]))


def ref_state(sd, ref_sd, mod):
    """the reference HashLayer's state_dict (key -> tensor) with this modality's parameters in both modalities' places"""
    out = {}
    for key, v in ref_sd.items():
        k = key.replace("gcl_t.", "gcl_i.").replace("lct_t.", "lct_i.").replace("txt_concept_proj.", "img_concept_proj.")
        if k.endswith("position.pe"):
            out[key] = v
        elif k.startswith("gcl_i.mlp.lns."):
            i, f = k.split(".")[3:5]
            out[key] = torch.tensor(sd["mlp%s.ln_%s" % (i, f[0])])
        elif k.startswith("gcl_i.mlp.mlps."):
            i, j, f = k.split(".")[3:6]
            out[key] = torch.tensor(sd["mlp%s.fc%d_%s" % (i, 1 if j == "0" else 2, f[0])])
        elif k == "gcl_i.common_concept_embedding.weight":
            out[key] = torch.tensor(sd["concept"])
        elif k.startswith("lct_i.transformer."):
            out[key] = torch.tensor(sd["blk." + k[len("lct_i.transformer."):]])
        elif k.startswith("lct_i.hashing.fc_list."):
            i, f = k.split(".")[3:5]
            out[key] = torch.tensor(sd["hash_w"][int(i):int(i) + 1] if f == "weight" else sd["hash_b"][int(i):int(i) + 1])
        elif k.startswith("img_concept_proj."):
            out[key] = torch.tensor(sd["proj_w" if k.endswith("weight") else "proj_b"])
        else:
            raise KeyError(key)
    assert all(tuple(out[k].shape) == tuple(v.shape) for k, v in ref_sd.items())
    return out


def _gcl(t, x, R):
    for i in range(R):
        p = "mlp%d." % i
        h = F.layer_norm(x, (x.shape[-1],), t[p + "ln_w"], t[p + "ln_b"], 1e-5)
        x = x + F.linear(F.gelu(F.linear(h, t[p + "fc1_w"], t[p + "fc1_b"])), t[p + "fc2_w"], t[p + "fc2_b"])
    return x, torch.tanh(F.linear(x, t["concept"]))


def _masked(scores, mask):
    """scores [L, B, K] with -inf on the masked tokens (models/MITH/hash/hash.py:142-148)"""
    if mask is None:
        return scores
    return scores + torch.where(torch.as_tensor(mask), float("-inf"), 0.0).to(scores.dtype).t()[:, :, None]


def selection(scores, mask, top_k):
    """scores [L, B, K] (any float dtype) -> (keep [L, B, K] bool as :151-156 selects, margin [L, B, K]: how far every unmasked entry's
    score is from the value at which it would change sides -- 0 for every entry; for a kept one also the token's (top_k + 1)-th
    positive score, which would displace it, and for a dropped positive one the top_k-th, which it would have to reach; inf on
    masked tokens)"""
    neg, inf = torch.full_like(scores, float("-inf")), torch.full_like(scores, float("inf"))
    sim = _masked(scores, mask)
    sim = torch.where(sim > 0, sim, neg)
    K = scores.shape[-1]
    top = torch.topk(sim, k=min(top_k + 1, K), dim=-1).values
    kth = top[..., top_k - 1:top_k]
    nxt = top[..., top_k:top_k + 1] if top_k < K else neg[..., :1]
    keep = (sim >= kth) & (sim > float("-inf"))
    rank = torch.where(keep, torch.where(torch.isfinite(nxt), scores - nxt, inf), torch.where(torch.isfinite(kth), kth - scores, inf))
    margin = torch.minimum(scores.abs(), torch.where(scores > 0, rank.abs(), inf))
    if mask is not None:
        margin = torch.where(torch.as_tensor(mask).t()[:, :, None], torch.full_like(margin, float("inf")), margin)
    return keep, margin


def head_outputs(t, ct, tt, mask, heads, top_k, keep=None):
    """one modality of the head over torch tensors of one dtype: t the parameters under draw_params' names, ct [B, D], tt [L, B, D]
    -> ((res_cls, cls_hash, tokens_hash, trans_tokens) with their graph, the selected scores [L, B, K] (-inf where dropped), the
    detached scores).  keep [L, B, K] bool: use this set instead of the head's own selection."""
    dtype = ct.dtype
    R = len({k.split(".")[0] for k in t if k.startswith("mlp")})
    layers = len({k.split(".")[2] for k in t if k.startswith("blk.")})
    K, D = t["concept"].shape
    y, cls_hash = _gcl(t, ct, R)
    res_cls = F.normalize(y, dim=-1)
    scores = _gcl(t, tt, R)[1].detach()                                           # [L, B, K], no gradient (:235)
    neg = torch.full_like(scores, float("-inf"))
    if keep is None:
        sim = _masked(scores.clone(), mask)
        sim = torch.where(sim > 0, sim, neg)
        kth = torch.topk(sim, k=top_k, dim=-1).values.min(dim=-1, keepdim=True).values
        sim = torch.where(sim >= kth, sim, neg)
    else:
        sim = torch.where(torch.as_tensor(keep), scores, neg)
    att = torch.softmax(sim, dim=0)
    att = torch.where(torch.isnan(att), torch.zeros_like(att), att)
    merged = torch.bmm(att.permute(1, 2, 0), tt.permute(1, 0, 2)).permute(1, 0, 2)       # [K, B, D]
    x = merged + torch.tensor(positional_encoding(D, K)).to(dtype)
    blk = {k[len("blk."):]: v for k, v in t.items() if k.startswith("blk.")}
    z = enc._blocks(x, blk, "", layers, heads, None)
    bits = torch.stack([F.linear(z[k], t["hash_w"][k:k + 1], t["hash_b"][k:k + 1]) for k in range(K)])      # [K, B, 1]
    tokens_hash = torch.tanh(bits.permute(1, 0, 2).squeeze(-1))
    trans = F.normalize(F.linear(z, t["proj_w"], t["proj_b"]), dim=-1)
    return (res_cls, cls_hash, tokens_hash, trans), sim, scores


def grad_name(key):
    """parameter name of draw_params -> its gradient's tensor name"""
    if key.startswith("mlp"):
        return "g_" + key.replace(".", "_")
    if key.startswith("blk."):
        _, _, i, k = key.split(".", 3)
        return "g_l%s_%s" % (i, next(kind for kind, kk in BC.PARAMS if kk == k))
    return "g_" + key


def e2e_key(name):
    """parameter name under model.hash -> (group: gcl / i / t, the restatement's key, row of a stacked hash tensor or None)"""
    p = name.split(".")
    if p[0].startswith("gcl"):
        if p[1] == "common_concept_embedding":
            return "gcl", "concept", None
        if p[2] == "lns":
            return "gcl", "mlp%s.ln_%s" % (p[3], p[4][0]), None
        return "gcl", "mlp%s.fc%d_%s" % (p[3], 1 if p[4] == "0" else 2, p[5][0]), None
    if p[0].startswith("lct"):
        g = p[0][-1]
        if p[1] == "transformer":
            return g, "blk." + ".".join(p[2:]), None
        return g, "hash_w" if p[-1] == "weight" else "hash_b", int(p[3])
    return p[0][0], "proj_w" if p[-1] == "weight" else "proj_b", None


def run_restatement(sd, cls, tok, mask, ups, heads, top_k, dtype, keep=None, scores_out=None):
    """sum_i (output_i . up_i).sum().backward() over one modality of the head in `dtype` -> {tensor name: numpy array}: the four
    outputs, g_cls [B, D], g_tokens [L, B, D], g_<parameter> (g_mlp<i>_<field>, g_l<i>_<block field>), and "keep" [L, B, K] bool, the
    keep-set used.  ups[i] None: that output does not enter the objective.  keep: use this set instead of the head's own."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        t = {k: torch.tensor(v).to(dtype).requires_grad_(True) for k, v in sd.items()}
        ct, tt = torch.tensor(cls).to(dtype).requires_grad_(True), torch.tensor(tok).to(dtype).requires_grad_(True)
        outs, sim, scores = head_outputs(t, ct, tt, mask, heads, top_k, keep)
        if scores_out is not None:
            scores_out.append(scores.clone())
        obj = sum((o * torch.tensor(u).to(dtype)).sum() for o, u in zip(outs, ups) if u is not None)
        obj.backward()
        zero = lambda p: torch.zeros_like(p) if p.grad is None else p.grad      # noqa: E731
        out = {n: o.detach().numpy().copy() for n, o in zip(OUTPUTS, outs)}
        out["g_cls"], out["g_tokens"] = zero(ct).numpy().copy(), zero(tt).numpy().copy()
        for k, p in t.items():
            out[grad_name(k)] = zero(p).numpy().copy()
        out["keep"] = (sim > float("-inf")).numpy().copy()
        return out
    finally:
        torch.set_num_threads(threads)


def kind_of(tensor):
    """g_mlp<i>_<field> -> g_mlp_<field>, g_l<i>_<field> -> g_blk_<field>, everything else is its own kind"""
    if tensor.startswith("g_mlp"):
        return "g_mlp_" + tensor.split("_", 2)[2]
    if tensor.startswith("g_l") and tensor[3].isdigit():
        return "g_blk_" + tensor.split("_", 2)[2]
    return tensor


rel_err = BC.rel_err


def thin(a):
    a = np.asarray(a).reshape(-1)
    return a if a.size <= FULL else a[::THIN]


def erefs(r32, r64):
    """per tensor and pooled (max) per kind"""
    per = {k: rel_err(r32[k], r64[k]) for k in r64 if k != "keep"}
    pool = {}
    for k, e in per.items():
        pool[kind_of(k)] = max(pool.get(kind_of(k), 0.0), e)
    return per, pool


_golden = None


def golden():
    global _golden
    if _golden is None:
        _golden = dict(np.load(GOLDEN))
    return _golden


def pool_eref(kind):
    """max of the stored e_ref over every committed case and layer of this tensor kind"""
    vals = [float(v) for k, v in golden().items() if "__eref_" in k and kind_of(k.split("__eref_")[1]) == kind]
    assert vals, kind
    return max(vals)


# ---- xmh_lta_aggregate on the inputs of tests/golden/encode_mith.npz (its text tokens and mask), K = 16 ----------------------------------
def lta_inputs():
    """-> scores [B, L, K], tokens [B, L, D], mask [B, L] bool, pe [K, D], top_k: the text tokens and the mask of the MITH encode golden,
    scores = tanh of a seeded normal tensor"""
    from xmh.models import weights as W
    from test_oracle_encode import mith_inputs
    g = np.load(os.path.join(os.path.dirname(GOLDEN), "encode_mith.npz"))
    _, _, _, tok_t, mask = mith_inputs(W, int(g["seed"]))
    assert np.array_equal(mask.numpy(), g["mask"])
    B, L, K, D = tok_t.shape[1], tok_t.shape[0], 16, tok_t.shape[2]
    scores = torch.tanh(W.synth_tensor(int(g["seed"]), "mith_head_grad.lta_scores", (B, L, K), 1.0))
    return scores, tok_t.permute(1, 0, 2).contiguous(), mask, torch.tensor(positional_encoding(D, K)).reshape(K, D), 8
