"""Shared by tools/make_golden_tower_tokens.py, tests/test_tower_tokens_cpu.py and tests/test_gpu_tower_tokens.py (not a test module):
the cases of the two CLIP towers trained through their TOKEN outputs -- shapes, seeded parameters, inputs and the two
upstream gradients --, the float64 restatement -- torch autograd over oracle.encode.clip_image / clip_text with return_patches=True and
a float64 state_dict as leaves -- and the error measure of tests/golden/tower_tokens.npz.

Parameters, images and ids are drawn by tests/tower_grad_cases.py (draw_image_tower / draw_text_tower / draw_images / draw_ids), whose
conventions hold here too: one CPU thread, the projection handed to the oracle repeated over the batch (the reference's torch.bmm),
e = max|x - fp64| / max|fp64| on whole tensors, pooled per tensor kind over the layers.  Tensors of more than FULL elements are stored
as every THIN-th flat element; THIN is 32 here (16 there), which keeps this golden file, with its larger cases, below that one.

The loss is (cls . up_cls).sum() + (tokens . up_tok).sum() with cls [B, E] and tokens in the towers' LND layout ([L - 1, B, E] image,
[L, B, E] text); `use` = "cls" or "tokens" keeps one term only.  Tensor kinds: y_cls, y_tok and the g_<parameter> kinds of
tower_grad_cases."""
import os

import numpy as np
import torch

import block_grad_cases as BC
import tower_grad_cases as TG
from oracle import encode as enc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tower_tokens.npz")
SEED = 3141
FULL, THIN = 256, 32
rel_err, checksum = BC.rel_err, BC.checksum
tower_of, kind_of, tensor_key, count_layers = TG.tower_of, TG.kind_of, TG.tensor_key, TG.count_layers
build_clip, tower_parameters = TG.build_clip, TG.tower_parameters
KINDS = {t: ("y_cls", "y_tok") + TG.KINDS[t][1:] for t in TG.KINDS}

# image: name -> (resolution, patch, width, layers, out_dim, B)
IMG_CASES = {
    "img_r8_p4_d64_b1": (8, 4, 64, 1, 16, 1),           # L = 5, one item: M = 5 rows, no multiple of the 4 rows a LayerNorm-backward block takes
    "img_r32_p8_d128_b3": (32, 8, 128, 2, 32, 3),       # M = 51
    "img_r64_p32_d64_b2": (64, 32, 64, 1, 48, 2),       # out_dim no multiple of 32, conv K = 3072
    "img_r28_p4_d64_b5": (28, 4, 64, 1, 16, 5),         # M = 250: several column chunks and TN splits, with remainders
}
# text: name -> (vocab, context, width, layers, out_dim, L, B, key padding)
TXT_CASES = {
    "txt_v50_c8_d64_l1_b1": (50, 8, 64, 1, 16, 1, 1, False),          # M = 1
    "txt_v11_c40_d64_b5_kpm": (11, 40, 64, 2, 32, 33, 5, True),       # ids repeat; EOS at rows 0, L - 1 and drawn ones: g_eos lands on a row of g_tokens
    "txt_v64_c16_d64_b3": (64, 16, 64, 1, 16, 7, 3, False),           # L < context
    "txt_v97_c64_d64_l50_b41": (97, 64, 64, 1, 16, 50, 41, False),    # M = 2050: 16 TN splits plus a remainder
    "txt_v97_c64_d64_l64_b65": (97, 64, 64, 1, 16, 64, 65, False),    # M = 4160 > 64 * 64: the chunk cap of the LayerNorm column sums
}
CASES = dict(IMG_CASES, **TXT_CASES)
# restatement only, not in the golden file
OTHER = [("img", (224, 32, 768, 1, 512, 2)), ("txt", (300, 77, 512, 2, 512, 32, 2, False))]


def thin(a):
    a = np.asarray(a).reshape(-1)
    return a if a.size <= FULL else a[::THIN]


def case_seed(name):
    return SEED + 10 * sorted(CASES).index(name)


def draw_upstream(seed, B, rows, out_dim):
    """up_cls [B, E] and up_tok [rows, B, E] (the LND layout of the tokens)"""
    rng = np.random.default_rng([seed, 31])
    return rng.standard_normal((B, out_dim)).astype(np.float32), rng.standard_normal((rows, B, out_dim)).astype(np.float32)


def image_inputs(spec, seed):
    res, patch, D, layers, out_dim, B = spec
    image, _ = TG.draw_images(seed, B, res, out_dim)
    return TG.draw_image_tower(seed, res, patch, D, layers, out_dim), image, draw_upstream(seed, B, (res // patch) ** 2, out_dim), None


def text_inputs(spec, seed):
    vocab, context, D, layers, out_dim, L, B, kp = spec
    ids, _ = TG.draw_ids(seed, B, L, vocab, out_dim)
    return TG.draw_text_tower(seed, vocab, context, D, layers, out_dim), ids, draw_upstream(seed, B, L, out_dim), (BC.draw_kpm(seed, B, L) if kp else None)


def spec_inputs(tower, spec, seed):
    return (image_inputs if tower == "img" else text_inputs)(spec, seed)


def case_inputs(name):
    """-> (state_dict of the tower, images or ids, (up_cls, up_tok), key padding mask or None)"""
    return spec_inputs(tower_of(name), CASES[name], case_seed(name))


def inputs_checksum(sd, x, ups, kpm):
    return checksum([sd[k] for k in sorted(sd)] + [x, ups[0], ups[1]] + ([] if kpm is None else [kpm.astype(np.uint8)]))


def tensor_names(tower, layers):
    return ["y_cls", "y_tok"] + TG.tensor_names(tower, layers)[1:]


def loss_of(cls, tokens, ups, use="both"):
    """(cls . up_cls).sum() + (tokens . up_tok).sum(), or one of the two terms"""
    terms = []
    if use in ("both", "cls"):
        terms.append((cls * ups[0]).sum())
    if use in ("both", "tokens"):
        terms.append((tokens * ups[1]).sum())
    return sum(terms)


def run_restatement(tower, sd, x, ups, kpm, dtype, use="both"):
    """loss_of(...).backward() over oracle.encode.clip_image / clip_text (return_patches=True) in `dtype` -> {tensor name: numpy array}"""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        t = {k: torch.tensor(v).to(dtype).requires_grad_(True) for k, v in sd.items()}
        proj = "visual.proj" if tower == "img" else "text_projection"
        fed = dict(t, **{proj: t[proj].unsqueeze(0).repeat(x.shape[0], 1, 1)})       # the reference's bmm, as in tower_grad_cases
        if tower == "img":
            cls, tokens = enc.clip_image(fed, torch.tensor(x).to(dtype), return_patches=True)
        else:
            cls, tokens, _ = enc.clip_text(fed, torch.tensor(x), None if kpm is None else torch.tensor(kpm), return_patches=True)
        loss_of(cls, tokens, [torch.tensor(u).to(dtype) for u in ups], use).backward()
        out = {"y_cls": cls.detach().numpy().copy(), "y_tok": tokens.detach().numpy().copy()}
        for name in tensor_names(tower, count_layers(tower, sd))[2:]:
            g = t[tensor_key(tower, name)].grad
            out[name] = (torch.zeros_like(t[tensor_key(tower, name)]) if g is None else g).numpy().copy().reshape(sd[tensor_key(tower, name)].shape)
        return out
    finally:
        torch.set_num_threads(threads)


erefs = TG.erefs

_golden = None


def golden():
    global _golden
    if _golden is None:
        _golden = dict(np.load(GOLDEN))
    return _golden


def pool_eref(tower, kind):
    """max of the stored e_ref over every committed case of this tower and every layer, for this tensor kind"""
    vals = [float(v) for k, v in golden().items() if k.startswith(tower) and "__eref_" in k and kind_of(k.split("__eref_")[1]) == kind]
    assert vals, (tower, kind)
    return max(vals)
