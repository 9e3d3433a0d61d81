"""Shared by tools/make_golden_tower_grad.py, tests/test_tower_grad_cpu.py and tests/test_gpu_tower_grad.py (not a test module): the
cases of the two CLIP towers' backward (shapes, seeded parameters, inputs and upstream gradients), the float64 restatement -- torch
autograd over oracle.encode.clip_image / clip_text with a float64 state_dict as leaves -- and the error measure of the golden file.

The reference's own towers cannot serve as the float64 side (their LayerNorm casts to fp32); their fp32 run is what
tests/golden/tower_grad.npz stores, and the fp32 run of the restatement here equals it to the bit at the committed shapes (asserted
by the generator).  Runs here use one CPU thread, so that the fp32 bits do not depend on how many a machine has.

Tensor kinds, per tower: y (the feature), g_<own parameter> (image: proj, ln_post_w/b, ln_pre_w/b, pos, cls, conv1; text:
text_projection, ln_final_w/b, pos, tok) and g_<parameter> for the twelve parameters of a block (pooled over the layers).  Stored
tensors of more than FULL elements keep every THIN-th flat element; e = max|x - fp64| / max|fp64| is always taken on whole tensors.

Text ids: EOS (vocab - 1) once per caption, padding id 0 behind it, drawn ids from [1, vocab - 2] before it; the EOS positions of a
case are L - 1 and 0 (a single caption has its EOS at L - 1) and drawn ones, in ascending order over the batch: the reference
normalises the rows in [L, B] order and the restatement in [B, L] order, and only so do the B rows that carry a gradient come in
the same order in both, which the bit equality of ln_final's gradients needs."""
import os

import numpy as np
import torch

import block_grad_cases as BC
from oracle import encode as enc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tower_grad.npz")
SEED = 2718
rel_err, thin, checksum = BC.rel_err, BC.thin, BC.checksum

IMG_OWN = (("proj", "visual.proj"), ("ln_post_w", "visual.ln_post.weight"), ("ln_post_b", "visual.ln_post.bias"),
           ("ln_pre_w", "visual.ln_pre.weight"), ("ln_pre_b", "visual.ln_pre.bias"), ("pos", "visual.positional_embedding"),
           ("cls", "visual.class_embedding"), ("conv1", "visual.conv1.weight"))
TXT_OWN = (("text_projection", "text_projection"), ("ln_final_w", "ln_final.weight"), ("ln_final_b", "ln_final.bias"),
           ("pos", "positional_embedding"), ("tok", "token_embedding.weight"))
OWN = {"img": IMG_OWN, "txt": TXT_OWN}
PREFIX = {"img": "visual.transformer.", "txt": "transformer."}
BLOCK_KINDS = tuple("g_" + k for k, _ in BC.PARAMS)
KINDS = {t: ("y",) + tuple("g_" + k for k, _ in OWN[t]) + BLOCK_KINDS for t in OWN}

# image: name -> (resolution, patch, width, layers, out_dim, B)
IMG_CASES = {
    "img_r8_p4_d64_b1": (8, 4, 64, 1, 16, 1),           # L = 5, a single item
    "img_r32_p8_d128_b3": (32, 8, 128, 2, 32, 3),       # L = 17, conv K = 192
    "img_r64_p32_d64_b2": (64, 32, 64, 1, 48, 2),       # conv K = 3072, out_dim no multiple of 32
    "img_r28_p4_d64_b5": (28, 4, 64, 1, 16, 5),         # L = 50
}
# text: name -> (vocab, context, width, layers, out_dim, L, B, key padding)
TXT_CASES = {
    "txt_v50_c8_d64_b1": (50, 8, 64, 1, 16, 8, 1, False),
    "txt_v11_c40_d64_b5_kpm": (11, 40, 64, 2, 32, 33, 5, True),      # every id repeats across and within rows
    "txt_v97_c77_d128_b2": (97, 77, 128, 1, 32, 77, 2, False),       # CLIP's context
    "txt_v64_c16_d64_b3": (64, 16, 64, 1, 16, 7, 3, False),          # L < context: g_pos rows from 7 on are zero
}
CASES = dict(IMG_CASES, **TXT_CASES)


def tower_of(name):
    return name[:3]


def case_seed(name):
    return SEED + 10 * sorted(CASES).index(name)


def _own(rng, key, shape):
    if key.endswith("ln_pre.weight") or key.endswith("ln_post.weight") or key == "ln_final.weight":
        return 1.0 + 0.1 * rng.standard_normal(shape)
    if key in ("visual.proj", "text_projection"):
        return shape[0] ** -0.5 * rng.standard_normal(shape)
    if key == "visual.conv1.weight":
        return 0.05 * rng.standard_normal(shape)
    return 0.1 * rng.standard_normal(shape)


def draw_image_tower(seed, res, patch, D, layers, out_dim):
    """state_dict of the image tower under the reference's key names"""
    L = (res // patch) ** 2 + 1
    shapes = {"visual.proj": (D, out_dim), "visual.positional_embedding": (L, D), "visual.class_embedding": (D,),
              "visual.conv1.weight": (D, 3, patch, patch)}
    sd = {}
    for t, (_, key) in enumerate(IMG_OWN):
        sd[key] = _own(np.random.default_rng([seed, 17, t]), key, shapes.get(key, (D,))).astype(np.float32)
    sd.update({PREFIX["img"] + k: v for k, v in BC.draw_params(seed, D, layers).items()})
    return sd


def draw_text_tower(seed, vocab, context, D, layers, out_dim):
    shapes = {"text_projection": (D, out_dim), "positional_embedding": (context, D), "token_embedding.weight": (vocab, D)}
    sd = {}
    for t, (_, key) in enumerate(TXT_OWN):
        sd[key] = _own(np.random.default_rng([seed, 19, t]), key, shapes.get(key, (D,))).astype(np.float32)
    sd.update({PREFIX["txt"] + k: v for k, v in BC.draw_params(seed, D, layers).items()})
    return sd


def draw_images(seed, B, res, out_dim):
    """image batch and the upstream gradient"""
    rng = np.random.default_rng([seed, 23])
    return rng.standard_normal((B, 3, res, res)).astype(np.float32), rng.standard_normal((B, out_dim)).astype(np.float32)


def draw_ids(seed, B, L, vocab, out_dim):
    """ids [B, L] int64 and the upstream gradient"""
    rng = np.random.default_rng([seed, 29])
    eos = sorted(([L - 1, 0] + [int(v) for v in rng.integers(0, L, size=max(B - 2, 0))])[:B])
    ids = np.zeros((B, L), dtype=np.int64)
    for b, e in enumerate(eos):
        ids[b, :e] = rng.integers(1, vocab - 1, size=e)
        ids[b, e] = vocab - 1
    return ids, rng.standard_normal((B, out_dim)).astype(np.float32)


def image_inputs(spec, seed):
    res, patch, D, layers, out_dim, B = spec
    image, up = draw_images(seed, B, res, out_dim)
    return draw_image_tower(seed, res, patch, D, layers, out_dim), image, up, None


def text_inputs(spec, seed):
    vocab, context, D, layers, out_dim, L, B, kp = spec
    ids, up = draw_ids(seed, B, L, vocab, out_dim)
    return draw_text_tower(seed, vocab, context, D, layers, out_dim), ids, up, (BC.draw_kpm(seed, B, L) if kp else None)


def case_inputs(name):
    """-> (state_dict of the tower, images or ids, upstream gradient, key padding mask or None)"""
    return (image_inputs if tower_of(name) == "img" else text_inputs)(CASES[name], case_seed(name))


def inputs_checksum(sd, x, up, kpm):
    return checksum([sd[k] for k in sorted(sd)] + [x, up] + ([] if kpm is None else [kpm.astype(np.uint8)]))


def tensor_names(tower, layers):
    return ["y"] + ["g_" + k for k, _ in OWN[tower]] + ["g_l%d_%s" % (i, k) for i in range(layers) for k, _ in BC.PARAMS]


def tensor_key(tower, name):
    """y is no parameter; g_<own> and g_l<i>_<param> -> the state_dict key"""
    own = dict(OWN[tower])
    if name[2:] in own:
        return own[name[2:]]
    _, layer, kind = name.split("_", 2)
    return "%sresblocks.%d.%s" % (PREFIX[tower], int(layer[1:]), dict(BC.PARAMS)[kind])


def kind_of(name):
    """y, g_<own>, g_l<i>_<param> -> its kind"""
    parts = name.split("_", 2)
    if len(parts) == 3 and parts[1][:1] == "l" and parts[1][1:].isdigit():
        return "g_" + parts[2]
    return name


def count_layers(tower, sd):
    return enc._count_layers(sd, PREFIX[tower])


def run_restatement(tower, sd, x, up, kpm, dtype):
    """(y . up).sum().backward() over oracle.encode.clip_image / clip_text in `dtype` -> {tensor name: numpy array}"""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        t = {k: torch.tensor(v).to(dtype).requires_grad_(True) for k, v in sd.items()}
        # the reference multiplies by the projection item by item (torch.bmm with the matrix repeated over the batch), and its
        # gradient is the sum of the items' products: hand the oracle the repeated matrix, so that its `x @ proj` is that bmm
        proj = "visual.proj" if tower == "img" else "text_projection"
        fed = dict(t, **{proj: t[proj].unsqueeze(0).repeat(x.shape[0], 1, 1)})
        if tower == "img":
            y = enc.clip_image(fed, torch.tensor(x).to(dtype))
        else:
            y = enc.clip_text(fed, torch.tensor(x), None if kpm is None else torch.tensor(kpm))
        (y * torch.tensor(up).to(dtype)).sum().backward()
        out = {"y": y.detach().numpy().copy()}
        for name in tensor_names(tower, count_layers(tower, sd))[1:]:
            g = t[tensor_key(tower, name)].grad
            out[name] = g.numpy().copy().reshape(sd[tensor_key(tower, name)].shape)
        return out
    finally:
        torch.set_num_threads(threads)


def erefs(r32, r64):
    """per tensor and pooled (max) per kind"""
    per = {k: rel_err(r32[k], r64[k]) for k in r64}
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


def pool_eref(tower, kind):
    """max of the stored e_ref over every committed case of this tower and every layer, for this tensor kind"""
    vals = [float(v) for k, v in golden().items() if k.startswith(tower) and "__eref_" in k and kind_of(k.split("__eref_")[1]) == kind]
    assert vals, (tower, kind)
    return max(vals)


# ---- the package's module for a case (GPU tests) -------------------------------------------------------------------------------
def build_clip(tower, sd):
    """xmh.models.clip.CLIP holding the case's tower; the other tower is the smallest the class takes (no layers), zeros"""
    from xmh.models.clip import CLIP
    if tower == "img":
        D, out_dim = sd["visual.proj"].shape
        patch = sd["visual.conv1.weight"].shape[-1]
        res = patch * round((sd["visual.positional_embedding"].shape[0] - 1) ** 0.5)
        m = CLIP(out_dim, res, count_layers(tower, sd), D, patch, 2, 4, 64, 1, 0)
    else:
        D, out_dim = sd["text_projection"].shape
        vocab, context = sd["token_embedding.weight"].shape[0], sd["positional_embedding"].shape[0]
        m = CLIP(out_dim, 4, 0, 64, 4, context, vocab, D, D // 64, count_layers(tower, sd))
    missing, unexpected = m.load_state_dict({k: torch.tensor(v) for k, v in sd.items()}, strict=False)
    assert not unexpected and all(k.startswith("visual.") != (tower == "img") or k == "logit_scale" for k in missing), (missing, unexpected)
    return m


def tower_parameters(tower, m):
    """{tensor name: parameter} of the case's tower in a CLIP module"""
    named = dict(m.named_parameters())
    layers = len((m.visual.transformer if tower == "img" else m.transformer).resblocks)
    return {name: named[tensor_key(tower, name)] for name in tensor_names(tower, layers)[1:]}
