"""Cases and restatements for the training image transform (xmh_image_preprocess_train_u8, xmh.dataset.preprocess.GpuTrainTransform).
Not a test module: tests/test_train_transform_cpu.py and tests/test_gpu_train_transform.py import it, and so does
tools/make_golden_train_transform.py, which writes tests/golden/train_transform.npz with Pillow.

Three restatements, all on the host:

* ``resize_u8(a, params, r)``: flip, crop, and Pillow's ImagingResample with the bilinear filter in plain Python doubles and
  integers -- ``precompute_coeffs`` / ``normalize_coeffs_8bpc`` operation by operation (``coeffs``), the horizontal pass, then the
  vertical one, accumulator started at 2^21, ``>> 22``, clip to [0, 255] after each pass, a pass skipped when the crop
  dimension already equals r.  Equal, to the bit, to
      Image.fromarray(a) [.transpose(FLIP_LEFT_RIGHT)] .crop((left, top, left + w, top + h)) .resize((r, r), Image.BILINEAR)
* ``to_tensor_normalize(u8)``: ToTensor + Normalize, every step in float32.
* ``draw(gen, sizes, ...)``: torchvision's published RandomHorizontalFlip.forward + RandomResizedCrop.get_params on a
  torch.Generator; it also says whether a box was accepted or is the central fallback.  torchvision itself is not a dependency
  of this repository, so the draw is pinned by its properties (tests/test_train_transform_cpu.py), not against the library.
"""
import math

import numpy as np
import torch

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
PRECISION_BITS = 32 - 8 - 2
R = 32

# name -> H, W of the source, (top, left, h, w, flip), kind of source, output size.  `stored`: the source travels in the golden
# file; the others ("formula") are regenerated from integer arithmetic alone.
CASES = {
    # crop smaller than r on both axes: upscale, 3 taps per output pixel
    "upscale":          dict(H=24, W=30, params=(2, 5, 20, 17, 0)),
    "upscale_flip":     dict(H=24, W=30, params=(2, 5, 20, 17, 1)),
    # non-integer downscale: 66 / 32 = 2.06 and 70 / 32 = 2.19 -> ceil 3 -> 7 taps on both axes
    "down7":            dict(H=74, W=70, params=(3, 2, 70, 66, 0)),
    "down7_flip":       dict(H=74, W=70, params=(3, 2, 70, 66, 1)),
    "down_odd":         dict(H=45, W=61, params=(3, 4, 37, 53, 1)),           # 1.16 / 1.66 -> 5 taps
    # passes skipped
    "w_eq_r":           dict(H=60, W=40, params=(5, 3, 50, 32, 0)),
    "h_eq_r":           dict(H=40, W=60, params=(4, 7, 32, 45, 1)),
    "both_eq_r":        dict(H=40, W=40, params=(8, 0, 32, 32, 1)),
    # the smallest crop
    "one_pixel":        dict(H=9, W=11, params=(4, 6, 1, 1, 0)),
    "one_pixel_flip":   dict(H=9, W=11, params=(8, 10, 1, 1, 1)),
    # boxes touching each edge, with and without flip (left = 0 and the right edge under flip among them)
    "edge_top":         dict(H=40, W=44, params=(0, 9, 21, 33, 0)),
    "edge_top_flip":    dict(H=40, W=44, params=(0, 9, 21, 33, 1)),
    "edge_bottom":      dict(H=40, W=44, params=(19, 9, 21, 33, 0)),
    "edge_bottom_flip": dict(H=40, W=44, params=(19, 9, 21, 33, 1)),
    "edge_left":        dict(H=40, W=44, params=(0, 0, 37, 19, 0)),
    "edge_left_flip":   dict(H=40, W=44, params=(0, 0, 37, 19, 1)),
    "edge_right":       dict(H=40, W=44, params=(3, 25, 37, 19, 0)),
    "edge_right_flip":  dict(H=40, W=44, params=(3, 25, 37, 19, 1)),
    "whole":            dict(H=40, W=44, params=(0, 0, 40, 44, 1)),
    # a saturated half: rounded taps may sum above 2^22, 255 * sum must clip, not wrap
    "saturated":        dict(H=50, W=70, params=(3, 2, 44, 65, 0), kind="half"),
    "saturated_up":     dict(H=20, W=20, params=(1, 1, 18, 17, 1), kind="half"),
    # the product's resolution
    "r224":             dict(H=300, W=400, params=(21, 40, 250, 333, 1), kind="smooth", r=224),
}

# batches: lists of (H, W, (top, left, h, w, flip), kind)
BATCHES = {
    # ragged, mixed flips, one large image: the table stride and the launch bounds come from the largest crop
    "ragged": [(40, 64, (3, 10, 30, 41, 0), "noise"), (64, 48, (0, 0, 64, 48, 1), "noise"), (50, 50, (9, 9, 32, 32, 1), "noise"),
               (300, 400, (17, 30, 270, 361, 0), "formula")],
    "single": [(40, 64, (3, 10, 30, 41, 1), "noise")],
    # same size: the stacked-tensor input
    "stacked": [(50, 50, (0, 0, 50, 50, 0), "noise"), (50, 50, (10, 5, 21, 40, 1), "noise"), (50, 50, (49, 49, 1, 1, 0), "noise"),
                (50, 50, (1, 2, 32, 45, 1), "noise"), (50, 50, (18, 0, 32, 32, 0), "noise")],
}


def source(H, W, seed, kind="noise"):
    """uint8 [H, W, 3]"""
    if kind == "smooth":                                           # integer arithmetic only; slow ramps, so that its resized bytes compress
        y, x, c = np.ogrid[:H, :W, :3]
        return (((x * 3) // 4 + y // 2 + c * 85 + (x * y) // 512 + ((x // 8) ^ (y // 8)) % 5 * 6 + seed) % 256).astype(np.uint8)
    if kind == "formula":                                          # integer arithmetic only: the same bytes everywhere
        y, x, c = np.ogrid[:H, :W, :3]
        return ((x * 7 + y * 13 + c * 85 + (x * y) % 251 + ((x ^ y) & 63) * 3 + seed) % 256).astype(np.uint8)
    a = np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)
    if kind == "half":
        a[: H // 2] = 255
    return a


def case_source_of(name):
    """cases of one shape and kind (a box and its flipped twin, the family of edge boxes) share ONE source: the first such case's"""
    c = CASES[name]
    key = (c["H"], c["W"], c.get("kind", "noise"))
    return next(n for n, d in CASES.items() if (d["H"], d["W"], d.get("kind", "noise")) == key)


def case_inputs(name):
    """-> (source uint8 [H, W, 3], params int64 [5], r)"""
    c = CASES[name]
    seed = 1000 + sorted(CASES).index(case_source_of(name))
    return source(c["H"], c["W"], seed, c.get("kind", "noise")), np.asarray(c["params"], dtype=np.int64), c.get("r", R)


def case_stored(name):
    """does the golden file hold this case's source under its own name (img_<name>)?  Formula sources are regenerated, shared ones
    are stored once, under the case they come from"""
    return CASES[name].get("kind", "noise") not in ("formula", "smooth") and case_source_of(name) == name


def batch_source_of(name, i):
    """index of the first image of the batch with the shape and kind of image i: they share a source"""
    spec = BATCHES[name]
    return next(j for j, t in enumerate(spec) if (t[0], t[1], t[3]) == (spec[i][0], spec[i][1], spec[i][3]))


def batch_inputs(name):
    """-> (list of uint8 [H, W, 3], params int64 [B, 5])"""
    spec = BATCHES[name]
    base = 2000 + 100 * sorted(BATCHES).index(name)
    return ([source(H, W, base + batch_source_of(name, i), kind) for i, (H, W, _, kind) in enumerate(spec)],
            np.asarray([p for _, _, p, _ in spec], dtype=np.int64))


def golden_source(g, name, regenerated):
    """the source of golden entry `name` (a case, or `<batch>.<i>`) as the golden file `g` stores it; the regenerated array for the
    formula sources, which are not stored"""
    if "." in name:
        b, i = name.split(".")
        kind, key = BATCHES[b][int(i)][3], "img_%s.%d" % (b, batch_source_of(b, int(i)))
    else:
        kind, key = CASES[name].get("kind", "noise"), "img_" + case_source_of(name)
    return regenerated if kind in ("formula", "smooth") else g[key]


# the float stage is one function of the uint8 result per pixel: a few cases pin it in the golden file, every case against the restatement
F32_CASES = ("upscale", "down7_flip", "both_eq_r", "one_pixel", "edge_right_flip", "saturated")


def taps(in_size, out_size):
    """tap count per output pixel: 2 * ceil(max(in / out, 1)) + 1"""
    return 2 * int(math.ceil(max(in_size / out_size, 1.0))) + 1


# ---- Pillow's ImagingResample, bilinear ---------------------------------------------------------------------------------------
def _bilinear(x):
    if x < 0.0:
        x = -x
    if x < 1.0:
        return 1.0 - x
    return 0.0


def coeffs(in_size, out_size):
    """precompute_coeffs + normalize_coeffs_8bpc for the whole-image box: bounds [out][2] = (first input index, tap count),
    kk [out][ksize] int taps with 22 fractional bits.  Python floats are C doubles, int() truncates like the C cast."""
    scale = in_size / out_size
    filterscale = scale
    if filterscale < 1.0:
        filterscale = 1.0
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds, kk = np.zeros((out_size, 2), dtype=np.int64), np.zeros((out_size, ksize), dtype=np.int64)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        ww = 0.0
        ss = 1.0 / filterscale
        xmin = int(center - support + 0.5)
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        xmax -= xmin
        k = []
        for x in range(xmax):
            w = _bilinear((x + xmin - center + 0.5) * ss)
            k.append(w)
            ww += w                                                   # left to right
        for x in range(xmax):
            if ww != 0.0:
                k[x] /= ww
        for x in range(xmax):
            kk[xx, x] = int(-0.5 + k[x] * (1 << PRECISION_BITS)) if k[x] < 0 else int(0.5 + k[x] * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return bounds, kk


def _pass(img, bounds, kk, axis):
    a = np.moveaxis(img.astype(np.int64), axis, 0)
    out = np.empty((len(bounds),) + a.shape[1:], dtype=np.int64)
    for i, (lo, n) in enumerate(bounds):
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(kk[i, :n], a[lo: lo + n], axes=(0, 0))
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis).astype(np.uint8)


def flip_crop(a, params):
    top, left, h, w, flip = (int(v) for v in params)
    if flip:
        a = a[:, ::-1]
    return np.ascontiguousarray(a[top: top + h, left: left + w])


def resize_u8(a, params, r=R):
    """uint8 [H, W, 3] -> uint8 [r, r, 3]: flip, crop, horizontal pass, vertical pass"""
    c = flip_crop(a, params)
    if c.shape[1] != r:
        c = _pass(c, *coeffs(c.shape[1], r), axis=1)
    if c.shape[0] != r:
        c = _pass(c, *coeffs(c.shape[0], r), axis=0)
    return c


def to_tensor_normalize(u8, mean=CLIP_MEAN, std=CLIP_STD):
    """ToTensor + Normalize: [r, r, 3] uint8 -> [3, r, r] float32, every step rounded to float32"""
    x = u8.transpose(2, 0, 1).astype(np.float32) / np.float32(255.0)
    m, s = np.asarray(mean, np.float32)[:, None, None], np.asarray(std, np.float32)[:, None, None]
    return ((x - m) / s).astype(np.float32)


def transform(a, params, r=R):
    return to_tensor_normalize(resize_u8(a, params, r))


def pillow_resize_u8(a, params, r=R):
    """the same through Pillow itself"""
    from PIL import Image
    top, left, h, w, flip = (int(v) for v in params)
    im = Image.fromarray(a)
    if flip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    return np.asarray(im.crop((left, top, left + w, top + h)).resize((r, r), Image.BILINEAR), dtype=np.uint8)


# ---- the draw ------------------------------------------------------------------------------------------------------------------
def draw_one(gen, H, W, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), p=0.5):
    """-> ((top, left, h, w, flip), accepted).  Calls on the generator, in order: rand(1) for the flip; per attempt one uniform
    for the area fraction and one for the log-ratio (bounds held as float32); on acceptance randint for top, then for left."""
    flip = int(bool(torch.rand(1, generator=gen) < p))
    area = H * W
    log_ratio = torch.log(torch.tensor(ratio))
    for _ in range(10):
        target_area = area * torch.empty(1).uniform_(scale[0], scale[1], generator=gen).item()
        aspect_ratio = torch.exp(torch.empty(1).uniform_(float(log_ratio[0]), float(log_ratio[1]), generator=gen)).item()
        w = int(round(math.sqrt(target_area * aspect_ratio)))
        h = int(round(math.sqrt(target_area / aspect_ratio)))
        if 0 < w <= W and 0 < h <= H:
            i = torch.randint(0, H - h + 1, size=(1,), generator=gen).item()
            j = torch.randint(0, W - w + 1, size=(1,), generator=gen).item()
            return (i, j, h, w, flip), True
    in_ratio = float(W) / float(H)
    if in_ratio < min(ratio):
        w = W
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = H
        w = int(round(h * max(ratio)))
    else:
        w, h = W, H
    return ((H - h) // 2, (W - w) // 2, h, w, flip), False


def draw(gen, sizes, **kw):
    out = [draw_one(gen, H, W, **kw) for H, W in sizes]
    return np.asarray([o[0] for o in out], dtype=np.int64).reshape(-1, 5), np.asarray([o[1] for o in out], dtype=bool)
