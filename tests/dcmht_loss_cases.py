"""Shared by tests/test_dcmht_loss_cpu.py and tests/test_gpu_dcmht_loss.py (not a test module): the DCMHT objective (reference
models/DCMHT/DCMHT.py:72-149) restated in the caller's dtype, the cases of the GPU module with their seeded inputs, the conditions
those inputs must meet, and the error measure with its yardstick.

The restatement.  `terms` is oracle.losses.similarity_loss / our_loss op for op, except that it keeps the dtype it is handed:
float64 is the oracle, float32 on one CPU thread is the yardstick (what the reference's own expression loses at that shape).

Inputs.  soft: softmax of random logits (what the older tests draw: every pair lies inside the euclidean margin).  saturated:
every row is one base bit pattern, shared by both modalities, with each bit flipped with a per-row probability p_i ~ U(0, 1);
logits SHARP * (+-1 + 0.3 noise), emitted as softmax pairs -- near-one-hot codes as a trained head emits them, with pairs beyond
the margin m = sqrt(2 K vartheta) (the inactive hinge branch) and pairs at nearly zero distance.  centred: randn rows, a quarter of
the image rows being noisy copies of text rows, so that cosines fall below the lower clamp, inside, and above the upper clamp.

Conditions (on the inputs, not measurements of the port).  Cosine: the gradient jumps at the clamp edges, so a pair that fp32
puts on the other side of an edge is a different function, not a rounding error: every pair cosine of the three pair terms keeps
GAP = 2e-5 (about 100 x the fp32 rounding of a normalised dot product) from both edges in float64; rows that do not are redrawn
from the case's generator.  Euclidean: loss and gradient are continuous at s = m, no gap is needed; a saturated case has at least
MIN_BEYOND of its non-relevant pairs beyond the margin in each pair term.

Error measure.  rel_err = max|x - ref| / max|ref| on whole tensors (the nine terms as one vector, each gradient).  The yardstick
per kind is max(pool, e_ref of the case): pool = the reference's own fp32 numbers of tests/golden/loss_dcmht.npz against the float64
restatement over the four golden cases, e_ref = the float32 restatement against the float64 one at the case's own inputs (the rule
of tests/test_gpu_block_grad.py for shapes outside the goldens)."""
import contextlib

import numpy as np
import torch

from oracle import losses as OL

TERMS = OL.DCMHT_TERMS
KINDS = ("terms", "g_img", "g_txt")
SEED = 1814
VARTHETA, THRESHOLD, ALPHA = 0.75, 0.1, 0.001
SHARP = 4.0
GAP = 2e-5
MIN_BEYOND = 0.03
NEAR_ZERO = 0.05                     # "nearly zero distance": s < NEAR_ZERO * m

# name -> B, K, C (None: labels=None, every sample its own class), similarity, inputs; copy = (image row, text row): that text row is
# the image row (an off-diagonal pair at distance exactly 0), zero_label: a row without any label (L_ii = 0), near_zero: every pair term
# has off-diagonal pairs closer than NEAR_ZERO m (the 33 rows of the K = 128 case hold none)
CASES = {
    "b257_k16_sat": dict(B=257, K=16, C=21, sim="euclidean", inputs="saturated", near_zero=True),
    "b300_k64_sat_copy_zero": dict(B=300, K=64, C=33, sim="euclidean", inputs="saturated", near_zero=True, copy=(7, 130), zero_label=11),
    "b257_k16_cos": dict(B=257, K=16, C=21, sim="cosine", inputs="centred"),
    "b64_k64_cos": dict(B=64, K=64, C=65, sim="cosine", inputs="centred"),
    "b1_k16": dict(B=1, K=16, C=3, sim="euclidean", inputs="soft"),
    "b5_k1": dict(B=5, K=1, C=1, sim="euclidean", inputs="soft"),
    "b33_k128_sat": dict(B=33, K=128, C=64, sim="euclidean", inputs="saturated"),
    "b300_k16_nolabels": dict(B=300, K=16, C=None, sim="euclidean", inputs="saturated", near_zero=True),
}

# B = 6, K = 4: what is poked into the image codes, and the terms the reference's expression then reports as NaN (every entry of
# both gradients is NaN in all three: the matrix products of the backward sum over the poisoned row)
NONFINITE = {
    "zero_row_cos": dict(sim="cosine", poke="zero_row", nan_terms=("loss", "intra_pos", "intra_neg", "inter_pos_i", "inter_neg_i")),
    "nan_cos": dict(sim="cosine", poke="nan", nan_terms=("loss", "intra_pos", "intra_neg", "inter_pos_i", "inter_neg_i", "quan_i")),
    "nan_euclid": dict(sim="euclidean", poke="nan", nan_terms=("loss", "intra_pos", "intra_neg", "inter_pos_i", "inter_neg_i", "quan_i")),
}
NONFINITE_B, NONFINITE_K, NONFINITE_C = 6, 4, 3


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def pair_terms(a, b, lsim, K, sim, vartheta=VARTHETA, threshold=THRESHOLD):
    """similarity_loss (:72-98) -> (positive, negative), in the dtype of a"""
    if sim == "euclidean":
        s = torch.cdist(a, b, p=2.0, compute_mode="donot_use_mm_for_euclid_dist")        # :78
        pos = s * lsim                                                                    # :81
        neg = s * (1 - lsim)                                                              # :82
        m = float(K * 2 * vartheta) ** 0.5                                                # :83
        neg = neg.clip(max=m)                                                             # :84
        neg = m * (1 - lsim) - neg                                                        # :85
        return pos.pow(2).mean(), neg.pow(2).mean()                                       # :87-88
    s = (a / a.norm(dim=-1, keepdim=True)) @ (b / b.norm(dim=-1, keepdim=True)).t()       # calc_utils.py:38-49
    s = s.clip(min=threshold).clip(max=1 - threshold)                                     # :93
    l = (-lsim * torch.log(s) - (1 - lsim) * torch.log(1 - s)).mean()                    # :94
    return l, l


def terms(image, text, labels, K, sim, vartheta=VARTHETA, threshold=THRESHOLD, alpha=ALPHA):
    """our_loss (:107-149) -> the nine terms in TERMS order, differentiable, in the dtype of image"""
    ls = OL.label_sim(labels).to(image.dtype)
    ip, in_ = pair_terms(image, text, ls, K, sim, vartheta, threshold)
    pi, ni = pair_terms(image, image, ls, K, sim, vartheta, threshold)
    pt, nt = pair_terms(text, text, ls, K, sim, vartheta, threshold)
    qi, qt = 1 - (2 * image - 1).pow(2).mean(), 1 - (2 * text - 1).pow(2).mean()          # :100-105
    loss = (pt + pi + ni + nt) + (ip + in_) + alpha * (qi + qt) / 2
    return [loss, ip, in_, pi, ni, pt, nt, qi, qt]


@contextlib.contextmanager
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


def restate(image, text, labels, K, sim, dtype=torch.float64, **kw):
    """image, text [B, 2K] (any float dtype, taken to `dtype`), labels [B, C] or None -> dict(terms [9], g_img, g_txt) as float64
    numpy: the terms and d loss / d image, d loss / d text of the restatement evaluated in `dtype`"""
    if labels is None:
        labels = torch.eye(image.shape[0])                                                # object_function :152-154
    a = image.detach().reshape(image.shape[0], -1).to(dtype).clone().requires_grad_(True)
    b = text.detach().reshape(text.shape[0], -1).to(dtype).clone().requires_grad_(True)
    with one_thread():
        t = terms(a, b, labels, K, sim, **kw)
        t[0].backward()
    return {"terms": np.array([float(v.detach()) for v in t], dtype=np.float64), "g_img": a.grad.double().numpy(),
            "g_txt": b.grad.double().numpy()}


def pair_grad(a, b, labels, K, sim, dtype=torch.float64):
    """d (positive + negative) / d a of one pair term (what xmh_pair_similarity_loss_grad computes with scale 1), float64 numpy"""
    x = a.detach().to(dtype).clone().requires_grad_(True)
    with one_thread():
        p, n = pair_terms(x, b.detach().to(dtype), OL.label_sim(labels).to(dtype), K, sim)
        (p + n).backward()
    return x.grad.double().numpy()


# ---- error measure and yardstick ----------------------------------------------------------------------------------------------
def rel_err(x, ref):
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(x - ref).max()) / (float(np.abs(ref).max()) or 1.0)


def errors(got, ref):
    return {k: rel_err(got[k], ref[k]) for k in KINDS}


_pool = None


def golden_pool():
    """per kind: the largest error of the reference's own fp32 run (the golden file) against the float64 restatement"""
    global _pool
    if _pool is None:
        worst = {k: 0.0 for k in KINDS}
        for name in OL.DCMHT_CASES:
            img, txt, labels, K, sim, vartheta, threshold, alpha, ref = OL.load_dcmht(name)
            gi, gt = OL.load_dcmht_grads(name)
            e = errors({"terms": ref, "g_img": gi, "g_txt": gt}, restate(img, txt, labels, K, sim, vartheta=vartheta, threshold=threshold, alpha=alpha))
            worst = {k: max(worst[k], e[k]) for k in KINDS}
        _pool = worst
    return dict(_pool)


def yardstick(e_ref):
    pool = golden_pool()
    return {k: max(pool[k], e_ref[k]) for k in KINDS}


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def _gen(name):
    return torch.Generator().manual_seed(SEED * 1000 + sorted(list(CASES) + list(NONFINITE)).index(name))


def _labels(g, B, C, zero_label=None):
    L = (torch.rand(B, C, generator=g) < 0.15).float()
    L[torch.arange(B), torch.randint(0, C, (B,), generator=g)] = 1.0
    if zero_label is not None:
        L[zero_label] = 0.0
    return L


def _soft(g, B, K):
    return torch.randn(B, K, 2, generator=g)


def _saturated(g, B, K, base):
    flip = torch.rand(B, K, generator=g) < torch.rand(B, 1, generator=g)
    bits = torch.where(flip, -base, base)[:, :, None] * torch.tensor([1.0, -1.0])
    return SHARP * (bits + 0.3 * torch.randn(B, K, 2, generator=g))


def cosines(image, text):
    """float64 cosine matrices of the three pair terms: (image, text), (image, image), (text, text)"""
    a, b = image.double(), text.double()
    a, b = a / a.norm(dim=-1, keepdim=True), b / b.norm(dim=-1, keepdim=True)
    return a @ b.t(), a @ a.t(), b @ b.t()


def _centred(g, B, K, threshold=THRESHOLD):
    D = 2 * K
    text = torch.randn(B, D, generator=g)
    image = torch.randn(B, D, generator=g)
    src = torch.randint(0, B, (B // 4,), generator=g)
    image[: B // 4] = text[src] + torch.rand(B // 4, 1, generator=g) * 0.6 * torch.randn(B // 4, D, generator=g)
    for _ in range(200):                              # redraw rows with a pair cosine within GAP of a clamp edge
        it, ii, tt = cosines(image, text)
        near = lambda c: ((c - threshold).abs() < GAP) | ((c - (1 - threshold)).abs() < GAP)     # noqa: E731
        bad_i = near(it).any(1) | near(ii).any(1)
        bad_t = near(tt).any(1)
        if not (bad_i.any() or bad_t.any()):
            return image, text
        for r in torch.nonzero(bad_i).flatten().tolist():
            image[r] = torch.randn(D, generator=g)
        for r in torch.nonzero(bad_t).flatten().tolist():
            text[r] = torch.randn(D, generator=g)
    raise AssertionError("no draw keeps every cosine %g away from the clamp edges" % GAP)


_built = {}


def build(name):
    """-> dict(B, K, C, sim, inputs, labels [B, C] or None, and either logits_i / logits_t [B, K, 2] (the codes are their softmax, taken
    where the test runs) or image / text [B, 2K] (centred codes, leaves)); the same tensors at every call"""
    if name not in _built:
        spec = CASES[name]
        B, K, C, g = spec["B"], spec["K"], spec["C"], _gen(name)
        c = dict(spec, labels=None if C is None else _labels(g, B, C, spec.get("zero_label")))
        if spec["inputs"] == "centred":
            c["image"], c["text"] = _centred(g, B, K)
        else:
            if spec["inputs"] == "saturated":
                base = torch.where(torch.rand(K, generator=g) < 0.5, -1.0, 1.0)
                c["logits_i"], c["logits_t"] = _saturated(g, B, K, base), _saturated(g, B, K, base)
            else:
                c["logits_i"], c["logits_t"] = _soft(g, B, K), _soft(g, B, K)
            if "copy" in spec:
                c["logits_t"][spec["copy"][1]] = c["logits_i"][spec["copy"][0]]
        _built[name] = c
    return _built[name]


def codes(c):
    """the two [B, 2K] fp32 code matrices of a built case, on the CPU"""
    if "image" in c:
        return c["image"], c["text"]
    B = c["B"]
    return torch.softmax(c["logits_i"], -1).reshape(B, -1), torch.softmax(c["logits_t"], -1).reshape(B, -1)


def build_nonfinite(name):
    """-> (image, text [B, 2K] fp32 with the poke applied to the image codes, labels, K, sim, frozenset of NaN terms)"""
    spec, g = NONFINITE[name], _gen(name)
    B, K = NONFINITE_B, NONFINITE_K
    image = torch.softmax(_soft(g, B, K), -1).reshape(B, -1).clone()
    text = torch.softmax(_soft(g, B, K), -1).reshape(B, -1).clone()
    labels = _labels(g, B, NONFINITE_C)
    if spec["poke"] == "zero_row":
        image[2] = 0.0
    else:
        image[1, 3] = float("nan")
    return image, text, labels, K, spec["sim"], frozenset(spec["nan_terms"])


# ---- the conditions on the inputs ---------------------------------------------------------------------------------------------
def measure(c, image, text):
    """what the conditions are about, per pair term (it = image-text, ii, tt), from float64 on the CPU.  euclidean: `beyond` = the share
    of the non-relevant pairs with s > m, `near_zero` = the share of the off-diagonal pairs with s < NEAR_ZERO m, `zero_off_diag` = the number of
    off-diagonal pairs at distance exactly 0.  cosine: `gap` = the smallest distance of a pair cosine from a clamp edge, `below` /
    `above` = the share of pairs outside the clamp on either side."""
    B, K = c["B"], c["K"]
    labels = torch.eye(B) if c["labels"] is None else c["labels"]
    rel = OL.label_sim(labels) > 0
    out = {}
    if c["sim"] == "cosine":
        for key, cs in zip(("it", "ii", "tt"), cosines(image, text)):
            out[key] = dict(gap=float(torch.minimum((cs - THRESHOLD).abs(), (cs - (1 - THRESHOLD)).abs()).min()),
                            below=float((cs < THRESHOLD).double().mean()), above=float((cs > 1 - THRESHOLD).double().mean()))
        return out
    m = float(K * 2 * VARTHETA) ** 0.5
    a, b = image.double(), text.double()
    off = ~torch.eye(B, dtype=torch.bool)
    for key, (x, y) in zip(("it", "ii", "tt"), ((a, b), (a, a), (b, b))):
        s = torch.cdist(x, y, p=2.0, compute_mode="donot_use_mm_for_euclid_dist")
        nonrel = ~rel
        out[key] = dict(beyond=float(((s > m) & nonrel).sum()) / max(int(nonrel.sum()), 1), near_zero=float(((s < NEAR_ZERO * m) & off).sum()) / max(int(off.sum()), 1),
                        zero_off_diag=int(((s == 0) & off).sum()), nonrel=float(nonrel.double().mean()))
    return out


def check_conditions(name, image, text):
    """asserts what the case promises of its inputs and returns the measurements; called by the CPU test on the CPU's codes and by
    the GPU test on the codes the device produced, before the comparison"""
    c = build(name)
    m = measure(c, image, text)
    assert torch.isfinite(image).all() and torch.isfinite(text).all(), name
    if c["sim"] == "cosine":
        for key, v in m.items():
            assert v["gap"] >= GAP, (name, key, v)
        assert m["it"]["below"] > 0.5 and m["it"]["above"] > 0 and min(1 - v["below"] - v["above"] for v in m.values()) > 0.05, (name, m)
    if c["inputs"] == "saturated":
        for key, v in m.items():
            assert v["beyond"] >= MIN_BEYOND, (name, key, v)
            assert v["near_zero"] > 0 or not c.get("near_zero"), (name, key, v)
    if "copy" in c:
        assert m["it"]["zero_off_diag"] >= 1 and torch.equal(image[c["copy"][0]], text[c["copy"][1]]), (name, m["it"])
    if c.get("zero_label") is not None:
        assert not c["labels"][c["zero_label"]].any()
    if c["labels"] is not None:
        assert c["labels"].shape == (c["B"], c["C"])
    return m


def describe(m):
    return "  ".join("%s[%s]" % (key, " ".join("%s %.3g" % kv for kv in sorted(v.items()))) for key, v in m.items())
