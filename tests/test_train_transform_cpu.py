"""The training image transform without a GPU: the numpy restatement of tests/train_transform_cases.py equals Pillow (where PIL
imports) and the Pillow-made goldens; the draw of GpuTrainTransform has the properties of torchvision's published algorithm; the
file layout's training split is built on request; what the host can refuse is refused before anything is launched."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import train_transform_cases as TC
from conftest import GOLDEN, ROOT


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(GOLDEN, "train_transform.npz")))


def _golden_items(g):
    """(name, source, params, r) of every golden entry: sources as the file stores them, formula sources regenerated"""
    items = []
    for name in TC.CASES:
        img, params, r = TC.case_inputs(name)
        items.append((name, TC.golden_source(g, name, img), params, r))
    for b in TC.BATCHES:
        imgs, params = TC.batch_inputs(b)
        for i, (im, p) in enumerate(zip(imgs, params)):
            name = "%s.%d" % (b, i)
            items.append((name, TC.golden_source(g, name, im), p, TC.R))
    return items


# 1 the restatement --------------------------------------------------------------------------------------------------------------
def test_restatement_equals_the_goldens(golden):
    items = _golden_items(golden)
    assert len(items) == len(TC.CASES) + sum(len(s) for s in TC.BATCHES.values())
    n_f32 = 0
    for name, img, params, r in items:
        assert np.array_equal(golden["params_" + name], params) and int(golden["r_" + name]) == r, name
        u8 = TC.resize_u8(img, params, r)
        assert u8.shape == (r, r, 3) and np.array_equal(u8, golden["u8_" + name]), name
        if "f32_" + name in golden:
            n_f32 += 1
            assert np.array_equal(TC.to_tensor_normalize(u8), golden["f32_" + name]), name
    assert n_f32 == len(TC.F32_CASES) and all("f32_" + n in golden for n in TC.F32_CASES)


def test_restatement_equals_pillow():
    pytest.importorskip("PIL")
    for name in TC.CASES:
        img, params, r = TC.case_inputs(name)
        assert np.array_equal(TC.resize_u8(img, params, r), TC.pillow_resize_u8(img, params, r)), name
    for b in TC.BATCHES:
        imgs, params = TC.batch_inputs(b)
        for i, (im, p) in enumerate(zip(imgs, params)):
            assert np.array_equal(TC.resize_u8(im, p), TC.pillow_resize_u8(im, p)), (b, i)


def test_cases_cover_what_they_name():
    """every route of the kernel has a case: tap counts 3 / 5 / 7, each pass skipped alone and both, flips at both edges"""
    r = TC.R
    p = {n: TC.CASES[n]["params"] for n in TC.CASES}
    assert TC.taps(p["upscale"][2], r) == TC.taps(p["upscale"][3], r) == 3 and max(p["upscale"][2:4]) < r
    assert TC.taps(p["down7"][2], r) == TC.taps(p["down7"][3], r) == 7 and p["down7"][2] % r and p["down7"][3] % r
    assert TC.taps(p["down_odd"][3], r) == 5
    assert p["w_eq_r"][3] == r != p["w_eq_r"][2] and p["h_eq_r"][2] == r != p["h_eq_r"][3] and p["both_eq_r"][2:4] == (r, r)
    assert p["one_pixel"][2:4] == (1, 1)
    for n, c in TC.CASES.items():
        top, left, h, w, flip = c["params"]
        assert 0 <= top and top + h <= c["H"] and 0 <= left and left + w <= c["W"] and h >= 1 and w >= 1, n
        if n.startswith("edge_"):
            side = n.split("_")[1]
            assert {"top": top == 0, "bottom": top + h == c["H"], "left": left == 0, "right": left + w == c["W"]}[side], n
            assert flip == int(n.endswith("_flip"))
    ragged = TC.BATCHES["ragged"]
    assert [s[:2] for s in ragged] == [(40, 64), (64, 48), (50, 50), (300, 400)] and {s[2][4] for s in ragged} == {0, 1}
    assert len(TC.BATCHES["single"]) == 1 and len({s[:2] for s in TC.BATCHES["stacked"]}) == 1
    # a saturated case really reaches the clip: some output pixel's taps sum above 2^22
    _, kk = TC.coeffs(p["saturated"][3], r)
    _, kh = TC.coeffs(p["saturated"][2], r)
    assert max(kk.sum(1).max(), kh.sum(1).max()) > (1 << TC.PRECISION_BITS)


# 2 the draw -----------------------------------------------------------------------------------------------------------------------
SIZES = [(375, 500), (480, 640), (500, 333), (64, 48), (33, 517), (224, 224), (7, 9), (1, 1)]


def _transform(**kw):
    from xmh.dataset.preprocess import GpuTrainTransform
    return GpuTrainTransform(**kw)


def test_draw_equals_its_restatement_and_keeps_the_published_properties():
    scale, ratio = (0.08, 1.0), (3.0 / 4.0, 4.0 / 3.0)
    t = _transform(resolution=224, seed=1814)
    sizes = SIZES * 400                                                   # 3200 draws
    got = t.draw(sizes)
    want, accepted = TC.draw(torch.Generator().manual_seed(1814), sizes)
    assert got.dtype == torch.int64 and tuple(got.shape) == (len(sizes), 5) and np.array_equal(got.numpy(), want)
    hw = np.asarray(sizes, dtype=np.int64)
    top, left, h, w, flip = want.T
    assert (h >= 1).all() and (w >= 1).all() and (top >= 0).all() and (left >= 0).all()
    assert (top + h <= hw[:, 0]).all() and (left + w <= hw[:, 1]).all() and set(np.unique(flip)) == {0, 1}
    assert 0.4 < flip.mean() < 0.6 and 0.5 < accepted.mean() < 1.0
    # accepted boxes: w = round(sqrt(ta * ar)), h = round(sqrt(ta / ar)) with ta / (H W) in [s0, s1] and ar in [r0, r1]; the unrounded
    # sides lie within 1/2 of w and h.  The float32 log / exp of the ratio bounds moves them by a few 2^-24 relative at most.
    a = accepted
    area, hf, wf = (hw[a, 0] * hw[a, 1]).astype(np.float64), h[a].astype(np.float64), w[a].astype(np.float64)
    eps = 1e-6
    assert ((wf + 0.5) * (hf + 0.5) >= scale[0] * area).all() and ((wf - 0.5) * (hf - 0.5) <= scale[1] * area).all()
    assert ((wf + 0.5) / (hf - 0.5) >= ratio[0] * (1 - eps)).all() and ((wf - 0.5) / (hf + 0.5) <= ratio[1] * (1 + eps)).all()
    # fallbacks are central and as large as the ratio bounds allow
    f = ~a
    assert (top[f] == (hw[f, 0] - h[f]) // 2).all() and (left[f] == (hw[f, 1] - w[f]) // 2).all()
    assert ((h[f] == hw[f, 0]) | (w[f] == hw[f, 1])).all()
    # other bounds are honoured too
    t2 = _transform(resolution=64, scale=(0.5, 0.6), ratio=(1.0, 1.0), p_flip=0.0, seed=3)
    p2 = t2.draw([(200, 300)] * 200).numpy()
    assert (p2[:, 4] == 0).all() and (np.abs(p2[:, 2] - p2[:, 3]) <= 1).all()
    assert (((p2[:, 2] + 0.5) * (p2[:, 3] + 0.5) >= 0.5 * 60000) & ((p2[:, 2] - 0.5) * (p2[:, 3] - 0.5) <= 0.6 * 60000)).all()
    assert (_transform(p_flip=1.0, seed=3).draw([(50, 60)] * 20).numpy()[:, 4] == 1).all()


def test_a_10_by_400_image_always_falls_back():
    """H W = 4000 and h <= 10 need target_area / aspect <= 110, i.e. target_area <= 147 < 0.08 * 4000: no attempt can be accepted"""
    for seed in range(25):
        t = _transform(seed=seed)
        p = t.draw([(10, 400)])
        assert p[0, :4].tolist() == [0, 193, 10, 13], seed
        g = torch.Generator().manual_seed(seed)
        for _ in range(1 + 20):                                          # the flip, then 10 attempts of two uniforms each
            torch.rand(1, generator=g)
        assert torch.equal(g.get_state(), t._gen.get_state()), seed
    assert _transform(seed=0).draw([(400, 10)])[0, :4].tolist() == [193, 0, 13, 10]


def test_same_seed_same_sequence_and_the_global_generator_is_untouched():
    torch.manual_seed(77)
    before = torch.get_rng_state().clone()
    a, b, c = _transform(seed=5), _transform(seed=5), _transform(seed=6)
    pa = [a.draw(SIZES) for _ in range(3)]
    pb = [b.draw(SIZES) for _ in range(3)]
    assert all(torch.equal(x, y) for x, y in zip(pa, pb)) and not torch.equal(pa[0], pa[1])
    assert not torch.equal(pa[0], c.draw(SIZES))
    d = _transform(seed=None)                                             # unseeded: a seed of its own, still not the global generator
    d.draw(SIZES)
    assert torch.equal(torch.get_rng_state(), before)


# 3 what the host refuses ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("params", [(0, 0, 9, 8, 0), (0, 0, 8, 9, 0), (-1, 0, 4, 4, 0), (0, -1, 4, 4, 0), (5, 0, 4, 4, 1), (0, 5, 4, 4, 0),
                                    (0, 0, 0, 4, 0), (0, 0, 4, 0, 1), (0, 0, 4, 4, 2), (0, 0, 4, 4, -1)])
def test_out_of_image_parameters_raise_before_any_launch(params, monkeypatch):
    from xmh import _lib
    from xmh.dataset import preprocess as P
    calls = []

    class Spy:
        def __getattr__(self, name):
            calls.append(name)
            return getattr(_lib.lib, name)
    monkeypatch.setattr(P, "lib", Spy())
    t = _transform(resolution=8, seed=1)
    ok = torch.zeros(8, 8, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="does not lie in its 8 x 8 image"):
        t([ok, ok], params=[(0, 0, 8, 8, 0), params])
    with pytest.raises(ValueError, match="does not lie"):
        t.resize_u8(torch.stack([ok, ok]), torch.tensor([params, (0, 0, 8, 8, 1)]))
    assert calls == []


def test_wrong_inputs_raise():
    t = _transform(resolution=8, seed=1)
    ok = torch.zeros(8, 8, 3, dtype=torch.uint8)
    with pytest.raises(TypeError):
        t(torch.zeros(1, 8, 8, 3))
    with pytest.raises(ValueError):
        t(torch.zeros(1, 3, 8, 8, dtype=torch.uint8))
    with pytest.raises(ValueError):
        t([])
    with pytest.raises(ValueError, match=r"\[B, 5\]"):
        t([ok], params=[(0, 0, 8, 8)])
    with pytest.raises(ValueError, match=r"\[B, 5\]"):
        t([ok, ok], params=[(0, 0, 8, 8, 0)])
    with pytest.raises(ValueError, match="integers"):
        t([ok], params=torch.tensor([[0.0, 0, 8, 8, 0]]))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            t([ok], params=[(0, 0, 8, 8, 0)])


def _entry_args(B=2, max_h=20, max_w=30, r=8, ws_bytes=None, pixels=1, desc=1, ws=1, out=1, mean=1, pixel_bytes=4000):
    """the C entry with non-null dummies: every refusal below comes before the first launch, nothing is dereferenced"""
    from xmh._lib import lib
    need = lib.xmh_image_preprocess_train_ws_bytes(B, max_h, max_w, r)
    buf = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    fp = ctypes.cast(buf, ctypes.c_void_p) if mean else None
    dummy = ctypes.c_void_p(4096)
    return lib.xmh_image_preprocess_train_u8(dummy if pixels else None, pixel_bytes, dummy if desc else None, B, max_h, max_w, r, fp, fp,
                                             dummy if ws else None, need if ws_bytes is None else ws_bytes, None, dummy if out else None, None)


def test_argument_errors_of_the_c_entry_without_a_gpu():
    from xmh import _lib
    lib = _lib.lib
    err = lambda: lib.xmh_last_error().decode()                                # noqa: E731
    assert _entry_args(B=0) == 0 and _entry_args(B=0, pixels=0, desc=0, ws=0, out=0) == 0
    assert _entry_args(B=-1) == -22 and "bad shape" in err()
    for kw in (dict(r=0), dict(max_h=0), dict(max_w=0), dict(r=1 << 17), dict(max_h=1 << 17), dict(max_w=-3)):
        assert _entry_args(**kw) == -22 and "bad shape" in err(), kw
        assert lib.xmh_image_preprocess_train_ws_bytes(kw.get("B", 2), kw.get("max_h", 20), kw.get("max_w", 30), kw.get("r", 8)) == 0
    for kw in (dict(pixels=0), dict(desc=0), dict(ws=0), dict(out=0)):
        assert _entry_args(**kw) == -22 and "null pointer" in err(), kw
    assert _entry_args(mean=0) == -22 and "mean/std" in err()
    assert _entry_args(pixel_bytes=2) == -22 and "pixel buffer" in err()
    need = lib.xmh_image_preprocess_train_ws_bytes(2, 20, 30, 8)
    assert _entry_args(ws_bytes=need - 1) == -12 and "workspace of %d bytes, %d needed" % (need - 1, need) in err()
    with pytest.raises(_lib.XmhError, match="workspace"):
        _lib.check(_entry_args(ws_bytes=0), "xmh_image_preprocess_train_u8")


def test_workspace_holds_the_tables_and_the_horizontal_rows():
    """2 * ceil(max(in / r, 1)) + 1 taps per output pixel on each axis, (first, count) bounds, max_h rows of r pixels per image"""
    from xmh._lib import lib
    for B, max_h, max_w, r in ((1, 1, 1, 32), (4, 270, 361, 32), (128, 480, 640, 224), (3, 32, 32, 32), (5, 65, 33, 32)):
        need = 4 * B * r * (2 + 2 + TC.taps(max_w, r) + TC.taps(max_h, r)) + 3 * B * max_h * r
        got = lib.xmh_image_preprocess_train_ws_bytes(B, max_h, max_w, r)
        assert need <= got <= need + 5 * 256, (B, max_h, max_w, r)


def test_binding_mirrors_the_header():
    from xmh import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "xmh.h")).read(), flags=re.S)
    for name in ("xmh_image_preprocess_train_ws_bytes", "xmh_image_preprocess_train_u8"):
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, header).group(1)
        assert decl.count(",") + 1 == len(_lib.PROTOTYPES[name][1]), name
    from xmh.dataset.preprocess import CROP_DESC
    struct = re.search(r"typedef struct \{([^}]*)\} xmh_crop_desc;", header).group(1)
    fields = [f.strip() for decl in struct.split(";") if decl.strip() for f in decl.strip().split(" ", 1)[1].split(",")]
    assert fields == list(CROP_DESC.names) and CROP_DESC.itemsize == 40


# 4 the file layout's training split ----------------------------------------------------------------------------------------------
class _Words:
    def tokenize(self, text):
        return str(text).strip().lower().split()

    def convert_tokens_to_ids(self, tokens):
        return [49406 if t == "<|startoftext|>" else 49407 if t == "<|endoftext|>" else 1 + sum(map(ord, t)) % 4000 for t in tokens]


def test_build_dataloader_gives_the_training_split_on_request(tmp_path):
    import scipy.io as scio
    from PIL import Image
    import xmh.dataset  # noqa: F401
    from xmh.dataset import build_dataloader
    from xmh.dataset.transformer_dataset import TransformerDataset
    rng = np.random.default_rng(5)
    n, C = 12, 4
    paths = []
    for i in range(n):
        h, w = [(20, 32), (32, 24), (25, 25)][i % 3]
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), mode="RGB").save(tmp_path / ("img%02d.png" % i))
        paths.append(str(tmp_path / ("img%02d.png" % i)))
    labels = (rng.random((n, C)) < 0.4).astype(np.int64)
    scio.savemat(tmp_path / "index.mat", {"index": np.asarray(paths)})
    scio.savemat(tmp_path / "caption.mat", {"caption": np.asarray([["photo number %d" % i] for i in range(n)])})
    scio.savemat(tmp_path / "label.mat", {"category": labels})
    files = dict(captionFile=str(tmp_path / "caption.mat"), indexFile=str(tmp_path / "index.mat"), labelFile=str(tmp_path / "label.mat"))
    common = dict(imageResolution=32, query_num=3, train_num=5, dataset_cls="transformer_dataset", tokenizer=_Words(), maxWords=8)
    np.random.seed(4)
    train, query, retrieval = build_dataloader(**files, **common)
    assert train is None and len(query) == 3 and len(retrieval) == n - 3 and not query.is_train and not retrieval.is_train
    np.random.seed(4)
    train, query2, retrieval2 = build_dataloader(**files, train_split=True, **common)
    assert isinstance(train, TransformerDataset) and train.is_train is True and len(train) == 5
    assert not query2.is_train and not retrieval2.is_train and len(query2) == 3 and len(retrieval2) == n - 3
    # the training set is the head of the retrieval set (reference dataset/builder.py:14-15)
    assert [str(x).strip() for x in train.indexs] == [str(x).strip() for x in retrieval2.indexs[:5]]
    assert torch.equal(train.get_all_label(), retrieval2.get_all_label()[:5])
    image, caption, mask, label, index = train[1]
    assert image.dtype == torch.uint8 and image.dim() == 3 and image.shape[-1] == 3 and tuple(caption.shape) == (8,)
    assert np.array_equal(image.numpy(), np.asarray(Image.open(str(train.indexs[1]).strip()).convert("RGB")))
    batch = TransformerDataset.collate([train[i] for i in range(5)])
    assert isinstance(batch[0], list) and all(im.dtype == torch.uint8 for im in batch[0])
    # constructed directly, as the reference's registry does
    direct = TransformerDataset(captions=train.captions, indexs=train.indexs, labels=train.labels, tokenizer=_Words(), maxWords=8)
    assert direct.is_train is True and len(direct) == 5
