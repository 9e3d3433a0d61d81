"""GPU parity of the training image transform (xmh_image_preprocess_train_u8 behind GpuTrainTransform): the uint8 stage and the
float stage are bit-equal to the numpy restatement of tests/train_transform_cases.py and to the Pillow-made goldens -- no
tolerance anywhere -- for single images, ragged batches and both input forms; the call does not synchronise; the C entry refuses
what the host can see; and a DCMHT runner built on the reference's file layout trains an epoch from image files."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import train_transform_cases as TC
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

_TF, _WANT = {}, {}


def _tf(r=TC.R):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    if r not in _TF:
        from xmh.dataset.preprocess import GpuTrainTransform
        _TF[r] = GpuTrainTransform(r, seed=1814)
    return _TF[r]


def _want(key, img, params, r=TC.R):
    """the restatement of one image, computed once: (uint8 [r, r, 3], float32 [3, r, r])"""
    if key not in _WANT:
        u8 = TC.resize_u8(img, params, r)
        _WANT[key] = (u8, TC.to_tensor_normalize(u8))
    return _WANT[key]


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(GOLDEN, "train_transform.npz")))


def _run(tf, imgs, params):
    """-> (uint8 [B, r, r, 3], float32 [B, 3, r, r]) numpy"""
    ts = [torch.from_numpy(np.ascontiguousarray(a)) for a in imgs]
    p = torch.from_numpy(np.asarray(params, dtype=np.int64).reshape(-1, 5))
    return tf.resize_u8(ts, p).cpu().numpy(), tf(ts, p).cpu().numpy()


# 1 single images -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TC.CASES))
def test_single_image_cases_are_bit_exact(golden, name):
    img, params, r = TC.case_inputs(name)
    if TC.case_stored(name):
        assert np.array_equal(img, golden["img_" + name])                     # the golden's source is the case's
    u8, f32 = _run(_tf(r), [img], params)
    want_u8, want_f = _want(name, img, params, r)
    assert u8.shape == (1, r, r, 3) and f32.shape == (1, 3, r, r) and f32.dtype == np.float32
    assert np.array_equal(u8[0], want_u8) and np.array_equal(u8[0], golden["u8_" + name])
    assert np.array_equal(f32[0], want_f)
    if "f32_" + name in golden:
        assert np.array_equal(f32[0], golden["f32_" + name])


# 2 batches --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TC.BATCHES))
def test_batches_are_bit_exact(golden, name):
    imgs, params = TC.batch_inputs(name)
    u8, f32 = _run(_tf(), imgs, params)
    assert u8.shape[0] == f32.shape[0] == len(imgs)
    for i, (im, p) in enumerate(zip(imgs, params)):
        want_u8, want_f = _want((name, i), im, p)
        assert np.array_equal(u8[i], want_u8) and np.array_equal(u8[i], golden["u8_%s.%d" % (name, i)]), i
        assert np.array_equal(f32[i], want_f), i


def test_stacked_tensor_list_and_device_inputs_give_the_same_bits():
    tf = _tf()
    imgs, params = TC.batch_inputs("stacked")
    p = torch.from_numpy(params)
    stacked = torch.from_numpy(np.stack(imgs))
    as_list = [torch.from_numpy(a) for a in imgs]
    ref = tf(as_list, p)
    assert torch.equal(tf(stacked, p), ref) and torch.equal(tf(stacked.cuda(), p), ref)
    assert torch.equal(tf([a.cuda() for a in as_list], p), ref) and torch.equal(tf([as_list[0].cuda()] + as_list[1:], p), ref)
    assert torch.equal(tf.resize_u8(stacked, p), tf.resize_u8(as_list, p))
    assert torch.equal(tf.last_params, p)
    # a single [H, W, 3] photo is a batch of one
    assert torch.equal(tf(as_list[1], p[1:2]), ref[1:2])


def test_the_same_call_twice_gives_the_same_bits():
    tf = _tf()
    imgs, params = TC.batch_inputs("ragged")
    a = _run(tf, imgs, params)
    b = _run(tf, imgs, params)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_drawn_parameters_are_kept_and_applied():
    tf = _tf()
    imgs, _ = TC.batch_inputs("ragged")
    out = tf([torch.from_numpy(a) for a in imgs]).cpu().numpy()
    p = tf.last_params.numpy()
    assert p.shape == (len(imgs), 5)
    for i, im in enumerate(imgs):
        assert np.array_equal(out[i], TC.transform(im, p[i])), i


# 3 no host synchronisation -------------------------------------------------------------------------------------------------------
def test_the_transform_does_not_synchronise():
    tf = _tf()
    imgs, params = TC.batch_inputs("ragged")
    ts, p = [torch.from_numpy(a) for a in imgs], torch.from_numpy(params)
    dev_ts = [t.cuda() for t in ts]
    warm = (tf(ts, p), tf(dev_ts, p), tf.resize_u8(ts, p))                    # warm-up: allocator, kernels loaded
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = (tf(ts, p), tf(dev_ts, p), tf.resize_u8(ts, p))
        drawn = tf(ts)                                                       # the draw is host work on a CPU generator
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(torch.equal(a, b) for a, b in zip(got, warm)) and tuple(drawn.shape) == (len(ts), 3, TC.R, TC.R)


def test_three_launches_per_batch_whatever_its_size():
    """the library's own launch counters (xmh_prof_enable / xmh_prof_read): each of the three kernels runs once per call, for one
    image as for a ragged batch"""
    from xmh import _lib
    tf = _tf()
    names = ("train_tf_tables", "train_tf_h", "train_tf_v")
    _lib.prof_enable(True)
    try:
        counts = []
        for batch in ("single", "ragged", "stacked"):
            imgs, params = TC.batch_inputs(batch)
            tf([torch.from_numpy(a) for a in imgs], torch.from_numpy(params))
            counts.append([_lib.prof_read(n)[1] for n in names])
    finally:
        _lib.prof_enable(False)
    assert counts == [[1, 1, 1], [2, 2, 2], [3, 3, 3]]


# 4 the C entry ----------------------------------------------------------------------------------------------------------------------
def test_argument_errors_of_the_c_entry():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from xmh._lib import current_stream, lib, ptr
    from xmh.dataset.preprocess import CLIP_MEAN, CLIP_STD, CROP_DESC
    img, params, r = TC.case_inputs("down_odd")
    H, W = img.shape[:2]
    desc = np.zeros(1, dtype=CROP_DESC)
    desc["H"], desc["W"] = H, W
    desc["top"], desc["left"], desc["h"], desc["w"], desc["flip"] = params
    pix = torch.from_numpy(img).cuda().reshape(-1)
    d = torch.from_numpy(desc.view(np.uint8).copy()).cuda()
    need = lib.xmh_image_preprocess_train_ws_bytes(1, int(params[2]), int(params[3]), r)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    out_u8 = torch.empty(1, r, r, 3, dtype=torch.uint8, device="cuda")
    out_f = torch.empty(1, 3, r, r, dtype=torch.float32, device="cuda")
    mean, std = (ctypes.c_float * 3)(*CLIP_MEAN), (ctypes.c_float * 3)(*CLIP_STD)

    def call(B=1, max_h=int(params[2]), max_w=int(params[3]), r=r, pixels=pix, desc=d, ws=ws, ws_bytes=need, u8=out_u8, f=out_f, mean=mean, nbytes=pix.numel()):
        m = ctypes.cast(mean, ctypes.c_void_p) if mean is not None else None
        return lib.xmh_image_preprocess_train_u8(ptr(pixels), nbytes, ptr(desc), B, max_h, max_w, r, m, ctypes.cast(std, ctypes.c_void_p),
                                                 ptr(ws), ws_bytes, ptr(u8), ptr(f), current_stream())
    err = lambda: lib.xmh_last_error().decode()                                # noqa: E731
    assert call(B=-1) == -22 and call(r=0) == -22 and call(max_h=0) == -22 and call(max_w=0) == -22 and "bad shape" in err()
    assert call(pixels=None) == -22 and call(desc=None) == -22 and call(ws=None) == -22 and call(u8=None, f=None) == -22 and "null pointer" in err()
    assert call(mean=None) == -22 and "mean/std" in err()
    assert call(nbytes=2) == -22
    assert call(ws_bytes=need - 1) == -12 and "workspace" in err()
    assert call(B=0, pixels=None, desc=None) == 0
    # the raw entry with whole-image descriptors (top kept, nothing sliced on the host) gives the same bits as the transform
    assert call() == 0 and call(f=None) == 0 and call(u8=None, mean=mean) == 0
    want_u8, want_f = _want("down_odd", img, params, r)
    assert np.array_equal(out_u8.cpu().numpy()[0], want_u8) and np.array_equal(out_f.cpu().numpy()[0], want_f)


def test_whole_photo_descriptors_take_the_general_path():
    """the transform uploads crop boxes only (top = left = 0, W = w); the C entry also takes WHOLE photos with the box in the
    descriptor -- non-zero top and left, W > w, flipped and not: one ragged call, same bits as the restatement"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from xmh._lib import check, current_stream, lib, ptr
    from xmh.dataset.preprocess import CLIP_MEAN, CLIP_STD, CROP_DESC
    names = ["down7", "down_odd", "upscale", "upscale_flip", "edge_right", "edge_right_flip", "edge_bottom", "w_eq_r", "h_eq_r", "one_pixel_flip"]
    inputs = [TC.case_inputs(n) for n in names]
    B, r = len(names), TC.R
    assert {int(p[4]) for _, p, _ in inputs} == {0, 1} and any(p[0] > 0 and p[1] > 0 and p[3] < a.shape[1] for a, p, _ in inputs)
    desc = np.zeros(B, dtype=CROP_DESC)
    sizes = np.asarray([a.shape[0] * a.shape[1] * 3 for a, _, _ in inputs], dtype=np.int64)
    desc["offset"] = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    for i, (a, p, _) in enumerate(inputs):
        desc[i]["H"], desc[i]["W"] = a.shape[:2]
        desc[i]["top"], desc[i]["left"], desc[i]["h"], desc[i]["w"], desc[i]["flip"] = p
    pix = torch.from_numpy(np.concatenate([a.reshape(-1) for a, _, _ in inputs])).cuda()
    d = torch.from_numpy(desc.view(np.uint8).copy()).cuda()
    max_h, max_w = int(desc["h"].max()), int(desc["w"].max())
    need = lib.xmh_image_preprocess_train_ws_bytes(B, max_h, max_w, r)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    out_u8 = torch.empty(B, r, r, 3, dtype=torch.uint8, device="cuda")
    out_f = torch.empty(B, 3, r, r, dtype=torch.float32, device="cuda")
    mean, std = (ctypes.c_float * 3)(*CLIP_MEAN), (ctypes.c_float * 3)(*CLIP_STD)
    check(lib.xmh_image_preprocess_train_u8(ptr(pix), pix.numel(), ptr(d), B, max_h, max_w, r, ctypes.cast(mean, ctypes.c_void_p),
                                            ctypes.cast(std, ctypes.c_void_p), ptr(ws), need, ptr(out_u8), ptr(out_f), current_stream()))
    got_u8, got_f = out_u8.cpu().numpy(), out_f.cpu().numpy()
    for i, (n, (a, p, _)) in enumerate(zip(names, inputs)):
        want_u8, want_f = _want(n, a, p, r)
        assert np.array_equal(got_u8[i], want_u8) and np.array_equal(got_f[i], want_f), n


# 5 end to end: a DCMHT runner trains from image files --------------------------------------------------------------------------------
class _Recorder:
    """stands where the runner keeps its training transform: records what went in, the drawn parameters and what came out"""

    def __init__(self, tf):
        self.tf, self.seen = tf, []

    def __call__(self, images, params=None):
        out = self.tf(images, params)
        self.seen.append(([im.clone() for im in images], self.tf.last_params.clone(), out))
        return out


def _file_trainer(tmp_path, root):
    import xmh.dataset  # noqa: F401
    import xmh.models  # noqa: F401
    import xmh.runners  # noqa: F401
    from xmh.common.register import registry
    from xmh.utils.config import Config
    if registry.get_tokenizer_class("toy_words_train") is None:
        @registry.register_tokenizer("toy_words_train")
        class ToyWords:                                           # the two methods the dataset calls
            def tokenize(self, text):
                return str(text).strip().lower().split()

            def convert_tokens_to_ids(self, tokens):
                return [49406 if t == "<|startoftext|>" else 49407 if t == "<|endoftext|>" else 1 + sum(map(ord, t)) % 4000 for t in tokens]
    small = "vision_layers=1,transformer_layers=1,vision_width=128,transformer_width=128,embed_dim=64,image_resolution=64"
    cfg = Config({
        "model": {"arch": "DCMHT", "clip_path": "synthetic:1814:" + small},
        "dataset": {"arch": "transformer_dataset", "name": "tiny", "path": str(root), "label_file": "label.mat", "tokenizer_arch": "toy_words_train",
                    "max_word": 32, "image_resolution": 64},
        "optimizer": {"lr": 0.001, "backbone_lr": 0.00001},
        "run": {"arch": "DCMHTTrainer", "output_dim": 16, "device": 0, "batch_size": 4, "num_workers": 0, "is_train": True, "query_num": 5,
                "train_num": 8, "epochs": 1, "save_dir": str(tmp_path), "log_dir": str(tmp_path), "seed": 1814},
    })
    t = registry.get_runner_class("DCMHTTrainer").from_config(cfg=cfg, autorun=False)
    t.lines = []
    t.logger = types.SimpleNamespace(info=t.lines.append)
    return t


def test_dcmht_runner_trains_an_epoch_from_image_files(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import scipy.io as scio
    from PIL import Image
    rng = np.random.default_rng(11)
    root = tmp_path / "data"
    (root / "tiny").mkdir(parents=True)
    n, C = 20, 6
    paths = []
    for i in range(n):
        h, w = [(40, 64), (64, 48), (50, 50)][i % 3]
        p = root / "tiny" / ("img%02d.png" % i)
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), mode="RGB").save(p)
        paths.append(str(p))
    labels = (rng.random((n, C)) < 0.4).astype(np.int64)
    labels[:, 0] = 1
    scio.savemat(root / "tiny" / "index.mat", {"index": np.asarray(paths)})
    scio.savemat(root / "tiny" / "caption.mat", {"caption": np.asarray([["photo number %d of a dog" % i] for i in range(n)])})
    scio.savemat(root / "tiny" / "label.mat", {"category": labels})
    finals = []
    for _ in range(2):
        t = _file_trainer(tmp_path, root)
        assert t.train_loader is not None and len(t.train_loader.dataset) == 8 and t.train_loader.dataset.is_train
        assert tuple(t.train_labels.shape) == (8, C) and t.retrieval_num == n - 5
        rec = _Recorder(t._train_image_transform())
        assert rec.tf.resolution == 64 and t.__dict__["_gpu_train_transform"] is rec.tf
        t.__dict__["_gpu_train_transform"] = rec
        fed, inner = [], t.model.forward_train
        t.model.forward_train = lambda image, text: (fed.append(image), inner(image, text))[1]
        before = {k: p.detach().clone() for k, p in t.model.named_parameters()}
        t.train_epoch(0)
        assert t.global_step == len(t.train_loader) == 2 and len(rec.seen) == 2 and len(fed) == 2
        loss = float(re.search(r"loss: (?:tensor\()?([-+0-9.eE]+|nan|inf)", t.lines[-1]).group(1))
        assert np.isfinite(loss)
        for k, p in t.model.named_parameters():
            if k != "backbone.logit_scale" and (k.startswith("backbone.") or k.startswith("hash.")):
                assert not torch.equal(p.detach(), before[k]) and bool(torch.isfinite(p).all()), k
        # what the model saw is the restatement of the photos under the transform's own draw
        sizes = set()
        for (photos, params, out), image in zip(rec.seen, fed):
            assert image is out and tuple(out.shape) == (4, 3, 64, 64) and out.dtype == torch.float32 and out.is_cuda
            got = out.cpu().numpy()
            for i, ph in enumerate(photos):
                assert ph.dtype == torch.uint8
                sizes.add(tuple(ph.shape))
                assert np.array_equal(got[i], TC.transform(ph.cpu().numpy(), params[i].numpy(), 64)), i
        assert len(sizes) == 3
        finals.append(({k: p.detach().clone() for k, p in t.model.named_parameters()}, [s[1] for s in rec.seen]))
    assert all(torch.equal(finals[0][0][k], finals[1][0][k]) for k in finals[0][0])
    assert all(torch.equal(a, b) for a, b in zip(finals[0][1], finals[1][1]))
