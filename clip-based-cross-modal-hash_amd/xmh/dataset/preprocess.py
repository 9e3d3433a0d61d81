"""GPU evaluation transform: the reference's ``Resize((r, r), BICUBIC) + ToTensor + Normalize`` (reference
dataset/transformer_dataset.py:38-42) on raw RGB uint8 batches, bit-exact with Pillow's resample, through
``xmh_image_preprocess_u8``.  The host only builds the per-size coefficient tables (a few hundred doubles, cached).

GPU training transform beside it: ``RandomHorizontalFlip + RandomResizedCrop(r) + ToTensor + Normalize`` (reference
dataset/transformer_dataset.py:34-40) on ragged batches through ``xmh_image_preprocess_train_u8``: the host draws and checks the
boxes, the device builds Pillow's bilinear tables per image and resamples (``GpuTrainTransform``)."""
from __future__ import annotations

import ctypes
import math
from typing import Dict, Tuple

import numpy as np
import torch

from .._lib import check, current_stream, lib, ptr, workspace

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)          # reference dataset/transformer_dataset.py:41
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
_PRECISION_BITS = 32 - 8 - 2


def resample_tables(in_size: int, out_size: int) -> Tuple[np.ndarray, np.ndarray]:
    """Pillow's bicubic coefficient tables for resizing ``in_size`` -> ``out_size`` pixels (whole-image box):
    bounds int32 [out, 2] = (first input index, tap count), kk int32 [out, ksize] = taps with 22 fractional bits.
    All arithmetic in float64 in Pillow's own order (the tap sum runs left to right)."""
    scale = float(in_size) / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)              # C (int) truncation; operands are positive or clamped
    xmin = np.where(center - support + 0.5 < 0, 0, xmin)
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    taps = np.arange(ksize, dtype=np.float64)[None, :]
    x = (taps + xmin[:, None] - center[:, None] + 0.5) * (1.0 / filterscale)
    ax = np.abs(x)
    a = -0.5
    w = np.where(ax < 1.0, ((a + 2.0) * ax - (a + 3.0)) * ax * ax + 1, np.where(ax < 2.0, (((ax - 5) * ax + 8) * ax - 4) * a, 0.0))
    live = taps < xmax[:, None]
    w = np.where(live, w, 0.0)
    ww = np.zeros(out_size, np.float64)
    for t in range(ksize):                                                        # left-to-right like the C loop
        ww = ww + w[:, t]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    q = np.where(w < 0, -0.5 + w * (1 << _PRECISION_BITS), 0.5 + w * (1 << _PRECISION_BITS))
    kk = np.where(live, np.trunc(q), 0.0).astype(np.int64).astype(np.int32)
    bounds = np.stack([xmin, xmax], 1).astype(np.int32)
    return bounds, kk


class GpuEvalTransform:
    """``transform(images_u8)``: uint8 RGB ``[B, H, W, 3]`` (or ``[H, W, 3]``), CPU or CUDA -> float32 ``[B, 3, r, r]`` on the GPU,
    equal to stacking the reference's eval transform over the batch."""

    def __init__(self, resolution: int = 224, mean=CLIP_MEAN, std=CLIP_STD):
        self.resolution = int(resolution)
        self._mean = (ctypes.c_float * 3)(*mean)
        self._std = (ctypes.c_float * 3)(*std)
        self._tables: Dict[tuple, tuple] = {}

    def _table(self, in_size: int, device) -> tuple:
        key = (in_size, str(device))
        t = self._tables.get(key)
        if t is None:
            b, k = resample_tables(in_size, self.resolution)
            t = (torch.from_numpy(b).to(device), torch.from_numpy(np.ascontiguousarray(k)).to(device), int(k.shape[1]))
            self._tables[key] = t
        return t

    def _run(self, images: torch.Tensor, want_u8: bool, want_f32: bool):
        if not torch.cuda.is_available():
            raise RuntimeError("GpuEvalTransform needs an MI355X; there is no CPU fallback")
        if images.dtype != torch.uint8:
            raise TypeError("GpuEvalTransform takes raw uint8 RGB images, got %s" % images.dtype)
        if images.dim() == 3:
            images = images.unsqueeze(0)
        if images.dim() != 4 or images.shape[-1] != 3:
            raise ValueError("expected [B, H, W, 3] uint8, got %s" % (tuple(images.shape),))
        if not images.is_cuda:
            images = images.cuda(non_blocking=True)
        images = images.contiguous()
        B, H, W, _ = images.shape
        r, dev = self.resolution, images.device
        bw = kw = bh = kh = None
        ksw = ksh = 0
        tmp = None
        if W != r:
            bw, kw, ksw = self._table(W, dev)
            tmp = torch.empty(B, H, r, 3, dtype=torch.uint8, device=dev)
        if H != r:
            bh, kh, ksh = self._table(H, dev)
        out_u8 = torch.empty(B, r, r, 3, dtype=torch.uint8, device=dev) if want_u8 else None
        out_f = torch.empty(B, 3, r, r, dtype=torch.float32, device=dev) if want_f32 else None
        check(lib.xmh_image_preprocess_u8(ptr(images), B, H, W, r, r, ptr(bw), ptr(kw), ksw, ptr(bh), ptr(kh), ksh,
                                          ctypes.cast(self._mean, ctypes.c_void_p), ctypes.cast(self._std, ctypes.c_void_p),
                                          ptr(tmp), ptr(out_u8), ptr(out_f), current_stream()), "xmh_image_preprocess_u8")
        return out_u8, out_f

    def __call__(self, images) -> torch.Tensor:
        """a stacked uint8 batch, or a list of [H, W, 3] uint8 photos of any sizes (one launch pair per size group)."""
        if isinstance(images, (list, tuple)):
            if not images:
                raise ValueError("empty image list")
            dev = images[0].device if images[0].is_cuda else torch.device("cuda", torch.cuda.current_device())
            out = torch.empty(len(images), 3, self.resolution, self.resolution, dtype=torch.float32, device=dev)
            groups: Dict[tuple, list] = {}
            for i, im in enumerate(images):
                groups.setdefault(tuple(im.shape), []).append(i)
            for shape, idx in groups.items():
                batch = torch.stack([images[i] if images[i].is_cuda else images[i].to(dev, non_blocking=True) for i in idx])
                res = self._run(batch, False, True)[1]
                out[torch.tensor(idx, device=out.device)] = res
            return out
        return self._run(images, False, True)[1]

    def resize_u8(self, images: torch.Tensor) -> torch.Tensor:
        """only the Pillow-exact resize: uint8 [B, r, r, 3]."""
        return self._run(images, True, False)[0]


# xmh_crop_desc (include/xmh.h): one per image, uploaded with the pixels
CROP_DESC = np.dtype([("offset", "<i8"), ("H", "<i4"), ("W", "<i4"), ("top", "<i4"), ("left", "<i4"), ("h", "<i4"), ("w", "<i4"),
                      ("flip", "<i4"), ("reserved", "<i4")])
assert CROP_DESC.itemsize == 40


class GpuTrainTransform:
    """The reference's training transform (dataset/transformer_dataset.py:34-40)

        Compose([RandomHorizontalFlip(), RandomResizedCrop(r), ToTensor(), Normalize(CLIP mean, std)])

    on a ragged batch of raw RGB uint8 photos: the host draws ``(top, left, h, w, flip)`` per image (``draw``, torchvision's
    published algorithm on a ``torch.Generator`` this object owns -- the caller's global generator is never touched), checks
    the boxes, and uploads the crop boxes' pixels with one descriptor per image; flip, crop, Pillow's antialiased bilinear resize
    and the normalisation run in three launches of ``xmh_image_preprocess_train_u8``, bit-exact with
    ``Image.fromarray(a)[.transpose(FLIP_LEFT_RIGHT)].crop(box).resize((r, r), Image.BILINEAR)``.  ``last_params`` keeps
    the parameters of the latest call."""

    def __init__(self, resolution: int = 224, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), p_flip: float = 0.5, seed=None,
                 mean=CLIP_MEAN, std=CLIP_STD):
        self.resolution = int(resolution)
        self.scale, self.ratio, self.p_flip = (float(scale[0]), float(scale[1])), (float(ratio[0]), float(ratio[1])), float(p_flip)
        self._mean = (ctypes.c_float * 3)(*mean)
        self._std = (ctypes.c_float * 3)(*std)
        self._gen = torch.Generator()
        if seed is None:
            self._gen.seed()
        else:
            self._gen.manual_seed(int(seed))
        self.last_params = None
        log_ratio = torch.log(torch.tensor(self.ratio))                          # float32, as torchvision holds them
        self._log_ratio = (float(log_ratio[0]), float(log_ratio[1]))
        self._p32 = float(torch.tensor(self.p_flip, dtype=torch.float32))
        self._u, self._k = torch.empty(1), torch.empty(1, dtype=torch.int64)     # where the draws land

    # ---- the draw (host) ---------------------------------------------------------------------------------------------------
    def _draw_one(self, H: int, W: int):
        """torchvision's RandomHorizontalFlip.forward followed by RandomResizedCrop.get_params, restated: the same draws from the
        generator in the same order (one rand for the flip; per attempt one uniform for the area, one for the log-ratio, and on
        acceptance two randints).  The draw sits on the training loop's thread, so each draw is ONE in-place op on a kept
        one-element tensor -- ``uniform_`` / ``random_`` are what ``torch.rand`` / ``torch.empty(1).uniform_`` / ``torch.randint``
        run underneath, value for value -- and the float32 log-ratio bounds are made once, in ``__init__``."""
        g, u, k = self._gen, self._u, self._k
        flip = int(u.uniform_(0.0, 1.0, generator=g).item() < self._p32)          # torch.rand(1) < p compares in float32
        area = H * W
        s0, s1 = self.scale
        lo, hi = self._log_ratio
        for _ in range(10):
            target_area = area * u.uniform_(s0, s1, generator=g).item()
            aspect = u.uniform_(lo, hi, generator=g).exp_().item()
            w = int(round(math.sqrt(target_area * aspect)))
            h = int(round(math.sqrt(target_area / aspect)))
            if 0 < w <= W and 0 < h <= H:
                top = k.random_(0, H - h + 1, generator=g).item()
                left = k.random_(0, W - w + 1, generator=g).item()
                return top, left, h, w, flip
        in_ratio = float(W) / float(H)                                            # central fallback, aspect clamped to the bounds
        if in_ratio < min(self.ratio):
            w = W
            h = int(round(w / min(self.ratio)))
        elif in_ratio > max(self.ratio):
            h = H
            w = int(round(h * max(self.ratio)))
        else:
            w, h = W, H
        return (H - h) // 2, (W - w) // 2, h, w, flip

    def draw(self, sizes) -> torch.Tensor:
        """sizes: B pairs (H, W) -> int64 [B, 5] = (top, left, h, w, flip), the box in the coordinates of the flipped image."""
        return torch.tensor([self._draw_one(int(H), int(W)) for H, W in sizes], dtype=torch.int64).reshape(-1, 5)

    # ---- the transform -----------------------------------------------------------------------------------------------------
    @staticmethod
    def _as_list(images):
        if isinstance(images, torch.Tensor):
            if images.dim() == 3:
                images = images.unsqueeze(0)
            if images.dim() != 4:
                raise ValueError("expected [B, H, W, 3] uint8, got %s" % (tuple(images.shape),))
            images = list(images.unbind(0))
        else:
            images = list(images)
        if not images:
            raise ValueError("empty image list")
        for im in images:
            if not isinstance(im, torch.Tensor) or im.dtype != torch.uint8:
                raise TypeError("GpuTrainTransform takes raw uint8 RGB images, got %s" % (getattr(im, "dtype", type(im)),))
            if im.dim() != 3 or im.shape[-1] != 3 or im.shape[0] < 1 or im.shape[1] < 1:
                raise ValueError("expected [H, W, 3] uint8 photos, got %s" % (tuple(im.shape),))
        return images

    @staticmethod
    def check_params(sizes, params) -> np.ndarray:
        """-> int64 [B, 5]; ValueError unless every box lies in its image (h, w >= 1) and flip is 0 or 1."""
        p = np.asarray(params.cpu() if isinstance(params, torch.Tensor) else params)
        if p.dtype.kind not in "iub" or p.shape != (len(sizes), 5):
            raise ValueError("params must be integers [B, 5] = (top, left, h, w, flip) for B = %d images, got %s %s" % (len(sizes), p.dtype, p.shape))
        p = p.astype(np.int64)
        hw = np.asarray(sizes, dtype=np.int64).reshape(-1, 2)
        top, left, h, w, flip = p.T
        bad = (top < 0) | (left < 0) | (h < 1) | (w < 1) | (top + h > hw[:, 0]) | (left + w > hw[:, 1]) | (flip < 0) | (flip > 1)
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            raise ValueError("image %d: box (top %d, left %d, h %d, w %d, flip %d) does not lie in its %d x %d image"
                             % (i, top[i], left[i], h[i], w[i], flip[i], hw[i, 0], hw[i, 1]))
        return p

    def pack(self, images, p: np.ndarray):
        """images (a checked list) and their checked parameters int64 [B, 5] -> (one uint8 device buffer = descriptors, padded to
        256 bytes, then the crops; bytes of descriptors; bytes of pixels).  Only the crop box of a photo travels -- rows
        [top, top + h), columns [left, left + w) of the flipped image, i.e. [W - left - w, W - left) of the stored one when
        flip is set -- so its descriptor says H = h, W = w, top = left = 0 and keeps the flip.  Photos on the host are copied into
        a pinned staging buffer behind the descriptors and go up in ONE asynchronous copy; photos already on the device are
        packed there and only the descriptors are uploaded."""
        B = len(images)
        on_dev = [im for im in images if im.is_cuda]
        dev = on_dev[0].device if on_dev else torch.device("cuda", torch.cuda.current_device())
        desc = np.zeros(B, dtype=CROP_DESC)
        nbytes = p[:, 2] * p[:, 3] * 3
        offsets = np.concatenate([[0], np.cumsum(nbytes)])
        desc["offset"] = offsets[:-1]
        desc["H"], desc["W"], desc["h"], desc["w"], desc["flip"] = p[:, 2], p[:, 3], p[:, 2], p[:, 3], p[:, 4]
        head_bytes, pixel_bytes = (desc.nbytes + 255) // 256 * 256, int(offsets[-1])       # the pixels start 256-aligned
        crops = []
        for im, (top, left, h, w, flip) in zip(images, p.tolist()):
            c0 = im.shape[1] - left - w if flip else left
            crops.append(im[top: top + h, c0: c0 + w])
        if on_dev:
            head = np.zeros(head_bytes, dtype=np.uint8)
            head[: desc.nbytes] = desc.view(np.uint8)
            packed = torch.cat([torch.from_numpy(head).to(dev, non_blocking=True)] + [c.to(dev, non_blocking=True).reshape(-1) for c in crops])
        else:
            # pinned, so the upload is asynchronous; torch's host allocator recycles the block only after that copy has finished
            host = torch.empty(head_bytes + pixel_bytes, dtype=torch.uint8, pin_memory=True)
            host[: desc.nbytes] = torch.from_numpy(desc.view(np.uint8))
            for c, lo, hi in zip(crops, (head_bytes + offsets[:-1]).tolist(), (head_bytes + offsets[1:]).tolist()):
                host[lo: hi].view(c.shape).copy_(c)
            packed = host.to(dev, non_blocking=True)
        return packed, head_bytes, pixel_bytes

    def launch(self, packed: torch.Tensor, head_bytes: int, pixel_bytes: int, B: int, max_h: int, max_w: int, want_u8: bool, want_f32: bool):
        """the three launches of xmh_image_preprocess_train_u8 on what ``pack`` made -> (uint8 [B, r, r, 3] or None, float32 [B, 3, r, r] or None)"""
        r, dev = self.resolution, packed.device
        ws_bytes = int(lib.xmh_image_preprocess_train_ws_bytes(B, max_h, max_w, r))
        if ws_bytes == 0:
            raise ValueError("crops of up to %d x %d pixels to %d x %d: beyond what xmh_image_preprocess_train_u8 takes" % (max_h, max_w, r, r))
        with torch.cuda.device(dev):
            ws = workspace(ws_bytes, dev)
            out_u8 = torch.empty(B, r, r, 3, dtype=torch.uint8, device=dev) if want_u8 else None
            out_f = torch.empty(B, 3, r, r, dtype=torch.float32, device=dev) if want_f32 else None
            check(lib.xmh_image_preprocess_train_u8(ctypes.c_void_p(packed.data_ptr() + head_bytes), pixel_bytes, ptr(packed), B, max_h, max_w, r,
                                                    ctypes.cast(self._mean, ctypes.c_void_p), ctypes.cast(self._std, ctypes.c_void_p),
                                                    ptr(ws), ws_bytes, ptr(out_u8), ptr(out_f), current_stream()),
                  "xmh_image_preprocess_train_u8")
        return out_u8, out_f

    def _run(self, images, params, want_u8: bool, want_f32: bool):
        images = self._as_list(images)
        sizes = [(int(im.shape[0]), int(im.shape[1])) for im in images]
        if params is None:
            params = self.draw(sizes)
        p = self.check_params(sizes, params)                                      # before anything is launched
        if not torch.cuda.is_available():
            raise RuntimeError("GpuTrainTransform needs an MI355X; there is no CPU fallback")
        self.last_params = torch.from_numpy(p.copy())
        packed, head_bytes, pixel_bytes = self.pack(images, p)
        return self.launch(packed, head_bytes, pixel_bytes, len(images), int(p[:, 2].max()), int(p[:, 3].max()), want_u8, want_f32)

    def __call__(self, images, params=None) -> torch.Tensor:
        """a stacked uint8 batch [B, H, W, 3], or a list of [H, W, 3] uint8 photos of any sizes (CPU or GPU) -> float32 [B, 3, r, r]
        on the GPU; ``params`` int [B, 5] = (top, left, h, w, flip), drawn when None."""
        return self._run(images, params, False, True)[1]

    def resize_u8(self, images, params) -> torch.Tensor:
        """only flip + crop + the Pillow-exact bilinear resize: uint8 [B, r, r, 3]."""
        return self._run(images, params, True, False)[0]
