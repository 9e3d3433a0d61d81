#!/usr/bin/env python3
"""The training image transform on the GPU (GpuTrainTransform, xmh_image_preprocess_train_u8) on a batch of COCO-like photos --
B = 128, 640 x 480 and 500 x 375 mixed, r = 224, one seeded draw of crop boxes and flips used by every side -- against the
reference's route measured in the same run: Pillow flip + crop + bilinear resize and ToTensor + Normalize on the host, one
thread and 16 threads.  python tools/bench_train_transform.py [--batch 128] [--iters 50] [--rounds 3] [--step-ms MS]
-> profiles/train_transform.txt

GPU figures come from stream events around `iters` calls after a warm-up, median of `rounds`:
  kernels    the three launches alone, on a packed buffer already on the device (GpuTrainTransform.launch)
  call       what train_epoch calls, tf(photos) with no boxes given: the draw on the host (a new one every call), pack (crop
             boxes into one pinned buffer), one upload and the three launches, from photos in host memory; beside it the
             host's wall clock per call, which is what the training loop's thread spends.  `boxes given` is the same without
             the draw, `draw` the draw alone (host clock)
  ragged     the three launches on a batch with one 1600 x 1200 photo taken whole among 127 crops of 500 x 375 photos: the
             horizontal pass is launched for B * max_h rows, most of which no image has
Bytes per call are what the algorithm needs, from the shapes: the crop's pixels read once (h w 3), the horizontal pass's rows
written and read (2 h r 3), the float output written (r r 12); the coefficient tables (a few KB per image) are left out.  The
yardstick for the byte rate is GpuEvalTransform on the same photos (whole images, bicubic, its own two byte-streaming passes:
H W 3 + 2 H r 3 + r r 12 bytes per image, its two size groups are two launch pairs and one scatter each).
The share of a training step uses the step time of tools/bench_train_step.py: --step-ms, or the figure in
profiles/train_step_bench.txt (run that tool first, in the same job, for a figure of the same machine).  No pass mark."""
import argparse
import os
import re
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "clip-based-cross-modal-hash_amd"))

SIZES = [(480, 640), (375, 500)]


def host_route(a, p, r, mean, std):
    """the reference's transform of one photo with the box already drawn: PIL flip, crop, resize, then ToTensor + Normalize"""
    from PIL import Image
    top, left, h, w, flip = (int(v) for v in p)
    im = Image.fromarray(a)
    if flip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    im = im.crop((left, top, left + w, top + h)).resize((r, r), Image.BILINEAR)
    x = torch.from_numpy(np.asarray(im).copy()).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    return x.sub_(mean).div_(std)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--resolution", type=int, default=224)
    ap.add_argument("--step-ms", type=float, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from xmh.dataset.preprocess import CLIP_MEAN, CLIP_STD, GpuEvalTransform, GpuTrainTransform
    B, r = a.batch, a.resolution
    rng = np.random.default_rng(1814)
    photos = [torch.from_numpy(rng.integers(0, 256, SIZES[i % 2] + (3,), dtype=np.uint8)) for i in range(B)]
    tf, ev = GpuTrainTransform(r, seed=1814), GpuEvalTransform(r)
    sizes = [tuple(ph.shape[:2]) for ph in photos]
    params = tf.draw(sizes)
    p = tf.check_params(sizes, params)
    max_h, max_w = int(p[:, 2].max()), int(p[:, 3].max())
    crop_bytes = int((p[:, 2] * p[:, 3] * 3).sum())
    whole_bytes = sum(h * w * 3 for h, w in sizes)
    train_bytes = crop_bytes + int((2 * p[:, 2] * r * 3).sum()) + B * r * r * 12
    eval_bytes = whole_bytes + sum(2 * h * r * 3 for h, _ in sizes) + B * r * r * 12

    def events(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(a.iters):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / a.iters * 1e-3

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.iters

    packed, head_bytes, pixel_bytes = tf.pack(photos, p)
    assert pixel_bytes == crop_bytes                           # only the crop boxes travel
    dev_photos = [ph.cuda() for ph in photos]
    # the ragged batch: one large photo taken whole among small crops
    rag_photos = [torch.from_numpy(rng.integers(0, 256, ((1200, 1600) if i == 0 else SIZES[1]) + (3,), dtype=np.uint8)) for i in range(B)]
    rag_sizes = [tuple(ph.shape[:2]) for ph in rag_photos]
    rp = tf.check_params(rag_sizes, tf.draw(rag_sizes))
    rp[0] = (0, 0, 1200, 1600, 0)
    rag_packed, rag_head, rag_pix = tf.pack(rag_photos, rp)
    rag_h, rag_w = int(rp[:, 2].max()), int(rp[:, 3].max())
    rag_bytes = int((rp[:, 2] * rp[:, 3] * 3).sum()) + int((2 * rp[:, 2] * r * 3).sum()) + B * r * r * 12
    rag_live = float(rp[:, 2].sum()) / (B * rag_h)
    del rag_photos
    sides = {
        "kernels": lambda: tf.launch(packed, head_bytes, pixel_bytes, B, max_h, max_w, False, True),
        "call": lambda: tf(photos),
        "given": lambda: tf(photos, params),
        "eval": lambda: ev(dev_photos),
        "ragged": lambda: tf.launch(rag_packed, rag_head, rag_pix, B, rag_h, rag_w, False, True),
    }
    for fn in sides.values():                                  # warm-up: code objects, allocator pools, the eval tables
        fn()
    torch.cuda.synchronize()
    got = {k: [] for k in sides}
    walls, walls_given, draws = [], [], []
    for _ in range(a.rounds):                                  # alternate the sides
        for k, fn in sides.items():
            got[k].append(events(fn))
        walls.append(wall(sides["call"]))
        walls_given.append(wall(sides["given"]))
        draws.append(wall(lambda: tf.draw(sizes)))
    med = {k: statistics.median(v) for k, v in got.items()}

    from xmh import _lib                                       # the three kernels one by one (events around each launch), a run of its own
    _lib.prof_enable(True)
    for _ in range(a.iters):
        sides["kernels"]()
    per_kernel = {n: _lib.prof_read(n) for n in ("train_tf_tables", "train_tf_h", "train_tf_v")}
    _lib.prof_enable(False)

    # the reference's route on the host, same boxes
    mean, std = torch.tensor(CLIP_MEAN)[:, None, None], torch.tensor(CLIP_STD)[:, None, None]
    arrays = [ph.numpy() for ph in photos]
    torch.set_num_threads(1)
    ref = torch.stack([host_route(x, q, r, mean, std) for x, q in zip(arrays, p)])
    assert torch.equal(tf(photos, params).cpu(), ref), "the GPU transform and the host route differ"
    host1, host16 = [], []
    for _ in range(a.rounds):
        t0 = time.perf_counter()
        torch.stack([host_route(x, q, r, mean, std) for x, q in zip(arrays, p)])
        host1.append(time.perf_counter() - t0)
        with ThreadPoolExecutor(16) as pool:
            t0 = time.perf_counter()
            torch.stack(list(pool.map(lambda xq: host_route(xq[0], xq[1], r, mean, std), zip(arrays, p))))
            host16.append(time.perf_counter() - t0)
    h1, h16 = statistics.median(host1), statistics.median(host16)

    step_ms, src = a.step_ms, "--step-ms"
    if step_ms is None:
        path = os.path.join(ROOT, "profiles", "train_step_bench.txt")
        m = re.search(r"forward_train \+ loss \+ backward \+ BertAdam\s+([0-9.]+) ms", open(path).read()) if os.path.exists(path) else None
        step_ms, src = (float(m.group(1)), "profiles/train_step_bench.txt") if m else (None, None)

    span = lambda v: "(%.3f .. %.3f)" % (min(v) * 1e3, max(v) * 1e3)                    # noqa: E731
    out = ["tools/bench_train_transform.py on %s" % torch.cuda.get_device_name(0),
           "training transform, %d photos (%s mixed) -> %d x %d, one seeded draw: crops up to %d x %d, %.1f MB of crop pixels sent "
           "(whole photos: %.1f MB)" % (B, " and ".join("%dx%d" % (w, h) for h, w in SIZES), r, r, max_h, max_w, crop_bytes / 1e6, whole_bytes / 1e6),
           "  %d rounds of %d calls per side, alternating; median (min .. max); the result equals the host route to the bit" % (a.rounds, a.iters),
           "  GPU, three launches on a packed device buffer   %8.3f ms %s  %6.1f MB algorithmic -> %7.1f GB/s" % (
               med["kernels"] * 1e3, span(got["kernels"]), train_bytes / 1e6, train_bytes / med["kernels"] / 1e9),
           "    of which, events around each launch (%d calls): %s" % (
               a.iters, ", ".join("%s %.4f ms" % (n[len("train_tf_"):], v[0]) for n, v in per_kernel.items())),
           "  ragged batch (one 1600x1200 photo whole, crops up to %d x %d; %.0f %% of the horizontal pass's rows exist): three launches "
           "%8.3f ms %s  %6.1f MB algorithmic -> %7.1f GB/s" % (rag_h, rag_w, 100 * rag_live, med["ragged"] * 1e3, span(got["ragged"]),
                                                                 rag_bytes / 1e6, rag_bytes / med["ragged"] / 1e9),
           "  GPU, whole call as train_epoch makes it: draw + pack + upload + launches (events) %8.3f ms %s  host wall clock per call %.3f ms %s" % (
               med["call"] * 1e3, span(got["call"]), statistics.median(walls) * 1e3, span(walls)),
           "    the same with the boxes given (no draw)       %8.3f ms %s  host wall clock per call %.3f ms %s" % (
               med["given"] * 1e3, span(got["given"]), statistics.median(walls_given) * 1e3, span(walls_given)),
           "    the draw alone, %d boxes on the host          %8.3f ms %s (host clock)" % (B, statistics.median(draws) * 1e3, span(draws)),
           "  GpuEvalTransform on the same photos (on device) %8.3f ms %s  %6.1f MB algorithmic -> %7.1f GB/s" % (
               med["eval"] * 1e3, span(got["eval"]), eval_bytes / 1e6, eval_bytes / med["eval"] / 1e9),
           "  byte rate of the training kernels / of the evaluation transform: %.2f" % ((train_bytes / med["kernels"]) / (eval_bytes / med["eval"])),
           "  host route with the boxes given (Pillow + ToTensor + Normalize), 1 thread   %8.2f ms %s  = %.0f x the whole GPU call" % (
               h1 * 1e3, span(host1), h1 / statistics.median(walls)),
           "  host route, 16 threads                                  %8.2f ms %s  = %.0f x the whole GPU call" % (
               h16 * 1e3, span(host16), h16 / statistics.median(walls))]
    if step_ms:
        out.append("  one DCMHT training step (%s): %.2f ms; the whole call with its draw is %.1f %% of it in host time (the draw %.1f %%), the three "
                   "launches %.2f %% in GPU time" % (src, step_ms, 100 * statistics.median(walls) * 1e3 / step_ms,
                                                     100 * statistics.median(draws) * 1e3 / step_ms, 100 * med["kernels"] * 1e3 / step_ms))
    else:
        out.append("  one DCMHT training step: not measured (run tools/bench_train_step.py first, or give --step-ms)")
    for s in out:
        print(s)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "train_transform.txt"), "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
