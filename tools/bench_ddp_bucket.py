#!/usr/bin/env python3
"""Pack and unpack of the gradient bucket (csrc/xmh_bucket.hip, xmh/ddp.py) on the parameter list of the full-size ViT-B/32 DCMHT
model (synthetic shapes, random gradients), against torch's own route in the same run:

  pack    xmh_bucket_pack(scale = 1 / W), one launch                 vs  torch._utils._flatten_dense_tensors(grads).mul_(1 / W)
  unpack  xmh_bucket_unpack, one launch                              vs  _unflatten_dense_tensors(flat, grads) and one copy_ per tensor

python tools/bench_ddp_bucket.py [--steps 30] [--warmup 5] [--world 8] [--bits 64] [--out FILE]

Times are device-event times around one call each (median and minimum over --steps, after --warmup calls), alternating the two
routes.  Bytes moved: 8 per element (4 read, 4 written) for our pack and unpack; the torch pack reads and writes the flat buffer a
second time for the scaling (16 per element).  Both are reported as a fraction of the 8 TB/s HBM peak of the specification and of the
6.29 TB/s a float4 copy reaches on this part.  The device tables are uploaded before the timed window: a training step re-uploads
them only when a gradient's address or presence changes."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "clip-based-cross-modal-hash_amd"))

PEAK, COPY = 8.0e12, 6.29e12


def timed(fn, steps, warmup):
    ev = []
    for i in range(warmup + steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        if i >= warmup:
            ev.append((a, b))
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in ev]
    return statistics.median(ms), min(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--bits", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import xmh.models  # noqa: F401
    from torch._utils import _flatten_dense_tensors, _unflatten_dense_tensors
    from xmh import _lib, ddp
    from xmh.models.dcmht import DCMHT
    from xmh.utils.config import Config
    model = DCMHT.from_config(Config({"clip_path": "synthetic:1814"}), output_dim=a.bits)
    shapes = [tuple(p.shape) for p in model.parameters() if p.numel() > 0]
    del model
    gen = torch.Generator(device="cuda").manual_seed(1814)
    grads = [torch.randn(s, device="cuda", generator=gen) * 0.01 for s in shapes]
    outs = [torch.empty_like(g) for g in grads]
    numels = [g.numel() for g in grads]
    numel = sum(numels)
    scale = 1.0 / a.world
    offsets, tail, total = ddp.bucket_layout(numels)
    cmap = ddp.chunk_map(numels, int(_lib.lib.xmh_bertadam_chunk()))
    up = lambda t: torch.from_numpy(t.view(np.uint8).reshape(-1).copy()).cuda()        # noqa: E731
    d_map, d_pack = up(cmap), up(ddp.bucket_table([g.data_ptr() for g in grads], numels))
    d_unpack = up(ddp.bucket_table([o.data_ptr() for o in outs], numels, flags=False))
    flat = torch.zeros(total, device="cuda")

    def ours_pack():
        _lib.check(_lib.lib.xmh_bucket_pack(_lib.ptr(d_pack), len(numels), _lib.ptr(d_map), len(cmap), scale, _lib.ptr(flat),
                                            _lib.current_stream()), "xmh_bucket_pack")

    def ours_unpack():
        _lib.check(_lib.lib.xmh_bucket_unpack(_lib.ptr(d_unpack), len(numels), _lib.ptr(d_map), len(cmap), _lib.ptr(flat),
                                              _lib.current_stream()), "xmh_bucket_unpack")

    kept = {}

    def torch_pack():
        kept["flat"] = _flatten_dense_tensors(grads).mul_(scale)

    def torch_unpack():
        for o, v in zip(outs, _unflatten_dense_tensors(kept["flat"], grads)):
            o.copy_(v)

    res = {}
    with torch.no_grad():
        for _ in range(2):                                                               # alternate the routes; the second round counts
            for name, fn in (("ours pack", ours_pack), ("torch pack", torch_pack), ("ours unpack", ours_unpack), ("torch unpack", torch_unpack)):
                res[name] = timed(fn, a.steps, a.warmup)
        ours_pack()
        torch_pack()
        torch.cuda.synchronize()
        same = all(torch.equal(flat[o:o + n], kept["flat"][s:s + n]) for o, n, s in zip(offsets, numels, np.cumsum([0] + numels[:-1]).tolist()))
    nbytes = {"ours pack": 8 * numel, "torch pack": 16 * numel, "ours unpack": 8 * numel, "torch unpack": 8 * numel}
    lines = [
        "gradient bucket, %d tensors, %.1f M parameters (ViT-B/32 + DCMHT heads, %d bits), scale 1 / %d, bucket of %.1f M floats in %d chunks"
        % (len(shapes), numel / 1e6, a.bits, a.world, total / 1e6, len(cmap)),
        "device %s, torch %s, %d timed calls after %d warm-up calls, device-event time per call; packed ranges equal torch's to the bit: %s"
        % (torch.cuda.get_device_name(0), torch.__version__, a.steps, a.warmup, same),
    ]
    for name in ("ours pack", "torch pack", "ours unpack", "torch unpack"):
        med, low = res[name]
        rate = nbytes[name] / (med * 1e-3)
        lines.append("%-13s median %8.3f ms  min %8.3f ms   %.3f GB moved, %.2f TB/s at the median = %.1f %% of 8 TB/s, %.1f %% of the 6.29 TB/s copy rate"
                     % (name, med, low, nbytes[name] / 1e9, rate / 1e12, 100.0 * rate / PEAK, 100.0 * rate / COPY))
    lines.append("ratio torch / ours: pack %.2fx, unpack %.2fx (event medians)"
                 % (res["torch pack"][0] / res["ours pack"][0], res["torch unpack"][0] / res["ours unpack"][0]))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
