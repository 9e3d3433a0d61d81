#!/usr/bin/env python3
"""BertAdam step time on the parameter list of the full-size ViT-B/32 DCMHT model (synthetic weights, random gradients):
the fused HIP step (xmh/optim.py, two launches) against the same step restated with the reference's sequence of torch ops per
parameter (models/common/optimizer.py:112-165), in the same run.

python tools/bench_bertadam.py [--steps 20] [--warmup 3] [--bits 64] [--out FILE]

Times are device-event times around one step() each (median and minimum over --steps), after --warmup steps; the gradients are
restored before every step outside the timed window, because a clipped gradient is written back and would not be clipped again.
Bytes moved: 4 per element for the norm, 16 read and 12 written by the update, 4 more where the tensor was clipped; reported
as a fraction of the 8 TB/s HBM peak.  The wall time per step (host loop included, one synchronisation at the end) is
printed beside the event time: the fused step's host side builds a table of a few hundred rows in Python."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "clip-based-cross-modal-hash_amd"))

PEAK = 8.0e12
HYPER = dict(lr=1e-3, warmup=0.1, t_total=1000, schedule="warmup_cosine", b1=0.9, b2=0.98, e=1e-6, weight_decay=0.2, max_grad_norm=1.0)


def reference_step(params, state, step, h):
    """the reference's loop body with torch ops, one parameter at a time"""
    from xmh.optim import SCHEDULES
    lr = h["lr"] * SCHEDULES[h["schedule"]](step / h["t_total"], h["warmup"])
    for p, (m, v) in zip(params, state):
        g = p.grad
        if h["max_grad_norm"] > 0:
            torch.nn.utils.clip_grad_norm_(p, h["max_grad_norm"])
        m.mul_(h["b1"]).add_(g, alpha=1 - h["b1"])
        v.mul_(h["b2"]).addcmul_(g, g, value=1 - h["b2"])
        update = m / (v.sqrt() + h["e"])
        if h["weight_decay"] > 0.0:
            update += h["weight_decay"] * p.data
        p.data.add_(-(lr * update))


def timed(step_fn, restore, steps, warmup):
    ev, wall = [], 0.0
    for i in range(warmup + steps):
        restore()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if i == warmup:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        a.record()
        step_fn(i)
        b.record()
        if i >= warmup:
            ev.append((a, b))
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / steps
    ms = [a.elapsed_time(b) for a, b in ev]
    return statistics.median(ms), min(ms), wall * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bits", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import xmh.models  # noqa: F401
    from xmh.models.dcmht import DCMHT
    from xmh.optim import BertAdam
    from xmh.utils.config import Config
    model = DCMHT.from_config(Config({"clip_path": "synthetic:1814"}), output_dim=a.bits)
    shapes = [tuple(p.shape) for p in model.parameters()]
    del model
    gen = torch.Generator(device="cuda").manual_seed(1814)
    mk = lambda s, scale: torch.randn(s, device="cuda", generator=gen) * scale      # noqa: E731
    g0 = [mk(s, 0.01) for s in shapes]
    sets = []
    for _ in range(2):
        params = [torch.nn.Parameter(mk(s, 0.05)) for s in shapes]
        for p, g in zip(params, g0):
            p.grad = g.clone()
        sets.append(params)
    numel = sum(g.numel() for g in g0)
    clipped = sum(g.numel() for g in g0 if float(g.norm()) + 1e-6 > HYPER["max_grad_norm"])
    nbytes = 32 * numel + 4 * clipped

    def restore_for(params):
        def restore():
            torch._foreach_copy_([p.grad for p in params], g0)
        return restore

    opt = BertAdam(sets[0], **HYPER)
    fused = timed(lambda i: opt.step(), restore_for(sets[0]), a.steps, a.warmup)
    state = [(torch.zeros_like(p), torch.zeros_like(p)) for p in sets[1]]
    with torch.no_grad():
        ref = timed(lambda i: reference_step(sets[1], state, i, HYPER), restore_for(sets[1]), a.steps, a.warmup)
    lines = [
        "BertAdam step, %d tensors, %.1f M parameters (ViT-B/32 + DCMHT heads, %d bits), %.1f %% of them in clipped tensors"
        % (len(shapes), numel / 1e6, a.bits, 100.0 * clipped / numel),
        "device %s, torch %s, %d timed steps after %d warm-up steps, device-event time per step()"
        % (torch.cuda.get_device_name(0), torch.__version__, a.steps, a.warmup),
        "bytes moved per step (32 B per parameter + 4 B where clipped): %.3f GB" % (nbytes / 1e9),
        "fused HIP step (2 launches):   median %8.3f ms  min %8.3f ms  wall %8.3f ms   %.2f TB/s at the median = %.1f %% of 8 TB/s"
        % (fused + (nbytes / fused[0] / 1e9, 100.0 * nbytes / (fused[0] * 1e-3) / PEAK)),
        "torch ops per parameter:       median %8.3f ms  min %8.3f ms  wall %8.3f ms" % ref,
        "ratio torch / fused: %.1fx (event median), %.1fx (wall)" % (ref[0] / fused[0], ref[2] / fused[2]),
    ]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
