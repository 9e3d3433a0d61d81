#!/usr/bin/env python3
"""One training step of the stage that makes TwDH's transforms (xmh/models/twdh_transform.py) -- the rows' packed labels
gathered, xmh_twdh_targets, the objective, its gradient, the fused BertAdam -- timed with stream events after a warm-up, and beside
it, alternately in the same process, the same step written with torch ops under autograd (the targets from a label-by-centre product,
hash_convert as a one-hot, x.mm(M), softmax, nn.BCELoss, the L1 norm) plus BertAdam's per-parameter arithmetic in torch ops, which is
how the reference would run it on the device.
python tools/bench_twdh_transform.py [--batch 200] [--classes 80] [--shapes 512x16 2048x64] [--iters 1000] [--rounds 5] [--count-kernels] [--out FILE]

Both sides get the tie vectors from the device (the host draw and its copy are left out on both).  The table gives the median and the
spread of the rounds, and the device kernels per step counted by torch.profiler over 20 steps (with --count-kernels; n/a
without it or where the profiler is not available).  There is no pass mark: at B = 200 the step is launch-bound on both sides."""
import argparse
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "clip-based-cross-modal-hash_amd"))

HYPER = dict(b1=0.9, b2=0.98, e=1e-6, weight_decay=0.2, max_grad_norm=1.0)


def torch_step(M, state, lab_f, cen_f, tie_f, L, S, alpha, lr, bce):
    s = lab_f @ cen_f
    t = torch.where(s == 0, tie_f.expand_as(s), s.sign())
    bits = ((t > 0) & (lab_f.sum(1, keepdim=True) > 0)).long()
    x = torch.nn.functional.one_hot(bits, 2).float().reshape(bits.shape[0], -1)
    p = torch.softmax(x[:, :2 * L].mm(M).view(bits.shape[0], -1, 2), dim=-1)
    loss = 1 - torch.pow(p[:, :, 0] - p[:, :, 1], 2).mean() + bce(p.view(bits.shape[0], -1), x[:, 2 * L:]) + alpha * M.norm(p=1)
    M.grad = None
    loss.backward()
    with torch.no_grad():                                                   # models/common/optimizer.py:102-167 for one parameter
        torch.nn.utils.clip_grad_norm_(M, HYPER["max_grad_norm"])
        state["m"].mul_(HYPER["b1"]).add_(M.grad, alpha=1 - HYPER["b1"])
        state["v"].mul_(HYPER["b2"]).addcmul_(M.grad, M.grad, value=1 - HYPER["b2"])
        update = state["m"] / (state["v"].sqrt() + HYPER["e"]) + HYPER["weight_decay"] * M
        M.add_(-lr * update)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=200)
    ap.add_argument("--classes", type=int, default=80)
    ap.add_argument("--shapes", nargs="+", default=["512x16", "2048x64"])
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--count-kernels", action="store_true", help="count the device kernels per step with torch.profiler")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "twdh_transform_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_twdh_transform: no GPU; a time taken elsewhere says nothing")
    from xmh import retrieval as R
    from xmh.models import twdh_transform as X
    from xmh.optim import BertAdam
    B, C, N = a.batch, a.classes, 10000
    rng = np.random.default_rng(1814)
    labels = (rng.random((N, C)) < 0.03).astype(np.int64)
    labels[np.arange(N), rng.integers(0, C, N)] = 1
    lines = ["TwDH transform stage, one step (targets, objective, gradient, BertAdam), B = %d, C = %d; %d rounds of %d steps, stream events, "
             "median us per step (min .. max)" % (B, C, a.rounds, a.iters),
             "%-10s %-30s %-30s %-12s %s" % ("L x S", "xmh", "torch ops", "torch / xmh", "kernels per step xmh / torch")]
    for shape in a.shapes:
        L, S = (int(v) for v in shape.split("x"))
        cen = rng.integers(0, 2, (C, L + S)) * 2 - 1
        M0 = rng.uniform(-1, 1, (2 * L, 2 * S)).astype(np.float32)
        lab_all = torch.tensor(labels).cuda()
        packed = R.pack_labels((lab_all == 1).to(torch.uint8))
        cen_i8, cen_f, lab_f = torch.tensor(cen).to(torch.int8).cuda(), torch.tensor(cen).float().cuda(), lab_all.float()
        idx = [torch.tensor(rng.choice(N, B, replace=False)).cuda() for _ in range(8)]
        ties = [(torch.randint(0, 2, (L + S,), device="cuda") * 2 - 1).to(torch.int8) for _ in range(8)]
        ties_f = [t.float() for t in ties]
        Mx = torch.nn.Parameter(torch.tensor(M0).cuda())
        opt = BertAdam([Mx], lr=1e-3, warmup=0.1, schedule="warmup_cosine", b1=0.9, b2=0.98, e=1e-6, t_total=100 * math.ceil(N / B),
                       weight_decay=0.2, max_grad_norm=1.0)
        Mt = torch.nn.Parameter(torch.tensor(M0).cuda())
        state = {"m": torch.zeros_like(Mt), "v": torch.zeros_like(Mt)}
        bce = torch.nn.BCELoss()
        count = [0]

        def step_xmh():
            i = count[0] % 8
            count[0] += 1
            loss, _ = X.transform_loss(Mx, X.transform_targets(packed.index_select(0, idx[i]), C, cen_i8, ties[i]), L, S, 1e-3)
            opt.zero_grad()
            loss.backward()
            opt.step()

        def step_torch():
            i = count[0] % 8
            count[0] += 1
            torch_step(Mt, state, lab_f.index_select(0, idx[i]), cen_f, ties_f[i], L, S, 1e-3, 1e-4, bce)

        def timed(fn):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(a.iters):
                fn()
            stop.record()
            stop.synchronize()
            return start.elapsed_time(stop) * 1e3 / a.iters

        def kernels(fn):
            if not a.count_kernels:
                return "n/a"
            try:
                from torch.profiler import ProfilerActivity, profile
                with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                    for _ in range(20):
                        fn()
                    torch.cuda.synchronize()
                n = sum(e.count for e in prof.key_averages() if getattr(e, "device_type", None) is not None and "cuda" in str(e.device_type).lower())
                return "%.1f" % (n / 20) if n else "n/a"
            except Exception:                                               # the profiler is optional equipment
                return "n/a"

        timed(step_xmh), timed(step_torch)                                  # warm-up of both sides
        tx, tt = [], []
        for _ in range(a.rounds):
            tx.append(timed(step_xmh))
            tt.append(timed(step_torch))
        fmt = lambda t: "%.1f (%.1f .. %.1f)" % (statistics.median(t), min(t), max(t))      # noqa: E731
        lines.append("%-10s %-30s %-30s %-12.2f %s / %s" % ("%d x %d" % (L, S), fmt(tx), fmt(tt), statistics.median(tt) / statistics.median(tx),
                                                         kernels(step_xmh), kernels(step_torch)))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
