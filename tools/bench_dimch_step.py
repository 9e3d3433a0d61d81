#!/usr/bin/env python3
"""DIMCH's objective, forward and backward, timed by stream events: xmh_dimch_loss / xmh_dimch_loss_grad through
xmh.models.dimch.DIMCHObjective, and beside it, in the same run, the same expression from torch ops on the device under autograd
(tests/dimch_cases.py:objective_terms -- the reference's expression without its [N, N, N] tensor, which at the second shape would be
2 TB).  python tools/bench_dimch_step.py [--shapes 20,8,16 128,64,64] [--classes 80] [--runs 30] [--warmup 5] [--out FILE]

Per shape (B, M, K) and side: the median of `runs` forward times and of `runs` backward times after `warmup` untimed steps, and the
ratio torch / xmh.  There is no pass mark: the yardstick is torch autograd measured in the same run.  The constants are those of the
reference's configs/DIMCH/config.yaml (smooth_chamfer, tanh)."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "clip-based-cross-modal-hash_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(forward, runs, warmup):
    """-> (median forward ms, median backward ms) of `runs` steps; forward() returns the scalar to differentiate"""
    fw, bw = [], []
    for it in range(warmup + runs):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        loss = forward()
        ev[1].record()
        loss.backward()
        ev[2].record()
        torch.cuda.synchronize()
        if it >= warmup:
            fw.append(ev[0].elapsed_time(ev[1]))
            bw.append(ev[1].elapsed_time(ev[2]))
    return statistics.median(fw), statistics.median(bw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["20,8,16", "128,64,64"])
    ap.add_argument("--classes", type=int, default=80)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dimch_step_bench.txt"))
    a = ap.parse_args()
    if a.runs < 20:
        sys.exit("bench_dimch_step: at least 20 runs")
    if not torch.cuda.is_available():
        sys.exit("bench_dimch_step: no GPU; a time taken elsewhere says nothing")
    import dimch_cases as DC
    from xmh.models.dimch import DIMCHObjective
    cst = dict(DC.CONFIG)
    obj = DIMCHObjective(**cst)
    lines = ["DIMCH objective (smooth_chamfer, tanh, C = %d), median of %d runs by stream events, ms" % (a.classes, a.runs),
             "%-14s %-10s %-10s %-12s %-12s %-10s %s" % ("B, M, K", "xmh fwd", "xmh bwd", "torch fwd", "torch bwd", "fwd ratio", "bwd ratio")]
    for shape in a.shapes:
        B, M, K = (int(v) for v in shape.split(","))
        c = DC._draw(B, M, K, a.classes, seed=1814)
        leaves = [torch.tensor(c[k]).cuda().requires_grad_(True) for k in DC.INPUTS]
        lab = torch.tensor(c["labels"]).cuda()
        lab_f = lab.float()
        xf, xb = timed(lambda: obj.terms(leaves[0], leaves[2], leaves[1], leaves[3], lab)[0], a.runs, a.warmup)
        tf, tb = timed(lambda: DC.objective_terms(*leaves, lab_f, cst)[0], a.runs, a.warmup)
        lines.append("%-14s %-10.3f %-10.3f %-12.3f %-12.3f %-10.2f %.2f" % ("%d, %d, %d" % (B, M, K), xf, xb, tf, tb, tf / xf, tb / xb))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
