#!/usr/bin/env python3
"""DSPH's HyP loss: forward + backward microseconds of xmh_hyp.hip (HyPProxies.forward + loss.backward()) against the reference's
expression (models/DSPH/loss/HyP.py:18-70, restated below in fp32 torch ops with its nonzero() counts, which synchronise with the
host) on the same GPU.  B 100, C 80, K 16 and 128 (the COCO default and configs[4]), alpha 0.8.

    python tools/bench_hyp.py [--iters 200] [--warmup 20]      -> one JSON line per shape"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "clip-based-cross-modal-hash_amd"))


def torch_hyp(x, y, proxies, label, threshold, alpha):
    """the reference expression, op for op (its len(nonzero()) counts and boolean-mask gathers included)"""
    nP = F.normalize(proxies, p=2, dim=1)
    cos, cos_t = F.normalize(x, p=2, dim=1).mm(nP.T), F.normalize(y, p=2, dim=1).mm(nP.T)
    p_num, n_num = len(label.nonzero()), len((label == 0).nonzero())
    zeros = torch.zeros_like(cos)
    loss = (torch.where(label == 1, 1 - cos, zeros).sum() / p_num + torch.where(label == 0, F.relu(cos - threshold), zeros).sum() / n_num
            + torch.where(label == 1, 1 - cos_t, zeros).sum() / p_num + torch.where(label == 0, F.relu(cos_t - threshold), zeros).sum() / n_num)
    if alpha > 0:
        index = label.sum(dim=1) > 1
        lab_ = label[index].float()
        x_, t_ = x[index], y[index]
        pairs = lab_.mm(lab_.T) == 0
        if len(pairs.nonzero()) != 0:
            nx_, nt_ = F.normalize(x_, p=2, dim=1), F.normalize(t_, p=2, dim=1)
            for sim in (nx_.mm(nx_.T), nt_.mm(nt_.T), nx_.mm(nt_.T)):
                loss = loss + torch.where(pairs, alpha * F.relu(sim - threshold), torch.zeros_like(sim)).sum() / len(pairs.nonzero())
    return loss


def time_us(step, iters, warmup):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1000.0)
    times.sort()
    return times[len(times) // 2], times[len(times) // 10]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    from xmh.models.dsph import HyPProxies
    g = torch.Generator().manual_seed(1814)
    B, C, alpha = 100, 80, 0.8
    for K, threshold in ((16, 0.25), (128, 0.0)):
        x = torch.tanh(torch.randn(B, K, generator=g) * 1.5).cuda().requires_grad_(True)
        y = torch.tanh(torch.randn(B, K, generator=g) * 1.5).cuda().requires_grad_(True)
        label = (torch.rand(B, C, generator=g) < 0.05).float()
        label[torch.arange(B), torch.randint(0, C, (B,), generator=g)] = 1.0
        label = label.cuda()
        hyp = HyPProxies(numclass=C, output_dim=K, alpha=alpha, threshold=threshold).cuda()

        def ours():
            hyp(x, y, label).backward()

        def ref():
            torch_hyp(x, y, hyp.proxies, label, threshold, alpha).backward()

        with torch.no_grad():
            want = torch_hyp(x, y, hyp.proxies, label, threshold, alpha)
            got = hyp(x, y, label)
        (o50, o10), (r50, r10) = time_us(ours, args.iters, args.warmup), time_us(ref, args.iters, args.warmup)
        print(json.dumps({"B": B, "K": K, "C": C, "alpha": alpha, "hip_fwd_bwd_us_p50": round(o50, 1), "hip_fwd_bwd_us_p10": round(o10, 1),
                          "torch_ref_fwd_bwd_us_p50": round(r50, 1), "torch_ref_fwd_bwd_us_p10": round(r10, 1),
                          "loss_abs_diff": abs(float(got) - float(want))}))


if __name__ == "__main__":
    main()
