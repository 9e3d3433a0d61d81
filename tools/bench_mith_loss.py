#!/usr/bin/env python3
"""MITH's training objective: forward + backward microseconds of xmh_mith_loss.hip (MITH.object_function + loss.backward()) against
the reference's expression (models/MITH/MITH.py:116-232, restated below op for op in fp32 torch, its four buffer writes included) on
the same GPU.  N 10 000 (COCO's train_num), B 100, D 512, K 16 / 64 / 128, default weights.

    python tools/bench_mith_loss.py [--iters 100] [--warmup 10]      -> one JSON line per shape"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "clip-based-cross-modal-hash_amd"))

INPUTS = ["res_img_cls", "res_txt_cls", "img_cls_hash", "txt_cls_hash", "tokens_hash_i", "tokens_hash_t", "trans_tokens_i",
          "trans_tokens_t"]


def torch_mith(buf, idx, S, rc_i, rc_t, c_i, c_t, t_i, t_t, T_i, T_t, w=(1.0, 1.0, 50.0, 10.0, 8.0, 0.01, 0.99), tau=0.07):
    """the reference expression, op for op (one buffer under its four names, as on the GPU)"""
    intra, distill, info_nce, inter, quan, alpha, lam = w
    buf[idx] = c_i.detach()
    buf[idx] = c_t.detach()
    buf[idx] = t_i.detach()
    buf[idx] = t_t.detach()
    Bs = torch.sign((c_i.detach() * lam + t_i.detach() * (1 - lam)) + (c_t.detach() * lam + t_t.detach() * (1 - lam)))

    def bayes(a, b):
        s = 0.5 * torch.matmul(a, b.t()).clamp(min=-64, max=64)
        return -torch.mean(S * s - torch.log(1 + torch.exp(s)))

    def nce(a, b):
        scores = a.mm(b.t())
        scores /= tau
        tg = torch.arange(a.size(0), device=a.device)
        return 0.5 * (F.cross_entropy(scores, tg) + F.cross_entropy(scores.transpose(0, 1), tg))

    def nce_bmm(a, b):
        a, b = a.permute(1, 0, 2), b.permute(1, 0, 2)
        sim = torch.bmm(a, b.permute(0, 2, 1))
        sim /= tau
        n, m = sim.shape[0], sim.shape[1]
        tg = torch.arange(m, device=a.device).repeat(n)
        return 0.5 * (F.cross_entropy(sim.reshape(n * m, m), tg) + F.cross_entropy(sim.transpose(1, 2).reshape(n * m, m), tg))

    B, K = c_i.shape
    loss = intra * (bayes(buf, t_i) + bayes(buf, t_t)) + inter * (bayes(buf, c_t) + bayes(buf, c_i))
    loss = loss + quan * (F.mse_loss(c_i * 0.5 + t_i * 0.5, Bs, reduction="sum") / B / K + F.mse_loss(c_t * 0.5 + t_t * 0.5, Bs, reduction="sum") / B / K)
    loss = loss + info_nce * (nce(rc_i, rc_t) + alpha * nce_bmm(T_i, T_t))
    item_1 = F.mse_loss(c_i.detach(), t_i, reduction="sum") + F.mse_loss(c_t.detach(), t_t, reduction="sum")
    item_2 = 0.1 * (F.mse_loss(c_i, t_i.detach(), reduction="sum") + F.mse_loss(c_t, t_t.detach(), reduction="sum"))
    return loss + distill * (item_1 + item_2) / B


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
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    from xmh.models.mith import MITH
    N, B, D = 10000, 100, 512
    for K in (16, 64, 128):
        g = torch.Generator().manual_seed(1814 + K)
        xs = [F.normalize(torch.randn(B, D, generator=g), dim=-1) for _ in range(2)] \
            + [torch.tanh(torch.randn(B, K, generator=g) * 1.5) for _ in range(4)] \
            + [F.normalize(torch.randn(K, B, D, generator=g), dim=-1) for _ in range(2)]
        xs = [x.cuda().requires_grad_(True) for x in xs]
        S = (torch.rand(N, B, generator=g) < 0.1).float().cuda()
        idx = torch.randperm(N, generator=g)[:B].cuda()
        m = MITH.__new__(MITH)                              # the objective reads the weights and the buffer only
        torch.nn.Module.__init__(m)
        for k, v in MITH.HYPER:
            setattr(m, k, v)
        m._bind_buffer(torch.randn(N, K, generator=g).cuda())
        ref_buf = m.img_buffer_cls.clone()

        def ours():
            loss, _ = m.object_function(**dict(zip(INPUTS, xs)), indexs=idx, label_sim=S)
            loss.backward()

        def ref():
            torch_mith(ref_buf, idx, S, *xs).backward()

        with torch.no_grad():
            got = float(m.object_function(**dict(zip(INPUTS, xs)), indexs=idx, label_sim=S)[0])
            want = float(torch_mith(ref_buf, idx, S, *xs))
        (o50, o10), (r50, r10) = time_us(ours, args.iters, args.warmup), time_us(ref, args.iters, args.warmup)
        print(json.dumps({"N": N, "B": B, "K": K, "D": D, "hip_fwd_bwd_us_p50": round(o50, 1), "hip_fwd_bwd_us_p10": round(o10, 1),
                          "torch_ref_fwd_bwd_us_p50": round(r50, 1), "torch_ref_fwd_bwd_us_p10": round(r10, 1),
                          "loss": got, "loss_abs_diff": abs(got - want)}), flush=True)


if __name__ == "__main__":
    main()
