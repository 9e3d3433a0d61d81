#!/usr/bin/env python3
"""Time UMoED's soft-MoE decoder head (xmh_head_umoed) at the configuration's shape, both modalities: B = 100, T = 50
(image) / 32 (text), d = 512, M = 64, 8 heads, 6 layers, 8 x 8 slots, F = 2048, V = 2.  Stream events around one call, median of 30 after
5 warm-up calls, with the spread.  In the same run the same head written from torch modules (nn.MultiheadAttention, nn.LayerNorm,
nn.Linear, einsum for the Soft-MoE; fp32, eval mode, no_grad) over the same parameters, and the largest difference of the two logits.

    python tools/bench_umoed_head.py [--out profiles/umoed_head_bench.txt] [--reps 30] [--once]

--once: one call of the library's head per modality and nothing else (for a kernel trace)."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "clip-based-cross-modal-hash_amd"))


def torch_head(th, tokens):
    """the reference's forward of TokenHash with MoE, from the torch modules that hold the parameters -> embeds [B, M, V]"""
    x = th.decoder_learned_parameters.unsqueeze(0).repeat(tokens.shape[0], 1, 1)
    for y in th.decoder.layers:
        x = y.norm1(x + y.self_attn(x, x, x, need_weights=False)[0])
        x = y.norm2(x + y.multihead_attn(x, tokens, tokens, need_weights=False)[0])
        h = F.relu(y.linear(x))
        logits = torch.einsum("bmf,fnp->bmnp", h, y.moe.phi)
        dispatch = logits.softmax(dim=1)
        combine = logits.flatten(start_dim=2).softmax(dim=-1).reshape(logits.shape)
        xs = torch.einsum("bmf,bmnp->bnpf", h, dispatch)
        ys = torch.einsum("bnpf,nfd->bnpd", xs, y.moe.experts.weight) + y.moe.experts.bias[None, :, None, :]
        x = y.norm3(x + torch.einsum("bnpd,bmnp->bmd", ys, combine))
    return th.classifier(x)


def timed(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "umoed_head_bench.txt"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    from xmh.models.umoed import UMoEDTokenHash
    torch.backends.cuda.matmul.allow_tf32 = False
    th = UMoEDTokenHash(outputDim=2, embedDim=512, setDim=64, decoder_heads=8, decoder_layers=6, hash_func="linear_subspace",
                        merge_func="concatenate", num_experts=8, slots_per_expert=8, MoE=True, hidden_dim=512, seed=1814)
    with torch.no_grad():                                        # every layer its own values: deepcopy's equal layers are a special case
        g = torch.Generator().manual_seed(7)
        for p in th.parameters():
            p.add_(torch.randn(p.shape, generator=g) * p.std() * 0.1)
    th = th.cuda().eval().requires_grad_(False)
    g = torch.Generator().manual_seed(11)
    tokens = {"image": torch.randn(a.batch, 50, 512, generator=g).cuda(), "text": torch.randn(a.batch, 32, 512, generator=g).cuda()}
    lines = ["UMoED head, B = %d, d = 512, M = 64, 8 heads, 6 layers, 8 x 8 slots, F = 2048, V = 2; ms per call, median of %d (min .. max); %s"
             % (a.batch, a.reps, torch.cuda.get_device_name(0))]
    with torch.no_grad():
        for name, x in tokens.items():
            if a.once:
                th(x)
                torch.cuda.synchronize()
                continue
            mine, ref = th(x)[0], torch_head(th, x)
            diff = float((mine - ref).abs().max() / ref.abs().max())
            t_x = timed(lambda: th(x), a.reps)
            t_t = timed(lambda: torch_head(th, x), a.reps)
            lines.append("%-5s T = %2d  xmh %.3f (%.3f .. %.3f)  torch modules %.3f (%.3f .. %.3f)  torch / xmh %.2f  max |xmh - torch| / max |torch| %.2e"
                         % (name, x.shape[1], *t_x, *t_t, t_t[0] / t_x[0], diff))
    if a.once:
        return
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
