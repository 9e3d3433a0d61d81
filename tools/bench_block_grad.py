#!/usr/bin/env python3
"""Forward + backward of a 12-layer CLIP block stack through Transformer.run_train (xmh_clip_blocks_forward_saved +
xmh_clip_blocks_backward, exact fp32) at the two tower shapes -- B 128 x L 50 x D 768 (ViT-B/32) and B 128 x L 32 x D 512 (text) --
timed by stream events, and beside it, in the same process, the same stack built from torch modules under autograd.
python tools/bench_block_grad.py [--layers 12] [--batch 128] [--iters 5] -> profiles/block_grad_bench.txt

FLOP accounting per layer (M = B L tokens): the four linear layers are 12 D^2 multiply-adds per token, forward 2 M 12 D^2 FLOP,
backward twice that (dX and dW); attention adds 4 M L D forward and 10 M L D backward (S, dP, dV, dQ, dK against S, PV).  Rates are
printed against the 157 TFLOP/s fp32 peak of the chip; an untuned fp32-MFMA GEMM reaches about 122 TFLOP/s there.  The rates are
per pass (forward, backward as the difference), not per kernel: a per-kernel table needs a rocprofv3 kernel trace of this script."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "clip-based-cross-modal-hash_amd"))

PEAK = 157e12


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e-3


class TorchBlock(torch.nn.Module):
    def __init__(self, D, heads):
        super().__init__()
        self.attn = torch.nn.MultiheadAttention(D, heads, batch_first=True)
        self.ln_1, self.ln_2 = torch.nn.LayerNorm(D), torch.nn.LayerNorm(D)
        self.c_fc, self.c_proj = torch.nn.Linear(D, 4 * D), torch.nn.Linear(4 * D, D)

    def forward(self, x, mask):
        h = self.ln_1(x)
        x = x + self.attn(h, h, h, need_weights=False, attn_mask=mask)[0]
        f = self.c_fc(self.ln_2(x))
        return x + self.c_proj(f * torch.sigmoid(1.702 * f))


def bench_shape(B, L, D, layers, causal, iters, out):
    from xmh.models.clip import Transformer
    heads = D // 64
    M = B * L
    gemm_fwd = 2.0 * M * 12 * D * D * layers
    attn_fwd, attn_bwd = 4.0 * M * L * D * layers, 10.0 * M * L * D * layers
    total = 3 * gemm_fwd + attn_fwd + attn_bwd
    torch.manual_seed(0)
    tr = Transformer(D, layers, heads).cuda()
    x = torch.randn(B, L, D, device="cuda", requires_grad=True)
    up = torch.randn(B, L, D, device="cuda")

    def ours():
        for p in tr.parameters():
            p.grad = None
        x.grad = None
        (tr.run_train(x, causal=causal) * up).sum().backward()

    def ours_fwd():
        with torch.no_grad():
            tr.run_train(x, causal=causal)

    blocks = torch.nn.ModuleList([TorchBlock(D, heads) for _ in range(layers)]).cuda()
    mask = torch.full((L, L), float("-inf"), device="cuda").triu_(1) if causal else None

    def theirs():
        for p in blocks.parameters():
            p.grad = None
        x.grad = None
        y = x
        for blk in blocks:
            y = blk(y, mask)
        (y * up).sum().backward()

    t_ours, t_fwd, t_torch = timed(ours, iters), timed(ours_fwd, iters), timed(theirs, iters)
    lines = ["B %d x L %d x D %d, %d layers%s: %.1f GFLOP forward + backward" % (B, L, D, layers, " (causal)" if causal else "", total / 1e9),
             "  run_train forward + backward   %8.2f ms  %6.1f TFLOP/s  %.2f of the fp32 peak" % (t_ours * 1e3, total / t_ours / 1e12, total / t_ours / PEAK),
             "  run_train forward (no_grad)    %8.2f ms  %6.1f TFLOP/s" % (t_fwd * 1e3, (gemm_fwd + attn_fwd) / t_fwd / 1e12),
             "  backward (difference)          %8.2f ms  %6.1f TFLOP/s  %.2f of the fp32 peak" % (
                 (t_ours - t_fwd) * 1e3, (2 * gemm_fwd + attn_bwd) / (t_ours - t_fwd) / 1e12, (2 * gemm_fwd + attn_bwd) / (t_ours - t_fwd) / PEAK),
             "  torch modules under autograd   %8.2f ms  %6.1f TFLOP/s  (ratio torch / run_train %.2f)" % (t_torch * 1e3, total / t_torch / 1e12, t_torch / t_ours)]
    for s in lines:
        print(s)
        out.append(s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--iters", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    out = ["tools/bench_block_grad.py on %s" % torch.cuda.get_device_name(0)]
    bench_shape(a.batch, 50, 768, a.layers, False, a.iters, out)
    bench_shape(a.batch, 32, 512, a.layers, True, a.iters, out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "block_grad_bench.txt"), "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
