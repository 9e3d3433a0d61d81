#!/usr/bin/env python3
"""Forward + backward of MITH's hash head in training mode, both modalities, through MITHHashLayer.encode_img_train /
encode_txt_train (xmh_mith_train_forward + xmh_mith_train_backward, exact fp32) at the workload's shape -- B 128, D 512, K 64,
L 49 image tokens and 32 text tokens with a padding mask, 2 residual MLPs + 2 transformer blocks -- timed by stream events, and
beside it, in the same process, the same head built from torch modules under autograd (fp32, the K one-row hash layers as one
batched product, so the comparison is not slowed by a Python loop over K).
python tools/bench_mith_head.py [--batch 128] [--bits 64] [--iters 10] -> profiles/mith_head_bench.txt
--side ours runs this package's head alone and writes no file: the loop to put under a rocprofv3 kernel trace.

The objective is sum_i (output_i . up_i).sum() over the four outputs of each modality, so every gradient path runs.  Times are per
pass (forward + backward, forward under no_grad, backward as the difference), not per kernel: a per-kernel table needs a
rocprofv3 kernel trace of this script."""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "clip-based-cross-modal-hash_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_block_grad import TorchBlock, timed  # noqa: E402


class TorchHead(torch.nn.Module):
    """one modality of models/MITH/hash/hash.py:193-247 from torch modules (the gcl is handed in: both modalities share it)"""

    def __init__(self, gcl, D, K, layers, top_k):
        super().__init__()
        self.gcl, self.K, self.top_k = gcl, K, top_k
        self.blocks = torch.nn.ModuleList([TorchBlock(D, D // 64) for _ in range(layers)])
        self.hash_w, self.hash_b = torch.nn.Parameter(torch.randn(K, D) * 0.04), torch.nn.Parameter(torch.zeros(K))
        self.proj = torch.nn.Linear(D, D)
        self.register_buffer("pe", torch.randn(K, D) / D ** 0.5)

    def forward(self, cls, tokens, mask):                      # cls [B, D], tokens [B, L, D], mask [B, L] bool or None
        y, cls_hash = self.gcl(cls)
        sim = self.gcl(tokens)[1].detach()                     # [B, L, K]
        if mask is not None:
            sim = sim.masked_fill(mask[:, :, None], float("-inf"))
        sim = torch.where(sim > 0, sim, torch.full_like(sim, float("-inf")))
        kth = torch.topk(sim, self.top_k, dim=-1).values.min(-1, keepdim=True).values
        sim = torch.where(sim >= kth, sim, torch.full_like(sim, float("-inf")))
        att = torch.nan_to_num(torch.softmax(sim, dim=1), nan=0.0)
        z = torch.bmm(att.transpose(1, 2), tokens) + self.pe   # [B, K, D]
        for blk in self.blocks:
            z = blk(z, None)
        tokens_hash = torch.tanh((z * self.hash_w).sum(-1) + self.hash_b)
        return F.normalize(y, dim=-1), cls_hash, tokens_hash, F.normalize(self.proj(z), dim=-1).transpose(0, 1)


class TorchGcl(torch.nn.Module):
    def __init__(self, D, K, R):
        super().__init__()
        self.lns = torch.nn.ModuleList([torch.nn.LayerNorm(D) for _ in range(R)])
        self.mlps = torch.nn.ModuleList([torch.nn.Sequential(torch.nn.Linear(D, 4 * D), torch.nn.GELU(), torch.nn.Linear(4 * D, D)) for _ in range(R)])
        self.concept = torch.nn.Linear(D, K, bias=False)

    def forward(self, x):
        for ln, mlp in zip(self.lns, self.mlps):
            x = x + mlp(ln(x))
        return x, torch.tanh(self.concept(x))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--bits", type=int, default=64)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--side", choices=("both", "ours"), default="both")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from xmh.models.mith import MITHHashLayer
    B, D, K, R, layers, top_k, Li, Lt = a.batch, 512, a.bits, 2, 2, 8, 49, 32
    torch.manual_seed(0)
    head = MITHHashLayer(D, K, 0.0, layers, "gelu", top_k, R).cuda()
    cls_i, cls_t = (torch.randn(B, D, device="cuda", requires_grad=True) for _ in range(2))
    tok_i, tok_t = torch.randn(Li, B, D, device="cuda", requires_grad=True), torch.randn(Lt, B, D, device="cuda", requires_grad=True)
    mask = torch.arange(Lt, device="cuda")[None, :] >= (4 + (7 * torch.arange(B, device="cuda")) % 27)[:, None]
    ups = [torch.randn(s, device="cuda") for s in ((B, D), (B, K), (B, K), (K, B, D))]
    leaves = (cls_i, cls_t, tok_i, tok_t)

    def objective(outs):
        return sum((o * u).sum() for o, u in zip(outs, ups))

    def clear(module):
        for p in module.parameters():
            p.grad = None
        for x in leaves:
            x.grad = None

    def ours():
        clear(head)
        (objective(head.encode_img_train(cls_i, tok_i)) + objective(head.encode_txt_train(cls_t, tok_t, mask))).backward()

    def ours_fwd():
        with torch.no_grad():
            head.encode_img_train(cls_i, tok_i)
            head.encode_txt_train(cls_t, tok_t, mask)

    if a.side == "ours":
        print("encode_*_train forward + backward %.3f ms over %d iterations" % (timed(ours, a.iters) * 1e3, a.iters))
        return
    gcl = TorchGcl(D, K, R)
    torch_heads = torch.nn.ModuleList([TorchHead(gcl, D, K, layers, top_k), TorchHead(gcl, D, K, layers, top_k)]).cuda()

    def theirs():
        clear(torch_heads)
        (objective(torch_heads[0](cls_i, tok_i.transpose(0, 1), None)) + objective(torch_heads[1](cls_t, tok_t.transpose(0, 1), mask))).backward()

    def theirs_fwd():
        with torch.no_grad():
            torch_heads[0](cls_i, tok_i.transpose(0, 1), None)
            torch_heads[1](cls_t, tok_t.transpose(0, 1), mask)

    for fn in (ours, theirs):                                   # warm both sides before either is timed
        fn()
    t_ours, t_fwd, t_torch, t_torch_fwd = timed(ours, a.iters), timed(ours_fwd, a.iters), timed(theirs, a.iters), timed(theirs_fwd, a.iters)
    out = ["tools/bench_mith_head.py on %s" % torch.cuda.get_device_name(0),
           "B %d, D %d, K %d, L %d image + %d text, %d residual MLPs, %d blocks, both modalities, %d iterations" % (B, D, K, Li, Lt, R, layers, a.iters),
           "  encode_*_train forward + backward   %8.3f ms" % (t_ours * 1e3),
           "  encode_*_train forward (no_grad)    %8.3f ms" % (t_fwd * 1e3),
           "  backward (difference)               %8.3f ms" % ((t_ours - t_fwd) * 1e3),
           "  torch modules forward + backward    %8.3f ms  (ratio torch / ours %.2f)" % (t_torch * 1e3, t_torch / t_ours),
           "  torch modules forward (no_grad)     %8.3f ms  (ratio torch / ours %.2f)" % (t_torch_fwd * 1e3, t_torch_fwd / t_fwd)]
    print("\n".join(out))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "mith_head_bench.txt"), "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
