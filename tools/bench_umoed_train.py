#!/usr/bin/env python3
"""Time one training step of UMoED's decoder head (xmh_head_umoed_train_forward + xmh_head_umoed_backward behind
UMoEDTokenHash.forward_train) at the configuration's shape, both modalities: B = 100, T = 50 (image) / 32 (text), d = 512,
M = 64, 8 heads, 6 layers, 8 x 8 slots, F = 2048, V = 2, dropout 0.3.  A step is the keep-mask draw, the forward, and the backward of
sum(embeds * G) to the tokens and every parameter.  Stream events around one step, median of 30 after 5 warm-up steps, with the spread.
In the same run the same head from torch modules under torch's autograd in train mode (tools/bench_umoed_head.py's torch-module head
with the reference's six dropout sites per layer; fp32) over the same parameters, and -- without dropout, where the two compute the
same function -- the largest difference of the logits and of the token gradients.

    python tools/bench_umoed_train.py [--out profiles/umoed_train_bench.txt] [--reps 30] [--once]

--once: one step of the library's head per modality and nothing else (for a kernel trace)."""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "clip-based-cross-modal-hash_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_umoed_head import timed  # noqa: E402


def torch_head_train(th, tokens):
    """bench_umoed_head.torch_head with SoftMoEDecoderLayer's dropouts: the modules' own (inside both nn.MultiheadAttention, and
    y.dropout at four places); they act when the modules are in train mode -> embeds [B, M, V]"""
    x = th.decoder_learned_parameters.unsqueeze(0).repeat(tokens.shape[0], 1, 1)
    for y in th.decoder.layers:
        x = y.norm1(x + y.dropout(y.self_attn(x, x, x, need_weights=False)[0]))
        x = y.norm2(x + y.dropout(y.multihead_attn(x, tokens, tokens, need_weights=False)[0]))
        h = y.dropout(F.relu(y.linear(x)))
        logits = torch.einsum("bmf,fnp->bmnp", h, y.moe.phi)
        dispatch = logits.softmax(dim=1)
        combine = logits.flatten(start_dim=2).softmax(dim=-1).reshape(logits.shape)
        xs = torch.einsum("bmf,bmnp->bnpf", h, dispatch)
        ys = torch.einsum("bnpf,nfd->bnpd", xs, y.moe.experts.weight) + y.moe.experts.bias[None, :, None, :]
        x = y.norm3(x + y.dropout(torch.einsum("bnpd,bmnp->bmd", ys, combine)))
    return th.classifier(x)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "umoed_train_bench.txt"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    from xmh.models.umoed import UMoEDTokenHash
    torch.backends.cuda.matmul.allow_tf32 = False
    th = UMoEDTokenHash(outputDim=2, embedDim=512, setDim=64, dropout=0.3, decoder_heads=8, decoder_layers=6, hash_func="linear_subspace",
                        merge_func="concatenate", num_experts=8, slots_per_expert=8, MoE=True, hidden_dim=512, seed=1814)
    with torch.no_grad():                                        # every layer its own values: deepcopy's equal layers are a special case
        g = torch.Generator().manual_seed(7)
        for p in th.parameters():
            p.add_(torch.randn(p.shape, generator=g) * p.std() * 0.1)
    th = th.cuda().train()
    th.generator = torch.Generator(device="cuda").manual_seed(3)
    g = torch.Generator().manual_seed(11)
    tokens = {"image": torch.randn(a.batch, 50, 512, generator=g).cuda(), "text": torch.randn(a.batch, 32, 512, generator=g).cuda()}
    up = torch.randn(a.batch, 64, 2, generator=g).cuda()

    def step(forward, x, **kw):
        th.zero_grad(set_to_none=True)
        x.grad = None
        embeds = forward(x, **kw)
        (embeds * up).sum().backward()
        return embeds

    xmh = lambda x, **kw: th.forward_train(x, **kw)[0]           # noqa: E731
    ref = lambda x: torch_head_train(th, x)                      # noqa: E731
    lines = ["UMoED head, one training step (mask draw + forward + backward), B = %d, d = 512, M = 64, 8 heads, 6 layers, 8 x 8 slots, F = 2048, "
             "V = 2, p = 0.3; ms per step, median of %d (min .. max); %s" % (a.batch, a.reps, torch.cuda.get_device_name(0))]
    for name, x in tokens.items():
        x.requires_grad_(True)
        if a.once:
            step(xmh, x)
            torch.cuda.synchronize()
            continue
        th.eval()                                                # torch's modules drop nothing in eval mode; forward_train takes keep=None
        e_x = step(xmh, x, keep=None).detach()
        g_x = x.grad.clone()
        e_t = step(ref, x).detach()
        diff_e, diff_g = float((e_x - e_t).abs().max() / e_t.abs().max()), float((g_x - x.grad).abs().max() / x.grad.abs().max())
        th.train()
        t_x = timed(lambda: step(xmh, x), a.reps)
        t_f = timed(lambda: xmh(x), a.reps)                      # the draw and the forward alone (a record is kept: the parameters want gradients)
        t_t = timed(lambda: step(ref, x), a.reps)
        lines.append("%-5s T = %2d  xmh %.3f (%.3f .. %.3f), of which draw + forward %.3f  torch modules %.3f (%.3f .. %.3f)  torch / xmh %.2f  "
                     "without dropout: max |xmh - torch| / max |torch| embeds %.2e, token gradient %.2e"
                     % (name, x.shape[1], *t_x, t_f[0], *t_t, t_t[0] / t_x[0], diff_e, diff_g))
    if a.once:
        return
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
