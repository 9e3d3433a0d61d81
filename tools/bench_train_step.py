#!/usr/bin/env python3
"""One full DCMHT training step on ViT-B/32 -- both towers forward and backward (CLIP.encode_image_train / encode_text_train: exact fp32,
xmh_tower_grad.hip + xmh_block_grad.hip), the two hash heads in train mode, the DCMHT objective and the fused BertAdam step -- timed by
stream events, and beside it, in the same process, the same model built from torch modules under autograd (the same loss kernels
and the same optimiser on its parameters, so the difference is the towers and the heads).
python tools/bench_train_step.py [--batch 128] [--layers 12] [--iters 5] [--rounds 3] -> profiles/train_step_bench.txt

The two sides are timed alternately, `rounds` times `iters` steps each after one warm-up step per side; the table gives the median
and the spread of the rounds.  There is no pass mark: the yardstick is torch autograd measured in the same run.  FLOP per step, from
the shapes: the linear layers of a block are 12 D^2 multiply-adds per token, forward 2 M 12 D^2, backward twice that; attention adds
4 M L D forward and 10 M L D backward; conv1 is 2 (B P) D (3 p p) forward and as much backward (no gradient to the image).  The rate is
the whole step's over the 157 TFLOP/s fp32 peak: an end-to-end figure, not a kernel's share of peak."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "clip-based-cross-modal-hash_amd"))

PEAK = 157e12


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


class TorchHead(torch.nn.Module):
    """one modality of the DCMHT head: attention over a length-1 sequence, BatchNorm (image) or LayerNorm (text), fc2 + relu, pair softmax"""

    def __init__(self, E, K, image):
        super().__init__()
        self.atten = torch.nn.MultiheadAttention(E, 8, batch_first=True)
        self.norm = torch.nn.BatchNorm1d(E) if image else torch.nn.LayerNorm(E)
        self.fc2 = torch.nn.Linear(E, 2 * K)

    def forward(self, x):
        x = x.unsqueeze(1)
        f = torch.relu(self.fc2(self.norm(self.atten(x, x, x, need_weights=False)[0].squeeze(1))))
        return torch.softmax(f.view(f.shape[0], -1, 2), -1).view(f.shape[0], -1)


class TorchClipDcmht(torch.nn.Module):
    def __init__(self, layers, K, res=224, patch=32, vw=768, tw=512, E=512, vocab=49408, context=77):
        super().__init__()
        self.conv1 = torch.nn.Conv2d(3, vw, patch, patch, bias=False)
        self.cls = torch.nn.Parameter(0.03 * torch.randn(vw))
        self.vpos = torch.nn.Parameter(0.03 * torch.randn((res // patch) ** 2 + 1, vw))
        self.ln_pre, self.ln_post = torch.nn.LayerNorm(vw), torch.nn.LayerNorm(vw)
        self.vblocks = torch.nn.ModuleList([TorchBlock(vw, vw // 64) for _ in range(layers)])
        self.vproj = torch.nn.Parameter(vw ** -0.5 * torch.randn(vw, E))
        self.tok = torch.nn.Embedding(vocab, tw)
        self.tpos = torch.nn.Parameter(0.01 * torch.randn(context, tw))
        self.tblocks = torch.nn.ModuleList([TorchBlock(tw, tw // 64) for _ in range(layers)])
        self.ln_final = torch.nn.LayerNorm(tw)
        self.tproj = torch.nn.Parameter(tw ** -0.5 * torch.randn(tw, E))
        self.img_hash, self.txt_hash = TorchHead(E, K, True), TorchHead(E, K, False)

    def backbone_parameters(self):
        heads = {id(p) for m in (self.img_hash, self.txt_hash) for p in m.parameters()}
        return [p for p in self.parameters() if id(p) not in heads]

    def forward(self, image, ids):
        x = self.conv1(image).flatten(2).transpose(1, 2)
        x = torch.cat([self.cls.expand(x.shape[0], 1, -1), x], 1) + self.vpos
        x = self.ln_pre(x)
        for blk in self.vblocks:
            x = blk(x, None)
        e_img = self.ln_post(x[:, 0]) @ self.vproj
        L = ids.shape[1]
        t = self.tok(ids) + self.tpos[:L]
        mask = torch.full((L, L), float("-inf"), device=ids.device).triu_(1)
        for blk in self.tblocks:
            t = blk(t, mask)
        e_txt = self.ln_final(t[torch.arange(ids.shape[0]), ids.argmax(-1)]) @ self.tproj
        return self.img_hash(e_img), self.txt_hash(e_txt)


def step_flop(B, layers, L_txt):
    total = 0.0
    for L, D in ((50, 768), (L_txt, 512)):
        M = B * L
        total += layers * (3 * 2.0 * M * 12 * D * D + 14.0 * M * L * D)
    return total + 2 * 2.0 * B * 49 * 768 * 3072


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--bits", type=int, default=16)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    import xmh.models  # noqa: F401
    from xmh.common.register import registry
    from xmh.models import weights as W
    from xmh.optim import BertAdam
    from xmh.utils.config import Config
    B, K, C = a.batch, a.bits, 24
    cfg = Config({"arch": "DCMHT", "clip_path": "synthetic:1814:vision_layers=%d,transformer_layers=%d" % (a.layers, a.layers)})
    model = registry.get_model_class("DCMHT").from_config(cfg, output_dim=K, train_num=B).float().cuda().train()
    torch.manual_seed(0)
    twin = TorchClipDcmht(a.layers, K).cuda().train()
    image, ids = W.synth_images(2, B).cuda(), W.synth_text(2, B)[0].cuda()
    g = torch.Generator().manual_seed(5)
    labels = (torch.rand(B, C, generator=g) < 0.1).float()
    labels[torch.arange(B), torch.arange(B) % C] = 1.0
    labels = labels.cuda()
    hyper = dict(lr=1e-3, warmup=0.1, t_total=10 ** 6, schedule="warmup_cosine", b1=0.9, b2=0.98, e=1e-6, weight_decay=0.2, max_grad_norm=1.0)
    opt = BertAdam([{"params": model.backbone.parameters(), "lr": 1e-5}, {"params": model.hash.parameters(), "lr": 1e-3}], **hyper)
    heads = list(twin.img_hash.parameters()) + list(twin.txt_hash.parameters())
    opt_t = BertAdam([{"params": twin.backbone_parameters(), "lr": 1e-5}, {"params": heads, "lr": 1e-3}], **hyper)

    def ours():
        loss, _ = model.object_function(*model.forward_train(image, ids), labels)
        opt.zero_grad()
        loss.backward()
        opt.step()

    def theirs():
        loss, _ = model.object_function(*twin(image, ids), labels)
        opt_t.zero_grad()
        loss.backward()
        opt_t.step()

    def timed(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(a.iters):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / a.iters * 1e-3

    for fn in (ours, theirs):                                  # warm-up: code objects, allocator pools, library heuristics
        fn()
    torch.cuda.synchronize()
    t_ours, t_torch = [], []
    for _ in range(a.rounds):                                  # alternate the two sides
        t_ours.append(timed(ours))
        t_torch.append(timed(theirs))
    flop = step_flop(B, a.layers, ids.shape[1])
    mo, mt = statistics.median(t_ours), statistics.median(t_torch)
    out = ["tools/bench_train_step.py on %s" % torch.cuda.get_device_name(0),
           "one DCMHT step, ViT-B/32, batch %d, %d + %d layers, %d text tokens, %d bits: %.1f GFLOP in the towers" % (
               B, a.layers, a.layers, ids.shape[1], K, flop / 1e9),
           "  %d rounds of %d steps per side, alternating; median (min .. max)" % (a.rounds, a.iters),
           "  forward_train + loss + backward + BertAdam   %8.2f ms (%.2f .. %.2f)  %6.1f TFLOP/s  %.2f of the fp32 peak, end to end" % (
               mo * 1e3, min(t_ours) * 1e3, max(t_ours) * 1e3, flop / mo / 1e12, flop / mo / PEAK),
           "  torch modules under autograd, same loss/opt  %8.2f ms (%.2f .. %.2f)  %6.1f TFLOP/s" % (
               mt * 1e3, min(t_torch) * 1e3, max(t_torch) * 1e3, flop / mt / 1e12),
           "  ratio torch / this package %.2f" % (mt / mo)]
    for s in out:
        print(s)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "train_step_bench.txt"), "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
