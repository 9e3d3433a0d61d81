#!/usr/bin/env python3
"""Train-mode hash heads: forward + backward microseconds of xmh_head_grad.hip through the autograd Functions of
xmh/models/heads.py, against the reference's expression run by torch on the same GPU in the same process (restated below from
torch modules: nn.MultiheadAttention on a length-1 sequence, nn.BatchNorm1d / nn.LayerNorm, nn.Linear, relu, pair softmax;
nn.Linear, nn.Dropout, tanh -- models/DCMHT/hash/hash.py:15-46, models/DSPH/hash/hash.py:6-15).  Embeddings carry no graph (the
frozen-backbone case); every parameter of the head receives its gradient.  B 100 and 128, E 512, K 16 / 64 / 128, both heads.

    python tools/bench_head_grad.py [--iters 200] [--warmup 20]      -> one JSON line per head and shape"""
import argparse
import json
import os
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "clip-based-cross-modal-hash_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_hyp import time_us  # noqa: E402


class TorchDCMHT(nn.Module):
    def __init__(self, E, K, layernorm):
        super().__init__()
        self.atten = nn.MultiheadAttention(E, num_heads=8, batch_first=True)
        self.norm = nn.LayerNorm(E) if layernorm else nn.BatchNorm1d(E)
        self.fc2 = nn.Linear(E, 2 * K)

    def forward(self, x):
        x = x.view(x.shape[0], 1, x.shape[1])
        e = self.atten(x, x, x, need_weights=False)[0].squeeze()
        e = torch.relu(self.fc2(self.norm(e)))
        return torch.softmax(e.view(e.shape[0], -1, 2), dim=-1).view(e.shape[0], -1)


class TorchDSPH(nn.Module):
    def __init__(self, E, K):
        super().__init__()
        self.fc = nn.Linear(E, K)
        self.drop_out = nn.Dropout(p=0.2)

    def forward(self, x):
        return torch.tanh(self.drop_out(self.fc(x)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    from xmh.models.heads import DCMHTModalityHash, DSPHLinearHash
    g = torch.Generator().manual_seed(1814)
    E = 512
    for B in (100, 128):
        for K in (16, 64, 128):
            x = torch.randn(B, E, generator=g).cuda()
            heads = [("dcmht_img", DCMHTModalityHash(E, K, 8, layernorm=False), TorchDCMHT(E, K, False), 2 * K),
                     ("dcmht_txt", DCMHTModalityHash(E, K, 8, layernorm=True), TorchDCMHT(E, K, True), 2 * K),
                     ("dsph", DSPHLinearHash(E, K), TorchDSPH(E, K), K)]
            for name, ours, ref, n_out in heads:
                ref.load_state_dict(ours.state_dict())
                ours, ref = ours.cuda().train(), ref.cuda().train()
                up = torch.randn(B, n_out, generator=g).cuda()

                def run(mod):
                    def step():
                        mod.zero_grad(set_to_none=True)
                        (mod(x) * up).sum().backward()
                    return step

                diff = None
                if name != "dsph":                                     # dropout draws differ; the DCMHT heads are deterministic
                    with torch.no_grad():
                        diff = float((ours(x) - ref(x)).abs().max())
                (o50, o10), (r50, r10) = time_us(run(ours), args.iters, args.warmup), time_us(run(ref), args.iters, args.warmup)
                print(json.dumps({"head": name, "B": B, "E": E, "K": K, "hip_fwd_bwd_us_p50": round(o50, 1), "hip_fwd_bwd_us_p10": round(o10, 1),
                                  "torch_ref_fwd_bwd_us_p50": round(r50, 1), "torch_ref_fwd_bwd_us_p10": round(r10, 1),
                                  "probs_max_abs_diff": diff}), flush=True)


if __name__ == "__main__":
    main()
