#!/usr/bin/env python3
"""The part of a DNPH training step this package adds -- embeddings -> DNPHHashLayer in train mode -> the objective with its noise
assignment -> backward() to the embeddings, the head's parameters and the proxies -- timed by a host clock around steps that end in a
device synchronise, and beside it, in the same process, the same step built from torch modules under autograd (nn.Linear / Dropout /
tanh, the reference's expression of the loss with torch.cdist and F.cross_entropy).  Both sides draw the same noise vectors and assign
them with the same host solver (xmh_assign_min_cost), so the difference is the head and objective kernels and their launches.  A second
pair of rows times the objective alone, forward and backward, with the noises already assigned (no host round trip).
python tools/bench_dnph_step.py [--batch 100] [--embed 512] [--classes 80] [--bits 16 64 128] [--iters 200] [--rounds 5] [--out FILE]

The two sides are timed alternately, `rounds` times `iters` steps each after a warm-up of `iters` steps per side; the table gives the
median and the spread of the rounds.  There is no pass mark: the yardstick is torch autograd measured in the same run.  The towers
and the optimisers are left out on both sides (tools/bench_train_step.py times a whole step of the towers)."""
import argparse
import os
import statistics
import sys
import time
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "clip-based-cross-modal-hash_amd"))


class TorchHead(torch.nn.Module):
    def __init__(self, E, K):
        super().__init__()
        self.fc, self.drop, self.pre = torch.nn.Linear(E, K), torch.nn.Dropout(0.2), torch.nn.Linear(E, 80)

    def forward(self, x):
        return torch.tanh(self.drop(self.fc(x))), self.pre(x)


def torch_loss(P, mrg, f1, f2, p1, p2, lab):
    """reference models/DNPH/loss/loss.py:12-33"""
    fa, la = F.normalize(torch.cat((f1, f2), 0), p=2, dim=-1), torch.cat((lab, lab), 0)
    D = torch.cdist(fa, F.normalize(P, p=2, dim=-1)) ** 2 + mrg * la
    p_loss = torch.sum(-la * F.log_softmax(-D, 1), -1).mean()
    t = torch.argmax(lab, -1)
    return p_loss + F.cross_entropy(p1, t) + F.cross_entropy(p2, t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--embed", type=int, default=512)
    ap.add_argument("--classes", type=int, default=80)
    ap.add_argument("--bits", type=int, nargs="+", default=[16, 64, 128])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dnph_step_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_dnph_step: no GPU; a time taken elsewhere says nothing")
    from xmh.models.dnph import DNPH, DNPHLoss, gene_noise
    from xmh.models.heads import DNPHHashLayer
    B, E, C = a.batch, a.embed, a.classes
    rng = np.random.default_rng(1814)
    labels = (rng.random((B, C)) < 0.04).astype(np.int64)
    labels[np.arange(B), rng.integers(0, C, B)] = 1
    lab_dev = torch.tensor(labels).cuda()
    lab_f = lab_dev.float()
    x = [torch.tensor(rng.standard_normal((B, E)).astype(np.float32)).cuda() for _ in range(2)]
    lines = ["DNPH head + objective, B = %d, E = %d, C = %d; %d rounds of %d steps, median ms per step (min .. max)" % (B, E, C, a.rounds, a.iters),
             "%-5s %-28s %-26s %-26s %s" % ("K", "what", "xmh", "torch modules", "torch / xmh")]
    for K in a.bits:
        head, loss_mod = DNPHHashLayer(E, K).cuda().train(), DNPHLoss(C, K).cuda()
        noise_rng = np.random.default_rng(7)
        me = types.SimpleNamespace(loss=loss_mod, noise_alpha=0.1, rand_unit_rect=lambda n, d: noise_rng.integers(0, 2, (n, d)) * 2 - 1)
        theads = [TorchHead(E, K).cuda().train() for _ in range(2)]
        tP = torch.nn.Parameter(loss_mod.proxies.detach().clone())
        xs = [t.clone().requires_grad_(True) for t in x]
        fixed = {}

        def step_xmh():
            fi, pi = head.encode_img(xs[0])
            ft, pt = head.encode_txt(xs[1])
            loss, _ = DNPH.compute_loss(me, fi, ft, pi, pt, lab_dev, None)
            loss.backward()

        def step_torch():
            (fi, pi), (ft, pt) = theads[0](xs[0]), theads[1](xs[1])
            s = me.rand_unit_rect(B, K)
            codes = torch.stack([fi.detach(), ft.detach()]).cpu().numpy()
            ni, nt = (torch.from_numpy(gene_noise(c, s)).float().cuda() for c in codes)
            loss = torch_loss(tP, 1.0, fi, ft, pi, pt, lab_f) - 0.1 * ((fi * ni).sum(-1).mean() + (ft * nt).sum(-1).mean())
            loss.backward()

        def objective_xmh():
            out = loss_mod.terms(fixed["f"][0], fixed["f"][1], fixed["p"][0], fixed["p"][1], lab_dev, None, fixed["n"][0], fixed["n"][1], 0.1)
            out[0].backward()

        def objective_torch():
            f, p, n = fixed["f"], fixed["p"], fixed["n"]
            loss = torch_loss(tP, 1.0, f[0], f[1], p[0], p[1], lab_f) - 0.1 * ((f[0] * n[0]).sum(-1).mean() + (f[1] * n[1]).sum(-1).mean())
            loss.backward()

        fixed["f"] = [torch.tanh(torch.randn(B, K, device="cuda")).requires_grad_(True) for _ in range(2)]
        fixed["p"] = [torch.randn(B, 80, device="cuda").requires_grad_(True) for _ in range(2)]
        fixed["n"] = [(torch.randint(0, 2, (B, K), device="cuda") * 2 - 1).float() for _ in range(2)]

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.iters):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / a.iters

        for what, fa, fb in (("head + objective + backward", step_xmh, step_torch), ("objective + backward", objective_xmh, objective_torch)):
            timed(fa), timed(fb)                                                    # warm-up of both sides
            ta, tb = [], []
            for _ in range(a.rounds):
                ta.append(timed(fa))
                tb.append(timed(fb))
            fmt = lambda t: "%.3f (%.3f .. %.3f)" % (statistics.median(t), min(t), max(t))      # noqa: E731
            lines.append("%-5d %-28s %-26s %-26s %.2f" % (K, what, fmt(ta), fmt(tb), statistics.median(tb) / statistics.median(ta)))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
