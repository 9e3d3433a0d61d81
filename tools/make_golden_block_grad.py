#!/usr/bin/env python3
"""Golden gradients of the CLIP block stack, produced by the UNMODIFIED reference Transformer (models/CLIP/model.py) through
oracle._ref_import, on the CPU in fp32: python tools/make_golden_block_grad.py [DIR] -> tests/golden/block_grad.npz (or DIR/).
Needs the reference checkout; nothing at test time runs or imports this.

Cases, seeds, the thinning rule and the float64 restatement live in tests/block_grad_cases.py.  Per case <c>: `<c>__seed`,
`<c>__checksum` of the regenerated parameters / inputs / mask, the reference's fp32 `(y . up).sum().backward()` as `<c>__y`,
`<c>__g_x`, `<c>__g_l<i>_<param>` (thinned), and per tensor `<c>__eref_<tensor>` = max|fp32 - fp64| / max|fp64| on the whole tensor,
the fp64 side being the restatement (the reference's LayerNorm refuses double parameters).  The restatement's own fp32 run must
equal the reference's to the bit -- asserted here, so a test may regenerate the stored tensors without the reference.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import block_grad_cases as BC  # noqa: E402
from oracle import _ref_import  # noqa: E402
from oracle.fixtures import out_path  # noqa: E402

_ref_import.setup()
from models.CLIP.model import Transformer  # noqa: E402  (the reference class)


def run_reference(sd, x, up, heads, causal, kpm):
    """the reference's Transformer in fp32 on [L, B, D] -> the dict run_restatement returns"""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        B, L, D = x.shape
        layers = len({k.split(".")[1] for k in sd})
        mask = torch.full((L, L), float("-inf")).triu_(1) if causal else None
        m = Transformer(D, layers, heads, mask)
        m.load_state_dict({k: torch.tensor(v) for k, v in sd.items()}, strict=True)
        xt = torch.tensor(x).requires_grad_(True)
        y, _ = m(xt.transpose(0, 1), key_padding_mask=None if kpm is None else torch.tensor(kpm))
        y = y.transpose(0, 1)
        (y * torch.tensor(up)).sum().backward()
        out = {"y": y.detach().numpy().copy(), "g_x": xt.grad.numpy().copy()}
        for i in range(layers):
            for kind, key in BC.PARAMS:
                out["g_l%d_%s" % (i, kind)] = m.get_parameter("resblocks.%d.%s" % (i, key)).grad.numpy().copy()
        return out
    finally:
        torch.set_num_threads(threads)


def main():
    out, pool = {}, {}
    for name, (D, heads, layers, L, B, causal, kp) in BC.CASES.items():
        sd, x, up, kpm = BC.case_inputs(name)
        ref = run_reference(sd, x, up, heads, causal, kpm)
        r32 = BC.run_restatement(sd, x, up, heads, causal, kpm, torch.float32)
        r64 = BC.run_restatement(sd, x, up, heads, causal, kpm, torch.float64)
        assert sorted(ref) == sorted(r32) == sorted(r64)
        for k in ref:
            assert np.isfinite(ref[k]).all(), (name, k)
            assert np.array_equal(ref[k], r32[k]), (name, k, BC.rel_err(ref[k], r32[k]))      # to the bit
        per, pl = BC.erefs(ref, r64)
        out[name + "__seed"] = np.int64(BC.case_seed(name))
        out[name + "__checksum"] = np.float64(BC.inputs_checksum(sd, x, up, kpm))
        for k in ref:
            out["%s__%s" % (name, k)] = BC.thin(ref[k]).astype(np.float32)
            out["%s__eref_%s" % (name, k)] = np.float64(per[k])
        for k, e in pl.items():
            pool[k] = max(pool.get(k, 0.0), e)
        print("%-24s %s" % (name, " ".join("%s %.1e" % (k[2:] if k != "y" else k, pl[k]) for k in BC.KINDS)))
    print("pooled e_ref:", " ".join("%s %.2e" % (k, pool[k]) for k in BC.KINDS))
    path = out_path("block_grad.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
