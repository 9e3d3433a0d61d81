#!/usr/bin/env python3
"""Golden gradients of the two CLIP towers, produced by the UNMODIFIED reference VisionTransformer and CLIP.encode_text
(models/CLIP/model.py) through oracle._ref_import, on the CPU in fp32: python tools/make_golden_tower_grad.py [DIR] ->
tests/golden/tower_grad.npz (or DIR/).  Needs the reference checkout; nothing at test time runs or imports this.

Cases, seeds, the thinning rule and the float64 restatement live in tests/tower_grad_cases.py.  Per case <c>: `<c>__seed`,
`<c>__checksum` of the regenerated parameters / inputs / mask, the reference's fp32 `(y . up).sum().backward()` as `<c>__y` and
`<c>__g_<tensor>` (thinned), and per tensor `<c>__eref_<tensor>` = max|fp32 - fp64| / max|fp64| on the whole tensor, the fp64 side
being the restatement.  The restatement's own fp32 run must equal the reference's to the bit -- asserted here, so a test may
regenerate the stored tensors without the reference.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tower_grad_cases as TC  # noqa: E402
from oracle import _ref_import  # noqa: E402
from oracle.fixtures import out_path  # noqa: E402

_ref_import.setup()
from models.CLIP.model import CLIP, VisionTransformer  # noqa: E402  (the reference classes)


def _collect(tower, m, y, layers, prefix):
    out = {"y": y.detach().numpy().copy()}
    for name in TC.tensor_names(tower, layers)[1:]:
        out[name] = m.get_parameter(TC.tensor_key(tower, name)[len(prefix):]).grad.numpy().copy()
    return out


def run_reference(tower, sd, x, up, kpm):
    """the reference's tower in fp32 -> the dict run_restatement returns"""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        layers = TC.count_layers(tower, sd)
        if tower == "img":
            D, out_dim = sd["visual.proj"].shape
            patch = sd["visual.conv1.weight"].shape[-1]
            res = patch * round((sd["visual.positional_embedding"].shape[0] - 1) ** 0.5)
            m = VisionTransformer(res, patch, D, layers, D // 64, out_dim)
            m.load_state_dict({k[len("visual."):]: torch.tensor(v) for k, v in sd.items()}, strict=True)
            y = m(torch.tensor(x))
            (y * torch.tensor(up)).sum().backward()
            return _collect(tower, m, y, layers, "visual.")
        D, out_dim = sd["text_projection"].shape
        vocab, context = sd["token_embedding.weight"].shape[0], sd["positional_embedding"].shape[0]
        m = CLIP(out_dim, 4, 0, 64, 4, context, vocab, D, D // 64, layers)
        missing, unexpected = m.load_state_dict({k: torch.tensor(v) for k, v in sd.items()}, strict=False)
        assert not unexpected and all(k.startswith("visual.") or k == "logit_scale" for k in missing), (missing, unexpected)
        y = m.encode_text(torch.tensor(x), key_padding_mask=None if kpm is None else torch.tensor(kpm))
        (y * torch.tensor(up)).sum().backward()
        return _collect(tower, m, y, layers, "")
    finally:
        torch.set_num_threads(threads)


def main():
    out, pool = {}, {"img": {}, "txt": {}}
    for name in TC.CASES:
        tower = TC.tower_of(name)
        sd, x, up, kpm = TC.case_inputs(name)
        ref = run_reference(tower, sd, x, up, kpm)
        r32 = TC.run_restatement(tower, sd, x, up, kpm, torch.float32)
        r64 = TC.run_restatement(tower, sd, x, up, kpm, torch.float64)
        assert sorted(ref) == sorted(r32) == sorted(r64)
        for k in ref:
            assert np.isfinite(ref[k]).all(), (name, k)
            assert np.array_equal(ref[k].reshape(r32[k].shape), r32[k]), (name, k, TC.rel_err(ref[k].reshape(r32[k].shape), r32[k]))      # to the bit
        per, pl = TC.erefs(r32, r64)
        out[name + "__seed"] = np.int64(TC.case_seed(name))
        out[name + "__checksum"] = np.float64(TC.inputs_checksum(sd, x, up, kpm))
        for k in ref:
            out["%s__%s" % (name, k)] = TC.thin(ref[k]).astype(np.float32)
            out["%s__eref_%s" % (name, k)] = np.float64(per[k])
        for k, e in pl.items():
            pool[tower][k] = max(pool[tower].get(k, 0.0), e)
        print("%-26s %s" % (name, " ".join("%s %.1e" % (k[2:] if k != "y" else k, pl[k]) for k in TC.KINDS[tower])))
    for tower in pool:
        print("pooled e_ref (%s):" % tower, " ".join("%s %.2e" % (k, pool[tower][k]) for k in TC.KINDS[tower]))
    path = out_path("tower_grad.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
