#!/usr/bin/env python3
"""Golden outputs and gradients of MITH's hash head in training mode, produced by the UNMODIFIED reference HashLayer
(models/MITH/hash/hash.py) through oracle._ref_import, in .train() on the CPU in fp32:
    python tools/make_golden_mith_head_grad.py [DIR] -> tests/golden/mith_head_grad.npz (or DIR/).
Needs the reference checkout; nothing at test time runs or imports this.

Cases, seeds, the thinning rule and the restatement live in tests/mith_head_grad_cases.py.  Per case <c>: `<c>__seed`, `<c>__checksum`
of the regenerated parameters / inputs / mask / upstream gradients, the reference's fp32 outputs and the gradients of
sum_i (output_i . up_i).sum() as `<c>__<tensor>` (thinned), and per tensor `<c>__eref_<tensor>` = max|fp32 - fp64| / max|fp64| on the
whole tensor, the fp64 side being the restatement.  Asserted here: the restatement's fp32 run equals the reference's to the bit, and
its fp32 and fp64 runs select the same LTA entries in every case, so the stored tensors belong to the keep-set the fp64 side uses.

`lta_parent__crc` / `lta_parent__thin`: xmh_lta_aggregate's output on MC.lta_inputs() as the library computed it BEFORE its kernel body
moved into csrc/xmh_lta.h (crc32 of the whole [B, K, D] fp32 output, and every THIN-th element).  That run needs a GPU and the earlier
library, so the two entries are carried over from the existing golden file unless a second argument names an .npz holding `out`.
"""
import os
import sys
import types
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mith_head_grad_cases as MC  # noqa: E402
from oracle import _ref_import  # noqa: E402
from oracle.fixtures import out_path  # noqa: E402

_ref_import.setup()
for _pkg in ("models.MITH.hash",):                    # as oracle/make_golden_mith.py: the package __init__ would pull in einops
    _m = types.ModuleType(_pkg)
    _m.__path__ = [os.path.join(_ref_import.REF, *_pkg.split("."))]
    sys.modules.setdefault(_pkg, _m)
from models.MITH.hash.hash import HashLayer  # noqa: E402  (the reference class)


def run_reference(sd, cls, tok, mask, ups, D, layers, R, K, top_k, mod):
    """the reference's HashLayer in .train(), fp32 -> the dict run_restatement returns (without "keep")"""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        m = HashLayer(clip_embed_dim=D, k_bits=K, dropout=0.0, transformer_layers=layers, activation="gelu", top_k_label=top_k,
                      res_mlp_layers=R).train()
        m.load_state_dict(MC.ref_state(sd, m.state_dict(), mod), strict=True)
        ct, tt = torch.tensor(cls).requires_grad_(True), torch.tensor(tok).requires_grad_(True)
        outs = m.encode_img(ct, tt) if mod == "img" else m.encode_txt(ct, tt, torch.tensor(mask))
        sum((o * torch.tensor(u)).sum() for o, u in zip(outs, ups)).backward()
        out = {n: o.detach().numpy().copy() for n, o in zip(MC.OUTPUTS, outs)}
        out["g_cls"], out["g_tokens"] = ct.grad.numpy().copy(), tt.grad.numpy().copy()
        gcl, lct, proj = (m.gcl_i, m.lct_i, m.img_concept_proj) if mod == "img" else (m.gcl_t, m.lct_t, m.txt_concept_proj)
        for i in range(R):
            for f, p in zip(MC.MLP_FIELDS, (gcl.mlp.lns[i].weight, gcl.mlp.lns[i].bias, gcl.mlp.mlps[i][0].weight, gcl.mlp.mlps[i][0].bias,
                                            gcl.mlp.mlps[i][3].weight, gcl.mlp.mlps[i][3].bias)):
                out["g_mlp%d_%s" % (i, f)] = p.grad.numpy().copy()
        out["g_concept"] = gcl.common_concept_embedding.weight.grad.numpy().copy()
        for i in range(layers):
            for kind, key in MC.BC.PARAMS:
                out["g_l%d_%s" % (i, kind)] = lct.transformer.get_parameter("resblocks.%d.%s" % (i, key)).grad.numpy().copy()
        out["g_hash_w"] = np.concatenate([fc.weight.grad.numpy() for fc in lct.hashing.fc_list], 0)
        out["g_hash_b"] = np.concatenate([fc.bias.grad.numpy() for fc in lct.hashing.fc_list], 0)
        out["g_proj_w"], out["g_proj_b"] = proj.weight.grad.numpy().copy(), proj.bias.grad.numpy().copy()
        return out
    finally:
        torch.set_num_threads(threads)


def main():
    out, pool = {}, {}
    for name, (D, heads, layers, R, K, top_k, L, B, mod, mk) in MC.CASES.items():
        sd, cls, tok, mask, ups = MC.case_inputs(name)
        ref = run_reference(sd, cls, tok, mask, ups, D, layers, R, K, top_k, mod)
        s32, s64 = [], []
        r32 = MC.run_restatement(sd, cls, tok, mask, ups, heads, top_k, torch.float32, scores_out=s32)
        r64 = MC.run_restatement(sd, cls, tok, mask, ups, heads, top_k, torch.float64, scores_out=s64)
        k32, k64 = r32.pop("keep"), r64.pop("keep")
        assert np.array_equal(k32, k64), (name, "the fp32 and fp64 runs select different LTA entries: choose another seed", int((k32 != k64).sum()))
        margin = MC.selection(s64[0], mask, top_k)[1]
        assert sorted(ref) == sorted(r32) == sorted(r64)
        for k in ref:
            assert np.isfinite(ref[k]).all(), (name, k)
            assert np.array_equal(ref[k], r32[k]), (name, k, MC.rel_err(ref[k], r32[k]))      # to the bit
        empty = int((~k64.any(axis=0)).sum())
        assert (name in MC.EMPTY_CONCEPT_CASES) <= (empty > 0), (name, "no (sample, concept) without a positive score")
        if mk == "pad_all":
            assert not k64[:, 1].any() and not ref["g_tokens"][:, 1].any()
        per, pl = MC.erefs(ref, r64)
        out[name + "__seed"] = np.int64(MC.case_seed(name))
        out[name + "__checksum"] = np.float64(MC.inputs_checksum(sd, cls, tok, mask, ups))
        for k in ref:
            out["%s__%s" % (name, k)] = MC.thin(ref[k]).astype(np.float32)
            out["%s__eref_%s" % (name, k)] = np.float64(per[k])
        for k, e in pl.items():
            pool[k] = max(pool.get(k, 0.0), e)
        print("%-32s kept %d of %d, empty (sample, concept) %d, smallest margin %.1e; %s" % (
            name, int(k64.sum()), k64.size, empty, float(margin.min()), " ".join("%s %.1e" % (k, pl[k]) for k in sorted(pl))))
    print("pooled e_ref:", " ".join("%s %.2e" % (k, pool[k]) for k in sorted(pool)))
    path = out_path("mith_head_grad.npz")
    if len(sys.argv) > 2:
        parent = np.load(sys.argv[2])["out"].astype(np.float32)
        out["lta_parent__crc"] = np.float64(zlib.crc32(np.ascontiguousarray(parent).tobytes()))
        out["lta_parent__thin"] = MC.thin(parent)
    elif os.path.exists(MC.GOLDEN):
        old = np.load(MC.GOLDEN)
        out.update({k: old[k] for k in ("lta_parent__crc", "lta_parent__thin") if k in old.files})
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
