#!/usr/bin/env python3
"""Golden trajectories of BertAdam, produced by the UNMODIFIED reference class (models/common/optimizer.py) through
oracle._ref_import, on the CPU, once in fp32 and once in fp64 on the same seeded parameters and gradients:
python tools/make_golden_bertadam.py [DIR] -> tests/golden/bertadam.npz (or DIR/).  Needs the reference checkout and the built
library (for the chunk length of the `large` case); nothing at test time runs or imports this.

Cases, seeds, the thinning rule and the file layout live in tests/bertadam_cases.py.  Per stored case: p, next_m, next_v and the
post-step grad of every step and tensor of the fp64 run, concatenated (`<case>__f64`), the fp32 run as its distance in units of
the last place from the rounded fp64 value (`<case>__ulp`, int32: exact, and it compresses to about a byte per element), the
get_lr() lists (`<case>__lr`) and the step counters (`<case>__count`, -1 = no state yet).
Yardstick: e = max|fp32 - fp64| / max|fp64| per whole tensor, pooled (max) per kind over every case, step and tensor that has a
finite value -> `eref_<kind>`; the same over the `large` case alone -> `large_eref_<kind>` (its tensors are not stored).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "clip-based-cross-modal-hash_amd"))
import bertadam_cases as BC  # noqa: E402
from oracle import _ref_import  # noqa: E402
from oracle.fixtures import out_path  # noqa: E402

_ref_import.setup()
from models.common.optimizer import BertAdam  # noqa: E402  (the reference class)

STATE = {"m": "next_m", "v": "next_v"}


def run_reference(case, chunk, dtype):
    """-> list over steps of dict(kind -> per-tensor numpy arrays or None, lr, count)"""
    tensors, steps, nan = BC.resolve(case, chunk)
    params = [torch.nn.Parameter(torch.tensor(BC.draw_param(case, t, s["shape"])).to(dtype)) for t, s in enumerate(tensors)]
    groups = []
    for gi in sorted({s["group"] for s in tensors}):
        members = [t for t, s in enumerate(tensors) if s["group"] == gi]
        groups.append(dict(params=[params[t] for t in members], **tensors[members[0]]["hyper"]))
    opt = BertAdam(groups, lr=BC.DEFAULTS["lr"])
    out = []
    for s in range(steps):
        for t, p in enumerate(params):
            g = BC.draw_grad(case, tensors, t, s, nan)
            p.grad = None if g is None else torch.tensor(g).to(dtype)
        opt.step()
        rec = {k: [None] * len(params) for k in BC.KINDS}
        for t, p in enumerate(params):
            st = opt.state[p]
            rec["p"][t] = p.detach().numpy().copy()
            if len(st):
                rec["m"][t], rec["v"][t] = st["next_m"].numpy().copy(), st["next_v"].numpy().copy()
            if p.grad is not None:
                rec["grad"][t] = p.grad.numpy().copy()
        rec["lr"] = [float(x) for x in opt.get_lr()]
        rec["count"] = [opt.state[p]["step"] if len(opt.state[p]) else -1 for p in params]
        out.append(rec)
    return out


def main():
    from xmh import _lib
    chunk = int(_lib.lib.xmh_bertadam_chunk())
    out, pool, large = {"chunk_when_written": np.int64(chunk)}, {k: 0.0 for k in BC.KINDS}, {k: 0.0 for k in BC.KINDS}
    p0 = BertAdam([torch.nn.Parameter(torch.zeros(3))], lr=0.1)
    p0.param_groups[0]["params"][0].grad = torch.ones(3)
    assert p0.get_lr() == [0]                                                    # before the first step
    for case, spec in BC.CASES.items():
        r32, r64 = run_reference(case, chunk, torch.float32), run_reference(case, chunk, torch.float64)
        own, values = BC.run_f64(case, chunk), {}
        for s, (a, b, c) in enumerate(zip(r32, r64, own)):
            assert a["count"] == b["count"] == [-1 if x is None else x for x in c["count"]], (case, s)
            assert np.allclose(a["lr"], b["lr"], rtol=0, atol=0) and np.allclose(b["lr"], c["lr"], rtol=1e-15, atol=0), (case, s)
            for kind in BC.KINDS:
                for t, (x, y) in enumerate(zip(a[kind], b[kind])):
                    assert (x is None) == (y is None)
                    if x is None:
                        continue
                    if np.isfinite(y).all():
                        assert np.isfinite(x).all(), (case, s, t, kind)
                        e = BC.rel_err(x, y)
                        pool[kind] = max(pool[kind], e)
                        if case == "large":
                            large[kind] = max(large[kind], e)
                        assert BC.rel_err(c[kind][t], y) <= 1e-12, (case, s, t, kind)      # the restatement follows the reference
                    else:
                        assert np.array_equal(np.isnan(x), np.isnan(y)), (case, s, t, kind)
                    values[(s, t, kind)] = (y, x)
        if spec.get("stored", True):
            out.update(BC.pack(case, values))
            out[case + "__lr"] = np.concatenate([np.asarray(b["lr"], dtype=np.float64) for b in r64])
            out[case + "__count"] = np.asarray([b["count"] for b in r64], dtype=np.int64)
        print("%-10s steps %d  e_ref so far: %s" % (case, len(r32), " ".join("%s %.2e" % (k, pool[k]) for k in BC.KINDS)))
    for k in BC.KINDS:
        out["eref_" + k], out["large_eref_" + k] = np.float64(pool[k]), np.float64(large[k])
    path = out_path("bertadam.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
