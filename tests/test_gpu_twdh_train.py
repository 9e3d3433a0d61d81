"""GPU: TwDH trained end to end.

Chain test: leaf embeddings through ``model.hash`` in train mode, the short-code transforms and ``object_function``, then
``backward()``; the loss and the gradients of every head parameter and of both embeddings against the float64 restatement of that
chain (tests/twdh_cases.py:chain), e <= TOL_FACTOR = 4 times the float32 restatement's e on the same inputs and relu masks -- the
rule of tests/test_gpu_tower_grad.py.  A relu input whose float64 value lies within the near-tie band of tests/test_gpu_head_grad.py
(TIE_FACTOR eps |n| |w|) may be masked either way: there the restatement takes the mask the forward itself stored, never the other
way round.  The two bias gradients in front of the BatchNorm are identically zero and compared absolutely.  One case runs at
long_dim 512 (N = 1024, the head kernels' cap).  Every ratio is printed before the first assertion.  Measured on an MI355X, worst
e / e_ref over the 19 tensors of a case (the bound is 4): 1.03 (g_out_w_txt) at lens (32, 4, 8), B = 37, where the loss has 0.73;
1.26 (g_norm_w_txt) at lens (512, 16, 32, 64), B = 5, where the loss has 0.07.

Runner test: TwDHTrainer.train_epoch_codes on the synthetic dataset, and train() from the constructor."""
import copy
import os
import re
import types

import numpy as np
import pytest
import torch

import twdh_cases as TC

pytestmark = pytest.mark.gpu

SMALL = "synthetic:1814:vision_layers=1,transformer_layers=1,vision_width=128,transformer_width=128,embed_dim=64,image_resolution=64"
LOSS = r"loss: (?:tensor\()?([-+0-9.eE]+|nan|inf)"
E = 64
TIE_CAP = 0.005                                      # oracle/heads_train.py: at most this share of a case's relu inputs


def _saved_f(mod, x):
    """the relu output f [B, N] the train forward stores (layout: include/xmh.h), from a forward of a COPY of the module"""
    c = copy.deepcopy(mod)
    with torch.no_grad():
        probs, xs, saved = c._train_forward(torch.as_tensor(x).cuda())
    B, e = xs.shape
    N = probs.shape[1]
    a256 = lambda v: (v + 255) & ~255                                           # noqa: E731
    off = 3 * a256(B * e * 4) + a256(max(B, e) * 4)
    return saved[off:off + B * N * 4].view(torch.float32).reshape(B, N).cpu().numpy()


@pytest.mark.parametrize("lens,B,C,seed", [((32, 4, 8), 37, 12, 4201), ((512, 16, 32, 64), 5, 16, 4202)])
def test_chain_head_transforms_objective_against_float64(lens, B, C, seed):
    from xmh.models.twdh import TwDH
    rng = np.random.default_rng(seed)
    keys = [str(k) for k in lens[1:]]
    m = TwDH(cfg=None, long_dim=lens[0], clipPath=SMALL, trans="synthetic", short_dims=list(lens[1:]), long_center="synthetic",
             short_center="synthetic", num_classes=C, quan_alpha=0.5, low_rate=0.3)
    P = {"img": TC.draw_head(seed + 1, lens[0], True, E), "txt": TC.draw_head(seed + 2, lens[0], False, E)}
    for mod, head in (("img", m.hash.img_hash), ("txt", m.hash.txt_hash)):
        sd = head.state_dict()
        sd.update({TC.HEAD_KEYS[k]: torch.tensor(v) for k, v in P[mod].items()})
        head.load_state_dict(sd, strict=True)
    m.hash.cuda().train()
    x = {mod: ((rng.random((B, E, 4)).sum(-1) - 2.0) * np.sqrt(3.0)).astype(np.float32) for mod in ("img", "txt")}
    labels = (rng.random((B, C)) < 0.15).astype(np.int64)
    labels[np.arange(B), rng.integers(0, C, B)] = 1
    labels[2] = 0
    labels[2, :2] = 1                                                            # two labels: ties
    torch.manual_seed(seed)
    ties = m.draw_ties()
    bits = TC.targets(labels, [m.long_center.numpy()] + [m.short_center[k].numpy() for k in keys], [ties["long"].numpy()] + [ties[k].numpy() for k in keys])
    T = torch.cat([m.trans[k] for k in keys], 1).numpy()

    port_mask = {"img": _saved_f(m.hash.img_hash, x["img"]) > 0, "txt": _saved_f(m.hash.txt_hash, x["txt"]) > 0}
    leaves = {mod: torch.tensor(x[mod]).cuda().requires_grad_(True) for mod in x}
    li, lt = m.hash.encode_img(leaves["img"]), m.hash.encode_txt(leaves["txt"])
    si, st = m._short_train(li), m._short_train(lt)
    assert li.requires_grad and all(v.requires_grad for v in si.values()) and tuple(st[keys[-1]].shape) == (B, 2 * lens[-1])
    loss, d = m.object_function(li, lt, si, st, labels=labels, ties=ties)
    loss.backward()
    got = {"loss": float(loss.detach())}
    for mod, head in (("img", m.hash.img_hash), ("txt", m.hash.txt_hash)):
        got["g_x_" + mod] = leaves[mod].grad.cpu().numpy()
        for k in TC.HEAD_PARAMS:
            got["g_%s_%s" % (k, mod)] = head.get_parameter(TC.HEAD_KEYS[k]).grad.cpu().numpy()

    args = (x, P, T, bits, lens, 0.5, 0.3)
    R = TC.chain(*args, torch.float64)
    masks = {}
    for mod in ("img", "txt"):
        differ = port_mask[mod] != R["mask_" + mod]
        assert (np.abs(R["z_" + mod]) <= R["tie_" + mod])[differ].all(), "a relu decision differs from float64 outside the near-tie band"
        assert differ.sum() <= TIE_CAP * differ.size
        masks[mod] = np.where(differ, port_mask[mod], R["mask_" + mod])
    R, R32 = TC.chain(*args, torch.float64, masks=masks), TC.chain(*args, torch.float32, masks=masks)
    rows = []
    for key in got:
        want, r32 = R[key], R32[key]
        if key in ("g_in_b_img", "g_out_b_img"):                                 # a bias in front of BatchNorm cancels: identically zero
            want = np.zeros_like(want)
        rows.append((key, TC.rel_err(got[key], want), TC.rel_err(r32, want)))
    for key, e, e_ref in rows:
        print("lens %s B %d  %-14s e %.3e  e_ref %.3e  ratio %.2f" % (lens, B, key, e, e_ref, e / e_ref if e_ref else float("inf")))
    for key, e, e_ref in rows:
        assert e <= TC.TOL_FACTOR * e_ref, (key, e, e_ref)
    assert float(d["All loss"]) == got["loss"] and np.isfinite(got["loss"])


def _trainer(tmp_path, autorun=False, lines=None, **run):
    import xmh.models  # noqa: F401
    import xmh.runners  # noqa: F401
    from xmh.common.register import registry
    from xmh.utils.config import Config
    cfg = Config({
        "model": {"arch": "TwDH", "clip_path": SMALL, "long_dim": 32, "trans_matrix": "synthetic", "short_dims": [8, 16], "long_center": "synthetic",
                  "short_center": "synthetic", "num_classes": 6, "low_rate": 0.3},
        "dataset": {"arch": "synthetic", "name": "synth", "num_classes": 6, "retrieval_num": 16, "max_word": 32, "image_resolution": 64},
        "optimizer": {"lr": 0.001, "backbone_lr": 0.00001},
        "run": dict({"arch": "TwDHTrainer", "output_dim": 16, "device": 0, "batch_size": 4, "num_workers": 0, "is_train": True, "query_num": 8,
                     "train_num": 8, "epochs": 1, "save_dir": str(tmp_path), "log_dir": str(tmp_path), "seed": 1814}, **run),
    })
    lines = [] if lines is None else lines
    t = registry.get_runner_class("TwDHTrainer").from_config(cfg=cfg, autorun=autorun, logger=types.SimpleNamespace(info=lines.append))
    t.lines = lines
    return t


def test_train_epoch_codes_moves_every_parameter_and_repeats_to_the_bit(tmp_path):
    finals, losses = [], []
    for _ in range(2):
        torch.manual_seed(1814)                                                  # the tie draws come from the CPU's global generator
        t = _trainer(tmp_path, epochs=2)
        before = {n: p.detach().clone() for n, p in t.model.named_parameters()}
        assert getattr(t, "optimizer", None) is None
        t.train_epoch_codes(0)
        t.train_epoch_codes(1)
        steps = 2 * len(t.train_loader)
        assert len(t.train_loader) == 2 and t.global_step == steps
        epoch_lines = [line for line in t.lines if re.match(r">>>>>> \[\d/2\] loss: ", line)]
        assert len(epoch_lines) == 2, t.lines
        print(epoch_lines[-1])
        assert re.fullmatch(r">>>>>> \[1/2\] loss: .+, lr: [0-9.]+(-[0-9.]+)*", epoch_lines[-1]), epoch_lines[-1]      # runner.py:137
        losses.append([float(re.search(LOSS, line).group(1)) for line in epoch_lines])
        assert np.isfinite(losses[-1]).all()
        for n, p in t.model.named_parameters():
            if n == "backbone.logit_scale":
                assert torch.equal(p.detach(), before[n]) and p.grad is None
            elif p.requires_grad:
                assert n.startswith("backbone.") or n.startswith("hash."), n
                assert p.grad is not None and not torch.equal(p.detach(), before[n]), n
                assert bool(torch.isfinite(p).all()), n
        finals.append({n: p.detach().clone() for n, p in t.model.named_parameters()})
    assert losses[0] == losses[1]
    assert all(torch.equal(finals[0][n], finals[1][n]) for n in finals[0])


def test_is_train_runs_train_then_valid_from_the_constructor(tmp_path):
    lines = []
    t = _trainer(tmp_path, autorun=True, lines=lines)
    assert t.global_step == len(t.train_loader)
    order = [i for i, line in enumerate(lines) if re.match(r">>>>>> \[0/1\] loss: ", line) or line == "Valid." or "FINISHED" in line]
    assert len(order) == 3 and re.match(r">>>>>> \[0/1\] loss: ", lines[order[0]]) and lines[order[1]] == "Valid." and "FINISHED" in lines[order[2]]
    files = set(os.listdir(os.path.join(str(tmp_path), "mat_files")))
    assert {"i2t-long.mat", "t2i-long.mat", "i2t-short-8.mat", "t2i-short-16.mat"} <= files, files
    with pytest.raises(NotImplementedError, match="TwDH's head"):
        t.train_epoch(0)
    t.distributed = True
    with pytest.raises(NotImplementedError, match="all-reduce"):
        t.train_epoch_codes(0)
