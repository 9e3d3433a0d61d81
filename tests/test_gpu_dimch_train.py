"""GPU: DIMCH trained end to end: DIMCHTrainer.train_epoch on the synthetic dataset over a tiny synthetic backbone
(5 image tokens, 32 text tokens, E = 64) with setDim 3 -- both towers' token outputs, the token-set head in train mode and the
set-distance objective behind torch.autograd, BertAdam; then valid()."""
import os
import re
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SMALL = "synthetic:1814:vision_layers=1,transformer_layers=1,vision_width=128,transformer_width=128,embed_dim=64,image_resolution=64"
LOSS = r"loss: (?:tensor\()?([-+0-9.eE]+|nan|inf)"


def _trainer(tmp_path, autorun=False, lines=None, hash_func="tanh", **run):
    import xmh.models  # noqa: F401
    import xmh.runners  # noqa: F401
    from xmh.common.register import registry
    from xmh.utils.config import Config
    cfg = Config({
        "model": {"arch": "DIMCH", "clip_path": SMALL, "setDim": 3, "dropout": 0.3, "hash_func": hash_func, "merge_func": "mean", "seed": 1814,
                  "distance": {"mode": "smooth_chamfer", "denominator": 2.0, "temperature": 16.0, "temperature_txt_scale": 1.0},
                  "chamfer": {"mmd_gamma": 0.5, "mmd_alpha": 1, "unif_alpha": 0.3, "token_triplet_margin": 0.3},
                  "hash_pars": {"triplet_alpha": 50, "quan_alpha": 1.0, "hash_triplet_alpha": 50, "triplet_margin": 0.3}},
        "dataset": {"arch": "synthetic", "name": "synth", "num_classes": 6, "retrieval_num": 16, "max_word": 32, "image_resolution": 64},
        "optimizer": {"lr": 0.001, "backbone_lr": 0.00001},
        "run": dict({"arch": "DIMCHTrainer", "output_dim": 16, "device": 0, "batch_size": 4, "num_workers": 0, "is_train": True, "query_num": 8,
                     "train_num": 8, "epochs": 1, "save_dir": str(tmp_path), "log_dir": str(tmp_path), "seed": 1814}, **run),
    })
    lines = [] if lines is None else lines
    torch.manual_seed(1814)                                                          # the loader's order and the dropout masks
    t = registry.get_runner_class("DIMCHTrainer").from_config(cfg=cfg, autorun=autorun, logger=types.SimpleNamespace(info=lines.append))
    t.lines = lines
    return t


def test_two_steps_move_every_parameter_and_repeat_to_the_bit(tmp_path):
    t = _trainer(tmp_path, display_step=1)
    assert t.hash_scale == 1 and tuple(t.model.hash.txt_token_hash.token_layer.weight.shape) == (3, 32, 3)
    before = {n: p.detach().clone() for n, p in t.model.named_parameters()}
    assert getattr(t, "optimizer", None) is None
    t.train_epoch(0)
    assert len(t.train_loader) == 2 and t.global_step == 2
    epoch_lines = [line for line in t.lines if re.match(r">>>>>> \[0/1\] loss: ", line)]
    assert len(epoch_lines) == 1, t.lines
    print(epoch_lines[-1])
    assert np.isfinite(float(re.search(LOSS, epoch_lines[0]).group(1)))
    assert any("Maximum Mean Discrepancy: " in line and "Quantization: image: " in line for line in t.lines), t.lines
    groups = {"backbone.": 0, "hash.": 0}
    for n, p in t.model.named_parameters():
        if n == "backbone.logit_scale":
            assert torch.equal(p.detach(), before[n]) and p.grad is None
        elif p.requires_grad:
            assert p.grad is not None and not torch.equal(p.detach(), before[n]), n
            assert bool(torch.isfinite(p).all()) and bool(torch.isfinite(p.grad).all()), n
            groups[next(g for g in groups if n.startswith(g))] += 1
    assert groups["hash."] == 12 and groups["backbone."] > 20, groups
    again = _trainer(tmp_path, display_step=1)
    again.train_epoch(0)
    for (n, p), (_, q) in zip(t.model.named_parameters(), again.model.named_parameters()):
        assert torch.equal(p.detach(), q.detach()), n
    t.distributed = True
    with pytest.raises(NotImplementedError, match="all-reduce"):
        t.train_epoch(0)


def test_is_train_runs_train_then_valid_with_tanh(tmp_path):
    lines = []
    t = _trainer(tmp_path, autorun=True, lines=lines)
    assert t.global_step == len(t.train_loader)
    order = [i for i, line in enumerate(lines) if re.match(r">>>>>> \[0/1\] loss: ", line) or line == "Valid." or "FINISHED" in line]
    assert len(order) == 3 and lines[order[1]] == "Valid." and "FINISHED" in lines[order[2]]
    maps = t.valid(1, k=t.top_k)
    assert len(maps) == 4 and all(0.0 <= v <= 1.0 for v in maps) and max(maps) > 0.0
    assert {"last.mat", "i2t-best.mat"} <= set(os.listdir(os.path.join(str(tmp_path), "mat_files")))
    img = torch.randn(3, 3, 64, 64).cuda()
    txt = next(iter(t.query_loader))[1][:3].cuda()
    e_img, h_img, e_txt, h_txt = t.model(img, txt)
    assert tuple(e_img.shape) == (3, 3, 16) and tuple(h_img.shape) == (3, 16) and tuple(e_txt.shape) == (3, 3, 16) and tuple(h_txt.shape) == (3, 16)
    a, b = t.generate_hash(img, txt)
    assert torch.equal(a, h_img) and torch.equal(b, h_txt) and set(t.merge_hash(a, b).unique().tolist()) <= {-1.0, 0.0, 1.0}


def test_softmax_trains_and_valid_says_what_is_not_built(tmp_path):
    t = _trainer(tmp_path, hash_func="softmax")
    assert t.hash_scale == 2 and t.model.output_dim == 32 and tuple(t.model.hash.img_token_hash.hash_layer[3].weight.shape) == (32, 32)
    t.train_epoch(0)
    line = [line for line in t.lines if re.match(r">>>>>> \[0/1\] loss: ", line)][0]
    assert np.isfinite(float(re.search(LOSS, line).group(1)))
    with pytest.raises(NotImplementedError, match="softmax"):
        t.valid(0)
