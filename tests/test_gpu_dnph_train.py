"""GPU: DNPH trained end to end.

Chain test: leaf embeddings through ``model.hash`` in train mode (a given keep mask per modality), then ``object_function`` with given
noise vectors, then ``backward()``; the loss and the gradients of every head parameter, of the proxies and of both embeddings against
the float64 restatement of that chain (tests/dnph_cases.py:chain), e <= TOL_FACTOR = 4 times the float32 restatement's e on the same
inputs -- the rule of tests/test_gpu_tower_grad.py.  The noise vectors assigned to the codes are constants of the objective: the
restatement takes the assignment the port made, after checking that its own codes lead to the same one.  Every ratio is printed
before the first assertion.  Measured on an MI355X, worst e / e_ref over the 12 tensors of a case (the bound is 4): 1.76 (loss) at
B = 37, K = 16, C = 12; 1.92 (g_hash_b_img) at B = 5, K = 64, C = 24; 1.99 (g_hash_b_img) at B = 37, K = 64, C = 80; 1.25 (g_pre_b_img)
at B = 5, K = 16, C = 5.

Runner tests: DNPHTrainer.train_epoch on the synthetic dataset, train() from the constructor, valid() after it."""
import os
import re
import types

import numpy as np
import pytest
import torch

import dnph_cases as DC

pytestmark = pytest.mark.gpu

SMALL = "synthetic:1814:vision_layers=1,transformer_layers=1,vision_width=128,transformer_width=128,embed_dim=64,image_resolution=64"
LOSS = r"loss: (?:tensor\()?([-+0-9.eE]+|nan|inf)"
E = 64


@pytest.mark.parametrize("B,K,C,seed", [(37, 16, 12, 5301), (5, 64, 24, 5302), (37, 64, 80, 5303), (5, 16, 5, 5304)])
def test_chain_head_objective_against_float64(B, K, C, seed):
    from xmh.models.dnph import DNPH, gene_noise
    rng = np.random.default_rng(seed)
    m = DNPH(cfg=None, outputDim=K, clipPath=SMALL, numclass=C, mrg=1.0, noise_alpha=0.1)
    Pm = {"img": DC.draw_head(seed + 1, K, E), "txt": DC.draw_head(seed + 2, K, E)}
    sd = m.hash.state_dict()
    for mod in Pm:
        sd.update({DC.HEAD_KEYS[k] % DC.MOD[mod]: torch.tensor(v) for k, v in Pm[mod].items()})
    m.hash.load_state_dict(sd, strict=True)
    m.hash.cuda().train()
    m.loss.cuda()
    x = {mod: ((rng.random((B, E, 4)).sum(-1) - 2.0) * np.sqrt(3.0)).astype(np.float32) for mod in ("img", "txt")}
    keep = {mod: (rng.random((B, K)) >= 0.2).astype(np.uint8) for mod in ("img", "txt")}
    labels = (rng.random((B, C)) < 0.15).astype(np.int64)
    labels[np.arange(B), rng.integers(0, C, B)] = 1
    labels[0] = 0
    labels[1] = 1
    s_vector = rng.integers(0, 2, (B, K)) * 2 - 1

    leaves = {mod: torch.tensor(x[mod]).cuda().requires_grad_(True) for mod in x}
    fi, pi = m.hash.encode_img(leaves["img"], keep=torch.tensor(keep["img"]))
    ft, pt = m.hash.encode_txt(leaves["txt"], keep=torch.tensor(keep["txt"]))
    assert fi.requires_grad and pi.requires_grad and tuple(fi.shape) == (B, K) and tuple(pt.shape) == (B, 80)
    assert bool((fi[torch.tensor(keep["img"] == 0).cuda()] == 0).all())              # the given mask was the one applied
    loss, d = m.object_function(fi, ft, pi, pt, labels=torch.tensor(labels), noises=s_vector)
    loss.backward()
    got = {"loss": loss.detach().cpu().double().numpy().reshape(1), "g_P": m.loss.proxies.grad.cpu().double().numpy()}
    for mod in ("img", "txt"):
        got["g_x_" + mod] = leaves[mod].grad.cpu().double().numpy()
        for k in DC.HEAD_PARAMS:
            got["g_%s_%s" % (k, mod)] = m.hash.get_parameter(DC.HEAD_KEYS[k] % DC.MOD[mod]).grad.cpu().double().numpy()

    noises = {"img": gene_noise(fi.detach().cpu().numpy(), s_vector).astype(np.float32),
              "txt": gene_noise(ft.detach().cpu().numpy(), s_vector).astype(np.float32)}
    args = (x, Pm, keep, m.loss.proxies.detach().cpu().numpy(), labels, noises, 1.0, 0.1, 0.2)
    R, R32 = DC.chain(*args, torch.float64), DC.chain(*args, torch.float32)
    for mod in ("img", "txt"):                                                       # the restatement's codes lead to the same assignment
        assert np.array_equal(gene_noise(R["f_" + mod].astype(np.float32), s_vector), noises[mod])
    rows = [(key, DC.rel_err(got[key], R[key]), DC.rel_err(R32[key], R[key])) for key in got]
    for key, e, e_ref in rows:
        print("B %d K %d C %d  %-14s e %.3e  e_ref %.3e  ratio %.2f" % (B, K, C, key, e, e_ref, e / e_ref if e_ref else float("inf")))
    for key, e, e_ref in rows:
        assert e <= DC.TOL_FACTOR * e_ref, (key, e, e_ref)
    assert float(d["All loss"]) == float(got["loss"][0]) and np.isfinite(got["loss"]).all()
    assert not d["All loss"].requires_grad and not d["Noise"]["image"].requires_grad and float(d["Noise"]["text"]) > 0


def _trainer(tmp_path, autorun=False, lines=None, **run):
    import xmh.models  # noqa: F401
    import xmh.runners  # noqa: F401
    from xmh.common.register import registry
    from xmh.utils.config import Config
    cfg = Config({
        "model": {"arch": "DNPH", "clip_path": SMALL, "numclass": 6, "mrg": 1.0, "noise_alpha": 0.1, "hash_func": "tanh", "seed": 1814},
        "dataset": {"arch": "synthetic", "name": "synth", "num_classes": 6, "retrieval_num": 16, "max_word": 32, "image_resolution": 64},
        "optimizer": {"lr": 0.001, "backbone_lr": 0.00001, "loss": {"lr": 0.01}},
        "run": dict({"arch": "DNPHTrainer", "output_dim": 16, "device": 0, "batch_size": 4, "num_workers": 0, "is_train": True, "query_num": 8,
                     "train_num": 8, "epochs": 1, "save_dir": str(tmp_path), "log_dir": str(tmp_path), "seed": 1814}, **run),
    })
    lines = [] if lines is None else lines
    t = registry.get_runner_class("DNPHTrainer").from_config(cfg=cfg, autorun=autorun, logger=types.SimpleNamespace(info=lines.append))
    t.lines = lines
    return t


def test_train_epoch_moves_every_parameter_and_steps_both_optimisers(tmp_path):
    t = _trainer(tmp_path, epochs=2, display_step=2)
    before = {n: p.detach().clone() for n, p in t.model.named_parameters()}
    assert getattr(t, "optimizer", None) is None
    t.train_epoch(0)
    t.train_epoch(1)
    assert len(t.train_loader) == 2 and t.global_step == 4
    assert isinstance(t.optimizer_loss, torch.optim.SGD) and t.optimizer_loss.param_groups[0]["lr"] == 0.01
    assert [id(p) for p in t.optimizer_loss.param_groups[0]["params"]] == [id(t.model.loss.proxies)]
    epoch_lines = [line for line in t.lines if re.match(r">>>>>> \[\d/2\] loss: ", line)]
    assert len(epoch_lines) == 2, t.lines
    print(epoch_lines[-1])
    assert np.isfinite([float(re.search(LOSS, line).group(1)) for line in epoch_lines]).all()
    assert any("Noise: image: " in line for line in t.lines), t.lines                 # the display line carries the nested dictionary
    groups = {"backbone.": 0, "hash.": 0, "loss.": 0}
    for n, p in t.model.named_parameters():
        if n == "backbone.logit_scale":
            assert torch.equal(p.detach(), before[n]) and p.grad is None
        elif p.requires_grad:
            assert p.grad is not None and not torch.equal(p.detach(), before[n]), n
            assert bool(torch.isfinite(p).all()), n
            groups[next(g for g in groups if n.startswith(g))] += 1
    assert groups["loss."] == 1 and groups["hash."] == 8 and groups["backbone."] > 20, groups
    assert all(len(t.optimizer.state[p]) > 0 for g in t.optimizer.param_groups for p in g["params"] if p.grad is not None)


def test_is_train_runs_train_then_valid_from_the_constructor(tmp_path):
    lines = []
    t = _trainer(tmp_path, autorun=True, lines=lines)
    assert t.global_step == len(t.train_loader)
    order = [i for i, line in enumerate(lines) if re.match(r">>>>>> \[0/1\] loss: ", line) or line == "Valid." or "FINISHED" in line]
    assert len(order) == 3 and re.match(r">>>>>> \[0/1\] loss: ", lines[order[0]]) and lines[order[1]] == "Valid." and "FINISHED" in lines[order[2]]
    assert os.path.isdir(os.path.join(str(tmp_path), "mat_files"))
    maps = t.valid(1, k=t.top_k)                                                     # valid() again, after train(): through generate_hash
    assert len(maps) == 4 and all(0.0 <= v <= 1.0 for v in maps) and max(maps) > 0.0
    assert t.max_mapi2t >= maps[0] and t.max_mapt2i >= maps[1]
    assert {"last.mat", "i2t-best.mat"} <= set(os.listdir(os.path.join(str(tmp_path), "mat_files")))
    t.distributed = True
    with pytest.raises(NotImplementedError, match="all-reduce"):
        t.train_epoch(0)
