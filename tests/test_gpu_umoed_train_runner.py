"""GPU: UMoED trained end to end: UMoEDTrainer.train_epoch_decoder / train_decoder / run() on the synthetic dataset over the
tiny synthetic backbone and configuration of tests/test_gpu_umoed_runner.py (5 image tokens, 32 text tokens, E = 64, setDim 4, V = 2, one
decoder layer of one head, 2 x 2 experts, dropout 0.3) with ``is_train: True``, ``train_num: 8``, ``batch_size: 4`` -- two batches an epoch
through both towers, the train-mode decoder head with its six dropout sites, the objective and the fused BertAdam.  The keep masks come from
a seeded generator on the head, so two trainers built from the same seeds end in the same bits."""
import os
import re
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SMALL = "synthetic:1814:vision_layers=1,transformer_layers=1,vision_width=128,transformer_width=128,embed_dim=64,image_resolution=64"
UNTOUCHED = ("backbone.logit_scale",)          # no output of the towers' token paths reads it: no gradient, no step


def _trainer(tmp_path, fusion=True, **run):
    import xmh.models  # noqa: F401
    import xmh.runners  # noqa: F401
    from xmh.common.register import registry
    from xmh.utils.config import Config
    cfg = Config({
        "model": {"arch": "UMoED", "clip_path": SMALL, "setDim": 4, "dropout": 0.3, "extreme": True, "extreme_T": 0.3, "triplet": True,
                  "distance_mode": "cosine", "MoE": True, "fusion": fusion, "num_experts": 2, "slots_per_expert": 2, "hash_func": "linear_subspace",
                  "merge_func": "concatenate", "decoder_heads": 1, "decoder_layers": 1, "hidden_dim": 64, "seed": 1814,
                  "distance": {"mode": "pairwise"}, "chamfer": {"unif_alpha": 0.8, "token_triplet_margin": 0.1},
                  "hash_pars": {"triplet_alpha": 1, "triplet_margin": 0.3}},
        "dataset": {"arch": "synthetic", "name": "synth", "num_classes": 6, "retrieval_num": 16, "max_word": 32, "image_resolution": 64},
        "optimizer": {"lr": 0.001, "backbone_lr": 0.00001},
        "run": dict({"arch": "UMoEDTrainer", "output_dim": 4, "device": 0, "batch_size": 4, "num_workers": 0, "is_train": True, "query_num": 8,
                     "train_num": 8, "epochs": 1, "save_dir": str(tmp_path), "log_dir": str(tmp_path), "seed": 1814}, **run),
    })
    lines = []
    t = registry.get_runner_class("UMoEDTrainer").from_config(cfg=cfg, autorun=False, logger=types.SimpleNamespace(info=lines.append))
    t.lines = lines
    layer = t.model.hash
    for i, head in enumerate([layer.hash_module] if layer.fusion else [layer.img_token_hash, layer.txt_token_hash]):
        head.generator = torch.Generator(device="cuda").manual_seed(1814 + i)      # the dropout masks
    return t


def _loss_of(line):
    return float(re.search(r"loss: (?:tensor\()?([-+0-9.eE]+|nan|inf)", line).group(1))


def test_train_epoch_decoder_moves_every_parameter_and_repeats_to_the_bit(tmp_path):
    finals = []
    for _ in range(2):
        t = _trainer(tmp_path, display_step=1)
        before = {n: p.detach().clone() for n, p in t.model.named_parameters()}
        assert t.is_train and getattr(t, "optimizer", None) is None
        t.train_epoch_decoder(0)
        steps = len(t.train_loader)
        assert steps == 2 and t.global_step == steps and t.model.training
        line = t.lines[-1]
        print(line)
        assert np.isfinite(_loss_of(line)) and "lr: " in line
        assert any("Display" in s and "Similarity" in s and "Diversity" in s for s in t.lines)          # the loss line of a display step
        still = [n for n, p in t.model.named_parameters() if torch.equal(p.detach(), before[n])]
        print("unchanged:", still)
        assert tuple(still) == UNTOUCHED and t.model.backbone.logit_scale.grad is None
        for n, p in t.model.named_parameters():
            assert bool(torch.isfinite(p).all()), n
            if n not in UNTOUCHED:
                assert n.startswith("backbone.") or n.startswith("hash.hash_module."), n
                assert t.optimizer.state[p]["step"] == steps, n
        finals.append({k: v.detach().clone() for k, v in t.model.state_dict().items()})
    assert all(torch.equal(finals[0][k], finals[1][k]) for k in finals[0])


def test_forward_train_heads_leaves_the_towers_alone_and_forward_train_reaches_them(tmp_path):
    t = _trainer(tmp_path)
    t.change_state(mode="train")
    image, text, _, label, index = next(iter(t.train_loader))
    image, text = image.cuda(), text.cuda()
    out = t.model.forward_train_heads(image, text)
    assert len(out) == 6 and out[4] is None and out[5] is None and out[0].requires_grad and not out[1].requires_grad
    loss = t.compute_loss(**dict(zip(t.FORWARD_OUTPUTS, out)), label=label, index=index)
    loss.backward()
    assert all(p.grad is None for p in t.model.backbone.parameters())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in t.model.hash.parameters())
    t.model.zero_grad(set_to_none=True)
    out = t.model.forward_train(image, text)
    assert len(out) == 6 and out[4] is None and tuple(out[0].shape) == (4, 4, 2) and tuple(out[3].shape) == (4, 4)
    t.compute_loss(**dict(zip(t.FORWARD_OUTPUTS, out)), label=label, index=index).backward()
    missing = [n for n, p in t.model.backbone.named_parameters() if p.grad is None]
    assert missing == ["logit_scale"], missing
    # eval mode is as before: the same six outputs, no graph
    t.change_state(mode="valid")
    with torch.no_grad():
        e_i, h_i, e_t, h_t, _, _ = t.model(image, text)
        e_i2, h_i2 = t.model.hash.encode_img_train(t.model.get_features(image, text)[0], keep=None)
    assert torch.equal(e_i, e_i2) and torch.equal(h_i, h_i2)                         # without a mask the train forward is the eval head


def test_run_trains_validates_and_writes_the_mat_files_while_the_pinned_names_keep_raising(tmp_path):
    t = _trainer(tmp_path)
    with pytest.raises(NotImplementedError, match="backward of the decoder head"):
        t.train_epoch(0)
    with pytest.raises(NotImplementedError, match="backward of the decoder head"):
        t.train()
    with pytest.raises(NotImplementedError, match="train_epoch_decoder"):
        t.train_epoch(0)
    with pytest.raises(NotImplementedError, match="distributed"):
        type(t).from_config(cfg=t.cfg, distributed=True, autorun=False, logger=t.logger)
    assert t.global_step == 0
    t.run()                                                                          # is_train: train_decoder()
    assert t.global_step == 2 and any("FINISHED" in s for s in t.lines) and any("MAP(i->t)" in s for s in t.lines)
    assert np.isfinite(_loss_of([s for s in t.lines if "] loss: " in s][-1]))
    files = set(os.listdir(os.path.join(str(tmp_path), "mat_files")))
    assert {"i2t-best.mat", "t2i-best.mat", "i2i-best.mat", "t2t-best.mat"} <= files
    assert all(np.isfinite(v) and 0.0 <= v <= 1.0 for v in (t.max_mapi2t, t.max_mapt2i, t.max_mapi2i, t.max_mapt2t))


def test_without_fusion_the_text_head_never_receives_a_gradient(tmp_path):
    t = _trainer(tmp_path, fusion=False)
    before = {n: p.detach().clone() for n, p in t.model.hash.named_parameters()}
    t.train_epoch_decoder(0)
    for n, p in t.model.hash.named_parameters():
        if n.startswith("txt_token_hash."):
            assert torch.equal(p.detach(), before[n]) and p.grad is None, n           # encode_txt runs img_token_hash, as in the reference
        else:
            assert not torch.equal(p.detach(), before[n]), n
