"""GPU: MITH trained end to end: MITH.forward_train_towers composes the towers' token outputs
(CLIP.encode_image_train_tokens / encode_text_train_tokens), the hash head (encode_img_train / encode_txt_train) and the loss
(MITHTrainer.compute_loss) into one graph; MITHTrainer.train_epoch_towers is the reference's epoch (runners/MITH/runner.py:98-123)
and MITHTrainer.train() runs it.

Each stage is pinned to float64 on its own (tests/test_gpu_tower_tokens.py, test_gpu_mith_head_grad.py, test_gpu_mith_loss.py);
what the chain adds is checked here as bit equality of the one-graph backward with the staged one."""
import re
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SMALL = "synthetic:1814:vision_layers=1,transformer_layers=1,vision_width=128,transformer_width=128,embed_dim=64,image_resolution=64"
LOSS = r"loss: (?:tensor\()?([-+0-9.eE]+|nan|inf)"


def _trainer(tmp_path, **run):
    import xmh.models  # noqa: F401
    import xmh.runners  # noqa: F401
    from xmh.common.register import registry
    from xmh.utils.config import Config
    cfg = Config({
        "model": {"arch": "MITH", "clip_path": SMALL, "transformer_layers": 1, "res_mlp_layers": 1, "top_k_label": 4, "hash_func": "tanh"},
        "dataset": {"arch": "synthetic", "name": "synth", "num_classes": 6, "retrieval_num": 16, "max_word": 32, "image_resolution": 64},
        "optimizer": {"lr": 0.001, "backbone_lr": 0.00001},
        "run": dict({"arch": "MITHTrainer", "output_dim": 16, "device": 0, "batch_size": 4, "num_workers": 0, "is_train": True, "query_num": 8,
                     "train_num": 8, "epochs": 1, "save_dir": str(tmp_path), "log_dir": str(tmp_path), "seed": 1814}, **run),
    })
    t = registry.get_runner_class("MITHTrainer").from_config(cfg=cfg, autorun=False)
    t.lines = []
    t.logger = types.SimpleNamespace(info=t.lines.append)
    return t


def _batch(t):
    image, text, kpm, label, index = next(iter(t.train_loader))
    return image.cuda(), text.cuda(), kpm.cuda(), label, index.numpy()


# 9 composition ---------------------------------------------------------------------------------------------------------------------
def test_backbone_gradients_compose_with_the_head_and_the_loss(tmp_path):
    t = _trainer(tmp_path)
    model = t.model.train()
    image, text, kpm, label, index = _batch(t)
    watched = dict(model.named_parameters())
    assert any(n.startswith("backbone.visual.") for n in watched) and any(n.startswith("hash.") for n in watched)

    def grads():
        out = {n: None if p.grad is None else p.grad.clone() for n, p in watched.items()}
        model.zero_grad(set_to_none=True)
        return out
    buffer0 = model.img_buffer_cls.clone()
    outs = model.forward_train_towers(image, text, key_padding_mask=kpm)
    assert len(outs) == 8 and all(o.requires_grad for o in outs)
    with torch.no_grad():                                                        # the eight tensors of forward, in the order of forward_train_heads
        assert [tuple(o.shape) for o in outs] == [tuple(o.shape) for o in model.forward_train_heads(image, text, key_padding_mask=kpm)]
    loss = t.compute_loss(*outs, label=label, index=index, epoch=0, times=1, global_step=1)
    loss.backward()
    one = grads()
    assert one["backbone.logit_scale"] is None
    for n, v in one.items():
        if n != "backbone.logit_scale":
            assert v is not None and bool(torch.isfinite(v).all()), n
    assert any(bool(v.any()) for n, v in one.items() if n.startswith("backbone.visual.")) and bool(one["backbone.token_embedding.weight"].any())

    # staged: tower outputs detached into leaves, head + loss backward to the leaves, then the towers' backward from the leaves' gradients
    model._bind_buffer(buffer0.clone())
    cls_i, tok_i = model.backbone.encode_image_train_tokens(image)
    eos_t, tok_t, new_mask = model.backbone.encode_text_train_tokens(text, key_padding_mask=kpm)
    stage = [cls_i, tok_i, eos_t, tok_t]
    leaves = [y.detach().requires_grad_(True) for y in stage]
    outs2 = (*model.hash.encode_img_train(leaves[0], leaves[1]), *model.hash.encode_txt_train(leaves[2], leaves[3], new_mask))
    loss2 = t.compute_loss(*outs2, label=label, index=index, epoch=0, times=1, global_step=1)
    assert torch.equal(loss2.detach(), loss.detach())
    loss2.backward()
    assert all(leaf.grad is not None for leaf in leaves)
    head = {n: p.grad.clone() for n, p in watched.items() if n.startswith("hash.")}
    assert all(p.grad is None for n, p in watched.items() if n.startswith("backbone."))
    for p in model.hash.parameters():
        p.grad = None
    torch.autograd.backward(stage, [leaf.grad for leaf in leaves])
    two = grads()
    two.update(head)
    for n in one:
        assert (one[n] is None) == (two[n] is None) and (one[n] is None or torch.equal(one[n], two[n])), n


# 10 train_epoch_towers -------------------------------------------------------------------------------------------------------------
def test_train_epoch_towers_moves_every_parameter_and_repeats_to_the_bit(tmp_path):
    finals = []
    for _ in range(2):
        t = _trainer(tmp_path)
        before = {n: p.detach().clone() for n, p in t.model.named_parameters()}
        assert getattr(t, "optimizer", None) is None
        seen = []
        real = t.compute_loss

        def recording(*a, **k):
            seen.append((a[6].detach().clone(), np.asarray(k["index"]).copy()))      # tokens_hash_t and the batch's rows
            return real(*a, **k)
        t.compute_loss = recording
        t.train_epoch_towers(0)
        steps = len(t.train_loader)
        assert steps == 2 and t.global_step == steps and len(seen) == steps
        line = t.lines[-1]
        loss = float(re.search(LOSS, line).group(1))
        print(line)
        assert np.isfinite(loss) and "lr: " in line
        for n, p in t.model.named_parameters():
            if n == "backbone.logit_scale":
                assert torch.equal(p.detach(), before[n]) and p.grad is None
            else:
                assert n.startswith("backbone.") or n.startswith("hash."), n
                assert not torch.equal(p.detach(), before[n]), n
                assert bool(torch.isfinite(p).all()), n
                assert t.optimizer.state[p]["step"] == steps, n
        tokens_hash_t, rows = seen[-1]
        assert torch.equal(t.model.img_buffer_cls[torch.as_tensor(rows).cuda()], tokens_hash_t.to(t.model.img_buffer_cls.dtype))
        finals.append({n: p.detach().clone() for n, p in t.model.named_parameters()})
    assert all(torch.equal(finals[0][n], finals[1][n]) for n in finals[0])


# 11 train() ----------------------------------------------------------------------------------------------------------------------
def test_train_runs_to_the_end_and_distributed_raises(tmp_path):
    t = _trainer(tmp_path)
    t.train()                                                                    # train_epoch_towers and valid for each epoch
    assert any("FINISHED" in line for line in t.lines) and t.global_step == len(t.train_loader)
    t.distributed = True
    with pytest.raises(NotImplementedError, match="all-reduce"):
        t.train_epoch_towers(0)
    with pytest.raises(NotImplementedError, match="MITH's head"):
        t.train_epoch(0)


def test_ten_epochs_on_one_batch_give_finite_losses(tmp_path):
    """Whether the objective falls at these rates (lr 1e-3, backbone 1e-5, ten warm-up-cosine steps) has not been established, so only
    finiteness is asserted; the ten losses are printed."""
    t = _trainer(tmp_path, epochs=10)
    t.train_loader = [next(iter(t.train_loader))]                                # one fixed batch per epoch
    losses = []
    for epoch in range(10):
        t.train_epoch_towers(epoch)
        losses.append(float(re.search(LOSS, t.lines[-1]).group(1)))
    print("losses", " ".join("%.6f" % v for v in losses))
    assert len(losses) == 10 and all(np.isfinite(losses))
