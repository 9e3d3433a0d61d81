"""GPU: UMoED evaluated end to end: UMoEDTrainer.valid() on the synthetic dataset over a tiny synthetic backbone (5 image
tokens, 32 text tokens, E = 64) with setDim 4, output_dim 4 (V = 2), one decoder layer of one head and 2 x 2 experts -- both towers' token
outputs, the soft-MoE decoder head, the packed scan for four mAPs, four .mat files with the fusion stream."""
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SMALL = "synthetic:1814:vision_layers=1,transformer_layers=1,vision_width=128,transformer_width=128,embed_dim=64,image_resolution=64"


def _trainer(tmp_path, lines=None, **run):
    import xmh.models  # noqa: F401
    import xmh.runners  # noqa: F401
    from xmh.common.register import registry
    from xmh.utils.config import Config
    cfg = Config({
        "model": {"arch": "UMoED", "clip_path": SMALL, "setDim": 4, "dropout": 0.3, "extreme": True, "extreme_T": 0.3, "triplet": True,
                  "distance_mode": "cosine", "MoE": True, "fusion": True, "num_experts": 2, "slots_per_expert": 2, "hash_func": "linear_subspace",
                  "merge_func": "concatenate", "decoder_heads": 1, "decoder_layers": 1, "hidden_dim": 64, "seed": 1814,
                  "distance": {"mode": "pairwise"}, "chamfer": {"unif_alpha": 0.8, "token_triplet_margin": 0.1},
                  "hash_pars": {"triplet_alpha": 1, "triplet_margin": 0.3}},
        "dataset": {"arch": "synthetic", "name": "synth", "num_classes": 6, "retrieval_num": 16, "max_word": 32, "image_resolution": 64},
        "optimizer": {"lr": 0.001, "backbone_lr": 0.00001},
        "run": dict({"arch": "UMoEDTrainer", "output_dim": 4, "device": 0, "batch_size": 4, "num_workers": 0, "is_train": False, "query_num": 8,
                     "train_num": 8, "epochs": 1, "save_dir": str(tmp_path), "log_dir": str(tmp_path), "seed": 1814}, **run),
    })
    lines = [] if lines is None else lines
    t = registry.get_runner_class("UMoEDTrainer").from_config(cfg=cfg, autorun=False, logger=types.SimpleNamespace(info=lines.append))
    t.lines = lines
    return t


def test_valid_reports_four_maps_and_writes_four_mat_files(tmp_path):
    import scipy.io as scio
    from oracle import retrieval as O
    t = _trainer(tmp_path)
    assert t.hash_scale == 1 and t.model.hash.hash_module.code_width == 4
    maps = t.valid(0, k=t.top_k)
    assert len(maps) == 4 and all(np.isfinite(v) and 0.0 <= v <= 1.0 for v in maps) and max(maps) > 0.0
    line = [s for s in t.lines if "MAP(i->t)" in s][-1]
    for tag in ("MAP(i->t): ", "MAP(t->i): ", "MAP(t->t): ", "MAP(i->i): ", "MAX MAP(i->i): ", "MAX MAP(t->t): "):
        assert tag in line, line
    assert (t.max_mapi2t, t.max_mapt2i, t.max_mapi2i, t.max_mapt2t) == tuple(maps)
    assert (t.best_epoch_i2t, t.best_epoch_t2i, t.best_epoch_i2i, t.best_epoch_t2t) == (0, 0, 0, 0)
    # the codes: get_code's three streams, the fusion one all zero; the head called directly gives the same image codes
    q_img, q_txt, q_fus = t.get_code(t.query_loader, t.query_num)
    r_img, r_txt, r_fus = t.get_code(t.retrieval_loader, t.retrieval_num)
    assert tuple(q_img.shape) == (8, 4) and tuple(r_txt.shape) == (16, 4) and set(q_img.unique().tolist()) <= {-1.0, 1.0}
    assert float(q_fus.abs().max()) == 0 and float(r_fus.abs().max()) == 0 and q_fus.shape == q_img.shape
    image, text, _, _, index = next(iter(t.query_loader))
    with torch.no_grad():
        tokens_i, tokens_t = t.model.get_features(image.cuda(), text.cuda())
        e_i, h_i = t.model.hash.encode_img(tokens_i)
        e_t, h_t = t.model.hash.encode_txt(tokens_t)
        out = t.model(image.cuda(), text.cuda())
    assert tuple(tokens_i.shape) == (4, 5, 64) and tuple(tokens_t.shape) == (4, 32, 64) and tuple(e_i.shape) == (4, 4, 2)
    assert torch.equal(q_img[index.cuda()], h_i) and torch.equal(q_txt[index.cuda()], h_t)
    assert len(out) == 6 and out[4] is None and out[5] is None and torch.equal(out[1], h_i) and torch.equal(out[2], e_t)
    assert torch.equal(h_i > 0, e_i[..., 1] > e_i[..., 0])                           # V = 2: bit m is +1 iff logit 1 beats logit 0
    a, b, f = t.generate_hash(image.cuda(), text.cuda())
    assert torch.equal(a, h_i) and torch.equal(b, h_t) and f is None
    # i -> i through the oracle's map_k (the reference's calc_map_k) on the same codes
    want = float(O.map_k(q_img.cpu(), r_img.cpu(), t.query_labels, t.retrieval_labels, t.top_k))
    assert abs(maps[2] - want) <= 1e-6, (maps[2], want)
    want_i2t = float(O.map_k(q_img.cpu(), r_txt.cpu(), t.query_labels, t.retrieval_labels, t.top_k))
    assert abs(maps[0] - want_i2t) <= 1e-6
    # four files, eight keys each
    files = set(os.listdir(os.path.join(str(tmp_path), "mat_files")))
    assert {"i2t-best.mat", "t2i-best.mat", "i2i-best.mat", "t2t-best.mat"} <= files
    for name in ("i2t", "t2i", "i2i", "t2t"):
        m = scio.loadmat(os.path.join(str(tmp_path), "mat_files", name + "-best.mat"))
        assert {"q_img", "q_txt", "q_fus", "r_img", "r_txt", "r_fus", "q_l", "r_l"} <= set(m)
        assert m["q_img"].shape == (8, 4) and m["r_fus"].shape == (16, 4) and m["q_l"].shape == (8, 6) and m["r_l"].shape == (16, 6)
        assert not m["q_fus"].any() and not m["r_fus"].any()
        assert np.array_equal(m["q_img"], q_img.cpu().numpy()) and np.array_equal(m["r_txt"], r_txt.cpu().numpy())
    # a second epoch that is no better keeps the first epoch's bests
    again = t.valid(1, k=t.top_k)
    assert tuple(again) == tuple(maps) and t.best_epoch_i2i == 0


def test_train_epoch_says_what_is_missing_and_the_objective_backpropagates(tmp_path):
    t = _trainer(tmp_path)
    with pytest.raises(NotImplementedError, match="backward of the decoder head"):
        t.train_epoch(0)
    with pytest.raises(NotImplementedError, match="backward of the decoder head"):
        t.train()                                                                    # the reference's loop: it raises at once
    with pytest.raises(NotImplementedError, match="distributed"):
        type(t).from_config(cfg=t.cfg, distributed=True, autorun=False, logger=t.logger)
    image, text, _, label, index = next(iter(t.query_loader))
    t.change_state(mode="valid")
    with torch.no_grad():
        e_i, h_i, e_t, h_t, _, _ = t.model(image.cuda(), text.cuda())
    e_i, e_t = e_i.requires_grad_(True), e_t.requires_grad_(True)
    loss = t.compute_loss(img_embeds=e_i, img_hash=h_i, txt_embeds=e_t, txt_hash=h_t, label=label, index=index)
    loss.backward()
    assert np.isfinite(float(loss.detach())) and e_i.grad is not None and e_t.grad is not None
    assert bool(torch.isfinite(e_i.grad).all()) and float(e_i.grad.abs().max()) > 0 and float(e_t.grad.abs().max()) > 0
    _, d = t.model.object_function(e_i.detach(), h_i, e_t.detach(), h_t, labels=label)
    assert set(d["Tokens"]["Similarity"]) == {"i2t", "t2i", "it2i", "it2t", "All"} and set(d["Tokens"]["Diversity"]) == {"i", "t", "it", "All"}
    assert float(d["All loss"]) == float(loss.detach())
