"""Shared by tests/test_dimch_train_step_cpu.py and tests/test_gpu_dimch_train_step.py (not a test module): the whole training step of
DIMCHTrainer.train_epoch -- both CLIP towers with their token outputs, the image tokens with the cls row first, the token-set head of
both modalities with its dropout, the set-distance objective, the backward through all of it, BertAdam over the backbone and head
groups -- restated for S steps in the dtype it is handed, the configuration of the two cases, the conditions their inputs must meet, and
the error measure.

The restatement composes only functions that a golden file pins to the reference: oracle.encode.clip_image / clip_text with
return_patches=True over a state_dict of leaves (the projection repeated over the batch, as train_step_cases._forward feeds them; the
text call takes no key padding mask: DIMCH passes none and every one of the 32 token rows is read; the eos output is unused),
dimch_cases.head_forward (what dimch_cases.head runs) once per modality with that step's keep mask and the configuration's p,
dimch_cases.objective_terms with the constants of the configuration, and bertadam_cases.step_f64 / lr_f64.  Parameters are assigned to
their optimiser group by name (backbone.* -> backbone_lr, hash.* -> lr), never read from the trainer.  Float64 is the oracle; float32,
with the parameters stored in float32 between the steps, is the yardstick.  Every run uses one CPU thread.  Keep masks are handed in
and never drawn here (`draw_masks` replays the heads' torch.rand(...) >= p calls, image then text, after torch.manual_seed).

The cases.  Trainer settings of train_step_cases.config with DIMCHTrainer: B = 4, C = 6, train_num 12 so that three batches cycle,
max_word 32, image_resolution 64, shuffle off, optimizer {lr 0.002, backbone_lr 0.0005, e 1e-3}, epochs = S = 5, each step its own
train_epoch call on one batch, so t_total = 5 and step 0 runs at rate 0; batches 0 and 1 come round again at steps 3 and 4.  `smooth`:
one block per tower at embed_dim 64, K = 16, tanh, smooth_chamfer, setDim 3, dropout 0.3, every constant of dimch_cases.CONFIG written
out: 5 image tokens, 32 text tokens.  `softmax`: two blocks per tower at embed_dim 128, output_dim 12, so a 24-wide code that is no
multiple of 16, the pair softmax, mode chamfer (the hard maximum), setDim 8, dropout 0: no mask is drawn.

Conditions on the inputs (check_conditions; none involves the port).  Every margin is measured from the two restatements: the float64
distance of a quantity from its kink must exceed TOL_FACTOR = 4 times the largest |float32 - float64| difference of that same quantity
over the steps.  1 kinks of the objective: every hinge argument of a masked triplet with a non-zero weight, every 1 - s, and in chamfer
mode the gap between the two largest entries behind every maximum; these must also be no less than the guard of dimch_cases.guarded
(1e-5, 1e-5, 1e-4).  2 relus: every pre-activation of both relus of both heads, and the float32 run takes the float64 run's decisions
everywhere.  3 each of the four triplet terms has at least one live triplet (a summand above 1e-16, the reference's count) at every
step.  4 every batch row has a label.

Error measure.  That of train_step_cases: rel_err = max|x - f64| / max|f64| per tensor, parameters as delta = p - p_initial, pooled per
quantity and tensor kind over steps and layers (`kind_of`: tower tensors by train_step_cases.kind_of, the twelve head tensors each a
kind of its own in grad, clipped, m and v); the four head outputs as compute_loss receives them go as (codes, <name>), the nine terms
relative to the largest as (terms, '').

The delta of a head's six tensors pools into one kind per head (hash.img_token_hash, hash.txt_token_hash).  A head's biases start at
zero, so their delta is -lr m / (sqrt(v) + e) and nothing else, and a hidden unit that the relu and the dropout leave alive in one or two
of the B M = 12 rows has a gradient a hundred times below the tensor's largest: there sqrt(v) is of the size of e = 1e-3, and an error of
m that is small against max|m| is divided by it -- in the float64 run max|m| / (sqrt(v) + e) over max|u| reaches 59 for
hash.img_token_hash.hash_layer.0.bias at step 1 (2.5 to 36 for the other head tensors).  Where in the tensor a float32 run's rounding
falls then decides the delta's error, and the yardstick of one such tensor is that accident: on the inputs and masks of `smooth` two
float32 runs of this very restatement on two CPUs give, for the delta of hash.img_token_hash.hash_layer.0.bias, 2.15e-5 and 8.95e-6 (a
factor of 2.4; the port's 3.93e-5 is 1.8 times the one and 4.4 times the other, with its grad, clipped, m and v of that tensor between
1.1 and 1.5 times their yardsticks), for hash.txt_token_hash.hash_layer.0.bias 5.4e-6 and 1.09e-5, and in `softmax` for
hash.txt_token_hash.hash_layer.3.bias 4.2e-6 and 1.6e-6.  A yardstick that uncertain cannot carry a factor of 4.  Pooled over the six
tensors of a head it is set by a weight matrix (2.45e-5 and 2.45e-5 for the image head, 1.95e-5 and 2.39e-5 for the text head in those
two runs) and moves by 1.2 at most; the factor stays 4."""
import numpy as np
import torch

import bertadam_cases as AC
import dimch_cases as DM
import train_step_cases as TS
from oracle import encode as enc

STEPS = TS.STEPS
DATA_SEED = 1828                     # the dataset's seed: the first from 1814 on that meets the conditions of both cases (see
                                     # tests/test_dimch_train_step_cpu.py for what 1814 to 1827 missed)
MASK_SEED = 1814                     # torch.manual_seed(MASK_SEED + s) before step s
B, C, TRAIN_NUM = 4, 6, 12
OPT_CFG = TS.OPT_CFG
ADAM = TS.ADAM
TOL_FACTOR = 4.0
NULL_G = TS.NULL_G
QUANTITIES = TS.QUANTITIES
MODS = ("img", "txt")
TERMS = DM.TERMS
OUTS = ("img_embeds", "img_hash", "txt_embeds", "txt_hash")
GUARD = {"hinge": 1e-5, "one_minus_s": 1e-5, "gap": 1e-4}          # dimch_cases.guarded's
_CLIP = "vision_layers=%d,transformer_layers=%d,vision_width=128,transformer_width=128,embed_dim=%d,image_resolution=64"
CASES = {
    "smooth": dict(clip=_CLIP % (1, 1, 64), K=16, setDim=3, dropout=0.3,
                   consts=dict(mode="smooth_chamfer", denominator=2.0, temperature=16.0, temperature_txt_scale=1.0, token_triplet_margin=0.3,
                               triplet_margin=0.3, mmd_gamma=0.5, triplet_alpha=50.0, mmd_alpha=1.0, unif_alpha=0.3, hash_triplet_alpha=50.0,
                               quan_alpha=1.0, hash_func="tanh")),
    "softmax": dict(clip=_CLIP % (2, 2, 128), K=12, setDim=8, dropout=0.0,
                    consts=dict(mode="chamfer", denominator=2.0, temperature=16.0, temperature_txt_scale=1.0, token_triplet_margin=0.3,
                                triplet_margin=0.3, mmd_gamma=0.5, triplet_alpha=50.0, mmd_alpha=1.0, unif_alpha=0.3, hash_triplet_alpha=50.0,
                                quan_alpha=1.0, hash_func="softmax")),
}
rel_err = AC.rel_err
Rows, pack, dense = TS.Rows, TS.pack, TS.dense
table = TS.table
assert CASES["smooth"]["consts"] == DM.CONFIG


# ---- configuration ------------------------------------------------------------------------------------------------------------
def config(case, out_dir, device, data_seed=DATA_SEED):
    c = CASES[case]
    k = c["consts"]
    return {
        "model": {"arch": "DIMCH", "clip_path": "synthetic:1814:" + c["clip"], "setDim": c["setDim"], "dropout": c["dropout"],
                  "hash_func": k["hash_func"], "merge_func": "mean", "seed": 1814,
                  "distance": {n: k[n] for n in ("mode", "denominator", "temperature", "temperature_txt_scale")},
                  "chamfer": {n: k[n] for n in ("mmd_gamma", "mmd_alpha", "unif_alpha", "token_triplet_margin")},
                  "hash_pars": {n: k[n] for n in ("triplet_alpha", "quan_alpha", "hash_triplet_alpha", "triplet_margin")}},
        "dataset": {"arch": "synthetic", "name": "synth", "num_classes": C, "retrieval_num": 16, "max_word": 32, "image_resolution": 64,
                    "seed": data_seed},
        "optimizer": dict(OPT_CFG),
        "run": {"arch": "DIMCHTrainer", "output_dim": c["K"], "device": device, "batch_size": B, "num_workers": 0, "is_train": True,
                "query_num": 8, "train_num": TRAIN_NUM, "epochs": STEPS, "shuffle": False, "save_dir": str(out_dir), "log_dir": str(out_dir),
                "seed": 1814},
    }


def trainer(case, out_dir, device, data_seed=DATA_SEED):
    """the runner of a case, its log lines collected in `.lines`"""
    import types
    import xmh.models  # noqa: F401
    import xmh.runners  # noqa: F401
    from xmh.common.register import registry
    from xmh.utils.config import Config
    t = registry.get_runner_class("DIMCHTrainer").from_config(cfg=Config(config(case, out_dir, device, data_seed)), autorun=False)
    t.lines = []
    t.logger = types.SimpleNamespace(info=t.lines.append)
    return t


def capture(t, case):
    """everything the restatement needs of a trainer, on the CPU: dict(case, sd0: the parameters by name, raw: the loader's batches as it
    yields them, consts / p: of the configuration, M, H: the set size and the hidden width of the heads, T: token rows per modality)"""
    c = CASES[case]
    sd0 = {n: p.detach().cpu().clone() for n, p in t.model.named_parameters()}
    raw = list(t.train_loader)
    assert len(raw) == TRAIN_NUM // B == 3
    for image, ids, kpm, label, index in raw:
        assert image.shape == (B, 3, 64, 64) and ids.shape == (B, 32) and label.shape == (B, C) and index.shape == (B,)
    assert sorted(int(i) for b in raw for i in b[4]) == list(range(TRAIN_NUM))
    width = c["K"] * (2 if c["consts"]["hash_func"] == "softmax" else 1)
    T = {}
    for mod in MODS:
        w, w1, w2 = (sd0["hash." + DM.HEAD_KEYS[k] % mod] for k in ("conv_w", "w1", "w2"))
        assert w.shape[0] == c["setDim"] and w2.shape[0] == width and w1.shape[0] == w1.shape[1] // 2
        T[mod] = w.shape[1]
        assert float(getattr(t.model.hash, mod + "_token_hash").dropout_p) == c["dropout"]
    assert T == {"img": 5, "txt": 32}
    assert sum(n.startswith("hash.") for n in sd0) == 12
    return dict(case=case, sd0=sd0, raw=raw, consts=dict(c["consts"]), p=c["dropout"], M=c["setDim"], H=int(w1.shape[0]), T=T)


def kind_of(name, quantity=None):
    """tensor kind for pooling: train_step_cases.kind_of, but the delta of a head's tensors as one kind per head (the module's docstring)"""
    if quantity == "delta" and name.startswith("hash."):
        return ".".join(name.split(".")[:2])
    return TS.kind_of(name)


def pool(per_step):
    """list over steps of `errors` -> {(quantity, kind): the largest over the steps, the layers and, for a head's delta, its tensors}"""
    out = {}
    for errs in per_step:
        for (q, name), e in errs.items():
            key = (q, kind_of(name, q) if name else "")
            out[key] = max(out.get(key, 0.0), e)
    return out


def group_of(name):
    assert name.startswith("backbone.") or name.startswith("hash."), name
    return "backbone" if name.startswith("backbone.") else "hash"


def hyper_of(name):
    return dict(ADAM, lr=OPT_CFG["backbone_lr" if group_of(name) == "backbone" else "lr"])


def draw_masks(cap, device="cpu", steps=STEPS, seed=MASK_SEED):
    """per step (keep_img, keep_txt), uint8 [B M, H] on the CPU, or None for a case without dropout: the heads' own
    torch.rand(B M, H, device=device) >= p calls, image then text, after torch.manual_seed(seed + s)"""
    if cap["p"] <= 0.0:
        return None
    out = []
    for s in range(steps):
        torch.manual_seed(seed + s)
        out.append(tuple((torch.rand(B * cap["M"], cap["H"], device=device) >= cap["p"]).cpu().to(torch.uint8) for _ in MODS))
    return out


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def run(cap, masks, steps=STEPS, dtype=torch.float64, keep=None):
    """S training steps from cap["sd0"] on cap["raw"][s % 3] in `dtype`.  masks: per step (keep_img, keep_txt) [B M, H] of 0 / 1, or
    None (no dropout).  -> list over the steps of `keep(s, record)` (the record itself without `keep`); a record holds, per parameter
    name, numpy arrays of `dtype`:
      grad (before clipping), clipped (what BertAdam leaves in p.grad), p (after the step), m, v (next_m / next_v),
    and loss, terms (the nine of dimch_cases.TERMS), lr (the rate each group stepped with), next_lr (what get_lr() reports afterwards),
    count (BertAdam's step counter), outs (the four head outputs in compute_loss's order, detached), pre (per modality the
    pre-activations of the two relus, float64 numpy), trace (dimch_cases' probe trace: every hinge argument, 1 - s, gap, live count),
    labels, buffers (none)."""
    npd = np.float64 if dtype == torch.float64 else np.float32
    cst, out = cap["consts"], []
    with TS.DC.one_thread():
        t = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in cap["sd0"].items()}
        head = {mod: {k: t["hash." + DM.HEAD_KEYS[k] % mod] for k in DM.HEAD_PARAMS} for mod in MODS}
        m = {k: np.zeros(tuple(x.shape), npd) for k, x in t.items()}
        v = {k: np.zeros(tuple(x.shape), npd) for k, x in t.items()}
        for s in range(steps):
            image, ids, _, label, _ = cap["raw"][s % len(cap["raw"])]
            for x in t.values():
                x.grad = None
            clip = {k[len("backbone."):]: x for k, x in t.items() if k.startswith("backbone.")}
            fed = dict(clip, **{k: clip[k].unsqueeze(0).repeat(image.shape[0], 1, 1) for k in ("visual.proj", "text_projection")})
            cls_i, tok_i = enc.clip_image(fed, image.to(dtype), return_patches=True)
            _, tok_t, _ = enc.clip_text(fed, ids, None, return_patches=True)
            tokens = {"img": torch.cat([cls_i.unsqueeze(1), tok_i.permute(1, 0, 2)], dim=1), "txt": tok_t.permute(1, 0, 2)}
            assert tuple(tokens["img"].shape[:2]) == (B, cap["T"]["img"]) and tuple(tokens["txt"].shape[:2]) == (B, cap["T"]["txt"])
            o, pre = {}, {}
            for i, mod in enumerate(MODS):
                km = None if masks is None else torch.as_tensor(masks[s][i]).to(dtype)
                o[mod + "_embeds"], o[mod + "_hash"], c_pre, a_pre = DM.head_forward(tokens[mod], head[mod], km, cap["p"], cst["hash_func"])
                pre[mod] = (c_pre.detach().double().numpy().copy(), a_pre.detach().double().numpy().copy())
            probe = {"trace": {}}
            terms = DM.objective_terms(o["img_embeds"], o["txt_embeds"], o["img_hash"], o["txt_hash"], torch.as_tensor(label), cst, probe)
            terms[0].backward()
            rec = {"loss": float(terms[0].detach()), "terms": terms.detach().double().numpy().copy(), "outs": [o[k].detach().numpy().copy() for k in OUTS],
                   "pre": pre, "trace": probe["trace"], "labels": np.asarray(label).copy(), "lr": {}, "next_lr": {}, "count": s + 1, "buffers": {}}
            for kind in QUANTITIES[:2] + ("p",) + QUANTITIES[3:]:
                rec[kind] = {}
            for k, x in t.items():
                if x.grad is None:
                    continue
                h = hyper_of(k)
                lr = AC.lr_f64(h, s)
                rec["lr"][group_of(k)], rec["next_lr"][group_of(k)] = lr, AC.lr_f64(h, s + 1)
                g = x.grad.numpy().copy()
                p, m[k], v[k], gc = AC.step_f64(x.detach().numpy(), g, m[k], v[k], lr, h)
                assert p.dtype == m[k].dtype == v[k].dtype == npd
                with torch.no_grad():
                    x.copy_(torch.from_numpy(p))
                rec["grad"][k], rec["clipped"][k], rec["p"][k] = pack(g), pack(np.asarray(gc)), p
                rec["m"][k], rec["v"][k] = pack(m[k].copy()), pack(v[k].copy())
            out.append(rec if keep is None else keep(s, rec))
    return out


# ---- conditions, sets, errors -------------------------------------------------------------------------------------------------
def _margin_noise(a64, a32):
    """two lists of arrays (NaN: not looked at) -> (smallest |float64|, largest |float32 - float64|)"""
    margin, noise = np.inf, 0.0
    for a, b in zip(a64, a32):
        assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b))
        if np.isfinite(a).any():
            margin, noise = min(margin, float(np.nanmin(np.abs(a)))), max(noise, float(np.nanmax(np.abs(b - a))))
    return margin, noise


def check_conditions(cap, r64, r32):
    """the conditions on the inputs, asserted on the float64 run (r32: the float32 run on the same masks) -> what was measured:
    kink name -> (margin, noise) over the run (hinge, one_minus_s, gap where the mode has maxima, relu_c / relu_a per modality),
    (step, 'live') -> the four live counts, (step, 'relu') -> decisions that differ in float32, (step, 'labels') -> labels per row"""
    out = {}
    kinks = ["hinge", "one_minus_s"] + (["gap"] if "gap" in r64[0]["trace"] else [])
    assert ("gap" in kinks) == ("chamfer" in cap["consts"]["mode"] and "smooth" not in cap["consts"]["mode"])
    for k in kinks:
        out[k] = _margin_noise([a for r in r64 for a in r["trace"][k]], [a for r in r32 for a in r["trace"][k]])
    for mod in MODS:
        for i, name in enumerate(("relu_c", "relu_a")):
            out["%s_%s" % (name, mod)] = _margin_noise([r["pre"][mod][i] for r in r64], [r["pre"][mod][i] for r in r32])
    for s, (a, b) in enumerate(zip(r64, r32)):
        live = [int(x) for x in a["trace"]["live"]]
        out[(s, "live")] = live
        assert len(live) == 4 and min(live) >= 1, ("a triplet term without a live triplet", s, live)
        assert len(a["trace"]["hinge"]) == 4 and len(a["trace"]["one_minus_s"]) == 1
        out[(s, "relu")] = sum(int(((x > 0) != (y > 0)).sum()) for mod in MODS for x, y in zip(a["pre"][mod], b["pre"][mod]))
        assert out[(s, "relu")] == 0, ("the float32 restatement takes another relu decision", s, out[(s, "relu")])
        out[(s, "labels")] = a["labels"].sum(1).astype(int).tolist()
        assert a["labels"].shape == (B, C) and min(out[(s, "labels")]) >= 1, ("a batch row without a label", s)
    for k, (margin, noise) in [(k, v) for k, v in out.items() if isinstance(k, str)]:
        assert margin > TOL_FACTOR * noise, ("a kink within TOL_FACTOR float32 differences", k, margin, noise)
        assert margin >= GUARD.get(k, 0.0), ("a kink inside dimch_cases' guard", k, margin, GUARD[k])
    return out


def condition_lines(what, cond):
    lines = []
    for key, v in cond.items():
        if isinstance(key, str):
            lines.append("%s condition %-12s margin %.3e  noise %.3e  ratio %.1f  guard %.0e" % (what, key, v[0], v[1], v[0] / v[1] if v[1] else np.inf,
                                                                                             GUARD.get(key, 0.0)))
        else:
            lines.append("%s condition step %d %s %s" % (what, key[0], key[1], v))
    return lines


def no_grad_set(cap, r64):
    return tuple(sorted(set(cap["sd0"]) - set(r64[0]["grad"])))


def null_set(r64):
    return tuple(sorted(k for k in r64[0]["grad"] if all(float(np.abs(dense(rec["grad"][k])).max()) < NULL_G for rec in r64)))


quantity = TS.quantity


def errors(rec, ref, sd0, null=()):
    """train_step_cases.errors and, on top, the nine terms relative to the largest as (terms, '') and the four head outputs as
    (codes, <name>)"""
    out = TS.errors(rec, ref, sd0, null)
    out[("terms", "")] = rel_err(rec["terms"], ref["terms"])
    for name, a, b in zip(OUTS, rec["outs"], ref["outs"]):
        out[("codes", name)] = rel_err(a, b)
    return out


def yardstick(cap, r64, r32, null=()):
    """the float32 restatement against the float64 one on these very inputs and masks -> (per-step `errors`, their pool, per step the
    float32 run's max|g| of every null tensor)"""
    per = [errors(b, a, cap["sd0"], null) for a, b in zip(r64, r32)]
    return per, pool(per), [{n: float(np.abs(dense(b["grad"][n])).max()) for n in null} for b in r32]
