"""Shared by tests/test_mith_train_step_cpu.py and tests/test_gpu_mith_train_step.py (not a test module): the whole training step of
MITHTrainer.train_epoch_towers -- both CLIP towers with their token outputs, the hash head of both modalities over the shared
GlobalConceptLearning, the rolling buffer's row write, the objective, the backward through all of it, BertAdam over the backbone and
head groups -- restated for S steps in the dtype it is handed, the configuration of the two cases, the conditions their inputs must
meet, and the error measure.

The restatement composes only functions that a golden file pins to the reference: oracle.encode.clip_image / clip_text with
return_patches=True over a state_dict of leaves (the projection repeated over the batch, as train_step_cases._forward feeds them; the
text call takes the loader's key padding mask and returns new_mask), mith_head_grad_cases.head_outputs once per modality (the
parameters under hash.gcl_i.* are the same leaves in both calls), oracle.losses.mith_terms with the model's seven weights, and
bertadam_cases.step_f64 / lr_f64.  The buffer Y starts as model.img_buffer_cls, is kept in `dtype`, and has the batch's rows
overwritten with the detached tokens_hash_t before the loss; label_sim = (train_labels @ label.T > 0), [train_num, B].  Parameters are
assigned to their optimiser group by name (backbone.* -> backbone_lr, hash.* -> lr), never read from the trainer.  Float64 is the
oracle; float32, with the parameters stored in float32 between the steps, is the yardstick.  Every run uses one CPU thread.

The K one-row layers hash.lct_*.hashing.fc_list.<k> are K parameters each and BertAdam clips them one by one; a record holds them
stacked to [K, D] / [K] under the name hash.lct_*.hashing.fc_list.weight / .bias (`record_key`), because a single scalar's relative
error is cancellation noise (on a one-scalar bias float32 gives up to 1.1e-4 on the gradient and 1.5e-3 on the delta).

The cases.  Trainer settings of train_step_cases.config with MITHTrainer: B = 4, C = 6, train_num 12 so that three batches cycle,
max_word 32, image_resolution 64, shuffle off, dataset seed 1814, optimizer {lr 0.002, backbone_lr 0.0005, e 1e-3}, epochs = S = 5,
each step its own train_epoch_towers call on one batch, so t_total = 5 and step 0 runs at rate 0.  `narrow`: two blocks per tower at
embed_dim 64, head K = 16 with one block, one residual MLP, top_k 4.  `wide`: one block per tower at embed_dim 128 (two attention
heads in the head's transformer), K = 24 (no multiple of 16), two head blocks, two residual MLPs, top_k 8.  4 image tokens and 32
text tokens per sample; batches 0 and 1 come round a second time at steps 3 and 4, when their buffer rows hold an earlier step's
tokens_hash_t; batch 2 is seen once; rows 4 to 11 of the buffer are untouched at step 0.

Conditions on the inputs (check_conditions; none involves the port).  1 clamp: max|Y[n] . x| over the four codes stays below
64 - mith_loss_cases.GAP at every step.  2 keep-set: the LTA selection is discontinuous, so the float32 restatement with its own
selection must choose exactly the float64 run's keep-set at every step and modality, and the smallest finite margin of the float64
run must exceed TOL_FACTOR times the largest |scores32 - scores64| over the unmasked entries and the steps.  3 empty concepts: at
least one (sample, concept) pair without a kept token at every step in each modality (the NaN -> 0 route of the aggregation).

Error measure.  That of train_step_cases: rel_err = max|x - f64| / max|f64| per tensor, parameters as delta = p - p_initial, pooled
per quantity and tensor kind over steps and layers.  Tower tensors pool by train_step_cases.kind_of, head tensors by
mith_head_grad_cases.kind_of with an i. / t. / gcl. prefix; the buffer's rows written so far go as (buffer, Y).

The one-row hashing layers of the two modalities pool into one kind (lct.g_hash_w, lct.g_hash_b).  Their K rows are clipped one by
one, so every row with a norm above 1 leaves the clip at norm 1, whatever it was before: the stacking that hides a small row's
cancellation noise (a row is a sum over the B = 4 samples) in `grad` is undone in `clipped`, m, v and delta.  In the float64 run the
row norms of one stacked tensor span 0.47 to 8.8; the float32 restatement's error is 8e-7 on the stacked gradient and up to 7.9e-6
on its smallest row, its largest delta error sits in the row of the smallest norm, and the yardstick of one modality -- the largest
of 16 rows times 5 steps of that noise -- differs by a factor of 2.2 between two float32 runs of this very restatement on two CPUs
(clipped, text: 5.0e-6 and 2.3e-6; delta, text: 8.2e-6 and 3.8e-6).  A yardstick that uncertain cannot carry a factor of 4; pooled
over the 2 K rows of both modalities it is the larger of the two and moves by 1.4 between those runs."""
import numpy as np
import torch

import bertadam_cases as AC
import mith_head_grad_cases as MC
import mith_loss_cases as ML
import train_step_cases as TS
from oracle import encode as enc
from oracle import losses as OL

STEPS = TS.STEPS
DATA_SEED = 1814                     # the dataset's seed: the first from 1814 on that meets the conditions of both cases
B, C, TRAIN_NUM = 4, 6, 12
OPT_CFG = TS.OPT_CFG
ADAM = TS.ADAM
GAP = ML.GAP
TOL_FACTOR = 4.0
NULL_G = TS.NULL_G
QUANTITIES = TS.QUANTITIES
MODS = ("i", "t")
TERMS = OL.MITH_TERMS
_CLIP = "vision_layers=%d,transformer_layers=%d,vision_width=128,transformer_width=128,embed_dim=%d,image_resolution=64"
CASES = {
    "narrow": dict(clip=_CLIP % (2, 2, 64), K=16, head={"transformer_layers": 1, "res_mlp_layers": 1, "top_k_label": 4}),
    "wide": dict(clip=_CLIP % (1, 1, 128), K=24, head={"transformer_layers": 2, "res_mlp_layers": 2, "top_k_label": 8}),
}
rel_err = AC.rel_err
Rows, pack, dense = TS.Rows, TS.pack, TS.dense


# ---- configuration ------------------------------------------------------------------------------------------------------------
def config(case, out_dir, device, data_seed=DATA_SEED):
    c = CASES[case]
    return {
        "model": dict({"arch": "MITH", "clip_path": "synthetic:1814:" + c["clip"], "hash_func": "tanh"}, **c["head"]),
        "dataset": {"arch": "synthetic", "name": "synth", "num_classes": C, "retrieval_num": 16, "max_word": 32, "image_resolution": 64,
                    "seed": data_seed},
        "optimizer": dict(OPT_CFG),
        "run": {"arch": "MITHTrainer", "output_dim": c["K"], "device": device, "batch_size": B, "num_workers": 0, "is_train": True,
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
    t = registry.get_runner_class("MITHTrainer").from_config(cfg=Config(config(case, out_dir, device, data_seed)), autorun=False)
    t.lines = []
    t.logger = types.SimpleNamespace(info=t.lines.append)
    return t


def capture(t, case):
    """everything the restatement needs of a trainer, on the CPU: dict(sd0: the parameters by name (gcl_t aliases gcl_i and has no name
    of its own), raw: the loader's batches as it yields them, Y0: the initial buffer, train_labels, weights: the loss's seven, heads,
    top_k: of the head's transformer and selection)"""
    model = t.model
    sd0 = {n: p.detach().cpu().clone() for n, p in model.named_parameters()}
    raw = list(t.train_loader)
    K = CASES[case]["K"]
    assert len(raw) == TRAIN_NUM // B == 3 and model.img_buffer_cls.shape == (TRAIN_NUM, K)
    for image, ids, kpm, label, index in raw:
        assert image.shape == (B, 3, 64, 64) and ids.shape == (B, 32) and kpm.shape == (B, 32) and label.shape == (B, C) and index.shape == (B,)
    assert sorted(int(i) for b in raw for i in b[4]) == list(range(TRAIN_NUM))
    return dict(sd0=sd0, raw=raw, Y0=model.img_buffer_cls.detach().cpu().clone(), train_labels=torch.as_tensor(t.train_labels).cpu().clone(),
                weights={n: float(getattr(model, n)) for n in ML.WEIGHTS}, heads=model.hash.lct_i.transformer.heads,
                top_k=model.hash.lct_i.lta.top_k)


def group_of(name):
    assert name.startswith("backbone.") or name.startswith("hash."), name
    return "backbone" if name.startswith("backbone.") else "hash"


def hyper_of(name):
    return dict(ADAM, lr=OPT_CFG["backbone_lr" if group_of(name) == "backbone" else "lr"])


def record_key(name):
    """parameter name -> (its name in a record, its row there or None): the K one-row hashing layers are stacked"""
    p = name.split(".")
    if len(p) == 6 and p[2] == "hashing" and p[3] == "fc_list":
        return ".".join(p[:4] + p[5:]), int(p[4])
    return name, None


def head_key(key):
    """record name under hash.* -> (group: gcl / i / t, the head restatement's key)"""
    p = key[len("hash."):].split(".")
    if p[1:3] == ["hashing", "fc_list"]:
        return p[0][-1], "hash_w" if p[-1] == "weight" else "hash_b"
    return MC.e2e_key(key[len("hash."):])[:2]


def kind_of(key):
    """tensor kind for pooling: tower tensors by train_step_cases.kind_of (layers pooled), head tensors by mith_head_grad_cases.kind_of
    with their group in front (the one-row hashing layers of both modalities as one kind, lct.: see the module's docstring), the
    buffer by its name"""
    if key.startswith("backbone."):
        return TS.kind_of(key)
    if key.startswith("hash."):
        g, k = head_key(key)
        return ("lct" if k in ("hash_w", "hash_b") else g) + "." + MC.kind_of(MC.grad_name(k))
    return key


def initial(sd0, dtype=np.float64):
    """sd0 -> {record name: numpy array of `dtype`}, the one-row layers stacked"""
    out, rows = {}, {}
    for n, v in sd0.items():
        key, row = record_key(n)
        if row is None:
            out[key] = v.numpy().astype(dtype)
        else:
            rows.setdefault(key, {})[row] = v.numpy().astype(dtype)
    for key, r in rows.items():
        assert sorted(r) == list(range(len(r)))
        out[key] = np.concatenate([r[k] for k in range(len(r))], 0)
    return out


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def run(cap, steps=STEPS, dtype=torch.float64, keeps=None, keep=None):
    """S training steps from cap["sd0"] on cap["raw"][s % 3] in `dtype`.  keeps: per step (image keep-set, text keep-set), [L, B, K]
    bool, or None for the head's own selection.  -> list over the steps of `keep(s, record)` (the record itself without `keep`); a
    record holds, per record name, numpy arrays of `dtype`:
      grad (before clipping), clipped (what BertAdam leaves in p.grad), p (after the step), m, v (next_m / next_v),
    and loss, terms (the ten of oracle.losses.MITH_TERMS), lr (the rate each group stepped with), next_lr (what get_lr() reports
    afterwards), count (BertAdam's step counter), Y (the buffer after the step's row write), rows (the batch's), outs (the eight head
    outputs in compute_loss's order, detached), and per modality scores [L, B, K] (detached), keep (the set used), margin
    (mith_head_grad_cases.selection's, of the scores and the token mask), mask (the token mask or None)."""
    npd = np.float64 if dtype == torch.float64 else np.float32
    out = []
    with ML.one_thread():
        t = {k: torch.tensor(v).requires_grad_(True) for k, v in initial(cap["sd0"], npd).items()}
        head = {g: {head_key(k)[1]: x for k, x in t.items() if k.startswith("hash.") and head_key(k)[0] in ("gcl", g)} for g in MODS}
        m = {k: np.zeros(tuple(x.shape), npd) for k, x in t.items()}
        v = {k: np.zeros(tuple(x.shape), npd) for k, x in t.items()}
        Y = cap["Y0"].to(dtype).clone()
        tl = cap["train_labels"].to(dtype)
        for s in range(steps):
            image, ids, kpm, label, index = cap["raw"][s % len(cap["raw"])]
            for x in t.values():
                x.grad = None
            clip = {k[len("backbone."):]: x for k, x in t.items() if k.startswith("backbone.")}
            fed = dict(clip, **{k: clip[k].unsqueeze(0).repeat(image.shape[0], 1, 1) for k in ("visual.proj", "text_projection")})
            cls_i, tok_i = enc.clip_image(fed, image.to(dtype), return_patches=True)
            eos_t, tok_t, new_mask = enc.clip_text(fed, ids, kpm, return_patches=True)
            mask = {"i": None, "t": new_mask.numpy()}
            oi, _, sc_i = MC.head_outputs(head["i"], cls_i, tok_i, None, cap["heads"], cap["top_k"], None if keeps is None else keeps[s][0])
            ot, _, sc_t = MC.head_outputs(head["t"], eos_t, tok_t, mask["t"], cap["heads"], cap["top_k"], None if keeps is None else keeps[s][1])
            Y = Y.clone()
            Y[torch.as_tensor(index).long()] = ot[2].detach()
            sim = ((tl @ torch.as_tensor(label).to(dtype).T) > 0).to(dtype)
            terms = OL.mith_terms((oi[0], ot[0], oi[1], ot[1], oi[2], ot[2], oi[3], ot[3]), Y, sim, cap["weights"])
            terms[0].backward()
            rec = {"loss": float(terms[0].detach()), "terms": np.array([float(x.detach()) for x in terms]), "Y": Y.numpy().copy(),
                   "rows": np.asarray(index).astype(np.int64), "outs": [x.detach().numpy().copy() for x in (*oi, *ot)],
                   "scores": {}, "keep": {}, "margin": {}, "mask": mask, "lr": {}, "next_lr": {}, "count": s + 1}
            for g, sc in (("i", sc_i), ("t", sc_t)):
                own, margin = MC.selection(sc, mask[g], cap["top_k"])
                rec["scores"][g], rec["margin"][g] = sc.numpy().copy(), margin.numpy().copy()
                rec["keep"][g] = own.numpy().copy() if keeps is None else np.asarray(keeps[s][MODS.index(g)]).copy()
            for kind in QUANTITIES[:2] + ("p",) + QUANTITIES[3:]:
                rec[kind] = {}
            for k, x in t.items():
                if x.grad is None:
                    continue
                h = hyper_of(k)
                lr = AC.lr_f64(h, s)
                rec["lr"][group_of(k)], rec["next_lr"][group_of(k)] = lr, AC.lr_f64(h, s + 1)
                g, p = x.grad.numpy().copy(), x.detach().numpy().copy()
                if ".hashing.fc_list." in k:                                     # K parameters of one row each: clipped one by one
                    gc = np.empty_like(g)
                    for r in range(p.shape[0]):
                        p[r:r + 1], m[k][r:r + 1], v[k][r:r + 1], gc[r:r + 1] = AC.step_f64(p[r:r + 1], g[r:r + 1], m[k][r:r + 1], v[k][r:r + 1], lr, h)
                else:
                    p, m[k], v[k], gc = AC.step_f64(p, g, m[k], v[k], lr, h)
                assert p.dtype == m[k].dtype == v[k].dtype == npd
                with torch.no_grad():
                    x.copy_(torch.from_numpy(p))
                rec["grad"][k], rec["clipped"][k], rec["p"][k] = pack(g), pack(np.asarray(gc)), p
                rec["m"][k], rec["v"][k] = pack(m[k].copy()), pack(v[k].copy())
            out.append(rec if keep is None else keep(s, rec))
    return out


def keeps_of(records):
    return [(rec["keep"]["i"], rec["keep"]["t"]) for rec in records]


# ---- conditions, sets, errors -------------------------------------------------------------------------------------------------
def check_conditions(r64, r32):
    """the conditions on the inputs, asserted on the float64 run with its own selection (r32: the float32 run with its own) -> what
    was measured: (step, clamp) -> max|Y . x|, (step, modality) -> (entries that differ, smallest finite margin, largest score
    difference, (sample, concept) pairs without a kept token), margin -> (smallest margin, largest score difference) over the run"""
    out, smallest, largest = {}, float("inf"), 0.0
    for s, (a, b) in enumerate(zip(r64, r32)):
        dots = max(float(np.abs(a["Y"] @ a["outs"][i].T).max()) for i in (1, 2, 5, 6))          # the four codes
        out[(s, "clamp")] = dots
        assert dots < ML.CLAMP - GAP, ("a buffer row within GAP of the clamp", s, dots)
        for g in MODS:
            diff = int((a["keep"][g] != b["keep"][g]).sum())
            margin = float(a["margin"][g][np.isfinite(a["margin"][g])].min())
            looked_at = np.broadcast_to(_unmasked(a["mask"][g], a["scores"][g].shape), a["scores"][g].shape)
            score = float(np.abs(b["scores"][g].astype(np.float64) - a["scores"][g])[looked_at].max())
            empty = int((~a["keep"][g].any(axis=0)).sum())
            out[(s, g)] = (diff, margin, score, empty)
            smallest, largest = min(smallest, margin), max(largest, score)
            assert diff == 0, ("the float32 restatement selects another keep-set", s, g, diff)
            assert empty >= 1, ("no (sample, concept) pair without a kept token", s, g)
    out["margin"] = (smallest, largest)
    assert smallest > TOL_FACTOR * largest, ("a selection margin within TOL_FACTOR score differences", smallest, largest)
    return out


def _unmasked(mask, shape):
    """[L, B, 1] bool: the tokens the selection looks at"""
    if mask is None:
        return np.ones((shape[0], shape[1], 1), bool)
    return ~np.asarray(mask).T[:, :, None]


def condition_lines(what, cond):
    lines = []
    for key, v in cond.items():
        if key == "margin":
            lines.append("%s condition smallest margin %.3e  largest score difference %.3e  ratio %.1f" % (what, v[0], v[1], v[0] / v[1] if v[1] else np.inf))
        elif key[1] == "clamp":
            lines.append("%s condition step %d max|Y . x| %.3f" % (what, key[0], v))
        else:
            lines.append("%s condition step %d %s  keep-set entries that differ in float32 %d  margin %.3e  score difference %.3e  empty concepts %d"
                         % ((what,) + key + v))
    return lines


def no_grad_set(cap, r64):
    return tuple(sorted({record_key(n)[0] for n in cap["sd0"]} - set(r64[0]["grad"])))


def null_set(r64):
    return tuple(sorted(k for k in r64[0]["grad"] if all(float(np.abs(dense(rec["grad"][k])).max()) < NULL_G for rec in r64)))


def quantity(rec, kind, name, init):
    """a record's tensor of one quantity as a dense numpy array; delta = p - p_initial in the record's dtype"""
    if kind == "delta":
        p = rec["p"][name]
        return p - init[name].astype(p.dtype)
    return dense(rec[kind][name])


def written_rows(cap, s):
    """the buffer rows written by the steps 0 .. s"""
    return np.unique(np.concatenate([np.asarray(cap["raw"][j % len(cap["raw"])][4]).astype(np.int64) for j in range(s + 1)]))


def errors(rec, ref, init, written):
    """rel_err of every tensor of a record against the float64 record: {(quantity, name): e}; the loss as (loss, ''), the ten terms
    relative to the largest as (terms, ''), the buffer's rows written so far as (buffer, Y)"""
    out = {("loss", ""): abs(rec["loss"] - ref["loss"]) / (abs(ref["loss"]) or 1.0), ("terms", ""): rel_err(rec["terms"], ref["terms"]),
           ("buffer", "Y"): rel_err(rec["Y"][written], ref["Y"][written])}
    for kind in QUANTITIES:
        for name in ref[kind] if kind != "delta" else ref["p"]:
            out[(kind, name)] = rel_err(quantity(rec, kind, name, init), quantity(ref, kind, name, init))
    return out


def pool(per_step):
    """list over steps of `errors` -> {(quantity, kind): the largest over the steps and layers}"""
    out = {}
    for errs in per_step:
        for (q, name), e in errs.items():
            key = (q, kind_of(name) if name else "")
            out[key] = max(out.get(key, 0.0), e)
    return out


def yardstick(cap, r64, r32):
    """the float32 restatement against the float64 one on these very inputs and keep-sets -> (per-step `errors`, their pool)"""
    init = initial(cap["sd0"])
    per = [errors(b, a, init, written_rows(cap, s)) for s, (a, b) in enumerate(zip(r64, r32))]
    return per, pool(per)


table = TS.table
