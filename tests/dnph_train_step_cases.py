"""Shared by tests/test_dnph_train_step_cpu.py and tests/test_gpu_dnph_train_step.py (not a test module): the whole training step of
DNPHTrainer.train_epoch -- both CLIP towers, the code and the 80 class logits of both modalities, the noise draw and its min-cost
assignment to the codes, the proxy + noise objective, the backward through all of it, BertAdam over the backbone and head groups, plain
SGD over the proxies -- restated for S steps in the dtype it is handed, the configuration of the two cases, the conditions their inputs
must meet, and the error measure.

The restatement composes only functions that a golden file pins to the reference: oracle.encode.clip_image / clip_text over a
state_dict of leaves (the projection repeated over the batch, as train_step_cases._forward feeds them; no key padding mask), the code
tanh((x W^T + b) keep / (1 - p)) and the 80-wide prediction layer x Wp^T + bp per modality as dnph_cases.chain writes them,
dnph_cases.objective_terms with mrg, noise_alpha and the assigned noise as constants, and bertadam_cases.step_f64 / lr_f64.  The
assignment is the restatement's own: all B! = 24 permutations of the float64 cost ||h_i - s_j||_2 are summed and the smallest total
wins (`brute_force`); xmh_assign_min_cost is never called.  The proxies step by p - lr g at the configuration's optimizer.loss.lr,
without momentum or weight decay, in `dtype`.  Parameters are assigned to their optimiser by name (backbone.* -> BertAdam at backbone_lr,
hash.* -> BertAdam at lr, loss.proxies -> the SGD), never read from the trainer.  Float64 is the oracle; float32, with the parameters
stored in float32 between the steps, is the yardstick.  Every run uses one CPU thread.  Keep masks and the +-1 noise matrices are handed
in and never drawn here (`draw_masks` replays the heads' torch.rand(B, K) >= 0.2 calls, image then text, after torch.manual_seed;
`draw_noises` replays np.random.default_rng(seed).integers(0, 2, (B, K)) * 2 - 1, one call per step).

The cases.  Trainer settings of train_step_cases.config with DNPHTrainer: B = 4, C = 6, train_num 12 so that three batches cycle,
max_word 32, image_resolution 64, shuffle off, optimizer {lr 0.002, backbone_lr 0.0005, e 1e-3, loss {lr 0.01}}, numclass 6, mrg 1.0,
noise_alpha 0.1 given explicitly (from_config's own default is 1.0), epochs = S = 5, each step its own train_epoch call on one batch, so
t_total = 5 and step 0 runs at rate 0 (the proxies' SGD has no schedule and moves at step 0).  `plain`: one block per tower at
embed_dim 64, K = 16.  `wide`: two blocks per tower at embed_dim 128, K = 24.  80 logits against 6 classes in both.

Conditions on the inputs (check_conditions; none involves the port).  1 the brute-force minimum is unique: at every step and modality
the best permutation's total cost lies below the second best by more than TOL_FACTOR = 4 times the largest float32-against-float64
change of any permutation's total, and the float32 run chooses the same permutation.  2 every code row and every proxy row has a norm
of at least 1e-6, far from F.normalize's eps branch (tests/test_gpu_dnph_loss_f64.py covers that branch).  3 every batch row has a label.

Error measure.  That of train_step_cases: rel_err = max|x - f64| / max|f64| per tensor, parameters as delta = p - p_initial, pooled per
quantity and tensor kind over steps and layers (`kind_of`: tower tensors by train_step_cases.kind_of, the eight head tensors each a kind
of its own in grad, clipped, m and v, the proxies a kind of their own throughout); the two codes and the two logit matrices as
compute_loss receives them go as (codes, <name>), the six terms relative to the largest as (terms, '').

The delta of a modality's four head tensors (code layer and prediction layer, weight and bias) pools into one kind per modality
(hash.image, hash.text), for the reason tests/dimch_train_step_cases.py gives with its figures: a bias that starts at zero has the delta
-lr m / (sqrt(v) + e), an entry whose gradient is far below the tensor's largest has sqrt(v) of the size of e = 1e-3, an error that is
small against max|m| is divided by it, and where a float32 run's rounding falls decides the yardstick of such a tensor.  Here two
float32 runs of this very restatement on two CPUs differ by up to 1.9 in a delta's yardstick, and the port's delta of the 24-entry
hash.text_hash.fc.bias in `wide`, 1.74e-5, is 2.3 times the one run's 7.4e-6 and 3.55 times the other's 4.90e-6 with grad, clipped, m
and v of that tensor at 1.3 times theirs at most: a bound that near cannot rest on one tensor's accident.  Pooled, the yardstick is set by a weight matrix
(1.68e-5 there) and the factor stays 4."""
import itertools

import numpy as np
import torch

import bertadam_cases as AC
import dnph_cases as DN
import train_step_cases as TS
from oracle import encode as enc

STEPS = TS.STEPS
DATA_SEED = 1814                     # the dataset's seed: the first from 1814 on that meets the conditions of both cases
MASK_SEED = 1814                     # torch.manual_seed(MASK_SEED + s) before step s
MODEL_SEED = 1814                    # model.seed: the proxies and model.noise_generator
B, C, TRAIN_NUM, CP = 4, 6, 12, 80
OPT_CFG = TS.OPT_CFG
ADAM = TS.ADAM
PROXY_LR = 0.01
MRG, NOISE_ALPHA, DROP_P = 1.0, 0.1, 0.2
MIN_NORM = 1e-6
TOL_FACTOR = 4.0
NULL_G = TS.NULL_G
QUANTITIES = TS.QUANTITIES
MODS = ("img", "txt")
TERMS = DN.TERMS
OUTS = ("img_hash", "txt_hash", "img_pre", "txt_pre")
PROXIES = "loss.proxies"
PERMS = np.array(list(itertools.permutations(range(B))))           # [24, B]: row i of the batch gets noise vector PERMS[k, i]
_CLIP = "vision_layers=%d,transformer_layers=%d,vision_width=128,transformer_width=128,embed_dim=%d,image_resolution=64"
CASES = {"plain": dict(clip=_CLIP % (1, 1, 64), K=16), "wide": dict(clip=_CLIP % (2, 2, 128), K=24)}
rel_err = AC.rel_err
Rows, pack, dense = TS.Rows, TS.pack, TS.dense
table = TS.table
quantity = TS.quantity


# ---- configuration ------------------------------------------------------------------------------------------------------------
def config(case, out_dir, device, data_seed=DATA_SEED):
    c = CASES[case]
    return {
        "model": {"arch": "DNPH", "clip_path": "synthetic:1814:" + c["clip"], "numclass": C, "mrg": MRG, "noise_alpha": NOISE_ALPHA,
                  "hash_func": "tanh", "seed": MODEL_SEED},
        "dataset": {"arch": "synthetic", "name": "synth", "num_classes": C, "retrieval_num": 16, "max_word": 32, "image_resolution": 64,
                    "seed": data_seed},
        "optimizer": dict(OPT_CFG, loss={"lr": PROXY_LR}),
        "run": {"arch": "DNPHTrainer", "output_dim": c["K"], "device": device, "batch_size": B, "num_workers": 0, "is_train": True,
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
    t = registry.get_runner_class("DNPHTrainer").from_config(cfg=Config(config(case, out_dir, device, data_seed)), autorun=False)
    t.lines = []
    t.logger = types.SimpleNamespace(info=t.lines.append)
    return t


def capture(t, case):
    """everything the restatement needs of a trainer, on the CPU: dict(case, K, sd0: the parameters by name, raw: the loader's batches
    as it yields them)"""
    K = CASES[case]["K"]
    sd0 = {n: p.detach().cpu().clone() for n, p in t.model.named_parameters()}
    raw = list(t.train_loader)
    assert len(raw) == TRAIN_NUM // B == 3
    for image, ids, kpm, label, index in raw:
        assert image.shape == (B, 3, 64, 64) and ids.shape == (B, 32) and label.shape == (B, C) and index.shape == (B,)
    assert sorted(int(i) for b in raw for i in b[4]) == list(range(TRAIN_NUM))
    assert tuple(sd0[PROXIES].shape) == (C, K) and sum(n.startswith("hash.") for n in sd0) == 8 and sum(n.startswith("loss.") for n in sd0) == 1
    for mod in MODS:
        assert sd0["hash." + DN.HEAD_KEYS["hash_w"] % DN.MOD[mod]].shape[0] == K and sd0["hash." + DN.HEAD_KEYS["pre_w"] % DN.MOD[mod]].shape[0] == CP
    return dict(case=case, K=K, sd0=sd0, raw=raw)


def kind_of(name, quantity=None):
    """tensor kind for pooling: train_step_cases.kind_of, but the delta of a modality's head tensors as one kind (the module's docstring)"""
    if quantity == "delta" and name.startswith("hash."):
        return "hash." + name.split(".")[1].split("_")[0]
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
    assert name.startswith("backbone.") or name.startswith("hash.") or name == PROXIES, name
    return "backbone" if name.startswith("backbone.") else "hash" if name.startswith("hash.") else "sgd"


def hyper_of(name):
    return dict(ADAM, lr=OPT_CFG["backbone_lr" if group_of(name) == "backbone" else "lr"])


def draw_masks(cap, device="cpu", steps=STEPS, seed=MASK_SEED):
    """per step (keep_img, keep_txt), uint8 [B, K] on the CPU: the heads' own torch.rand(B, K, device=device) >= 0.2 calls, image then
    text, after torch.manual_seed(seed + s)"""
    out = []
    for s in range(steps):
        torch.manual_seed(seed + s)
        out.append(tuple((torch.rand(B, cap["K"], device=device) >= DROP_P).cpu().to(torch.uint8) for _ in MODS))
    return out


def draw_noises(cap, steps=STEPS, seed=MODEL_SEED):
    """per step the +-1 matrix [B, K] int64 that model.rand_unit_rect draws: one generator for the run, one call per step"""
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 2, size=(B, cap["K"]), dtype=np.int64) * 2 - 1 for _ in range(steps)]


def brute_force(h, s):
    """codes h [B, K] and noise vectors s [B, K] (any dtype; the cost is float64) -> (index into PERMS of the smallest total of
    ||h_i - s_perm(i)||_2, the 24 totals)"""
    h, s = np.asarray(h, np.float64), np.asarray(s, np.float64)
    cost = np.sqrt(((h[:, None, :] - s[None, :, :]) ** 2).sum(-1))
    totals = np.array([sum(cost[i, p[i]] for i in range(len(p))) for p in PERMS])
    return int(np.argmin(totals)), totals


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def run(cap, masks, noises, steps=STEPS, dtype=torch.float64, perms=None, keep=None):
    """S training steps from cap["sd0"] on cap["raw"][s % 3] in `dtype`.  masks: per step (keep_img, keep_txt) [B, K] of 0 / 1; noises:
    per step the +-1 matrix [B, K]; perms: per step (image, text) indices into PERMS to take, or None for the run's own brute force.
    -> list over the steps of `keep(s, record)` (the record itself without `keep`); a record holds, per parameter name, numpy arrays of
    `dtype`:
      grad (before clipping; the proxies' too), clipped (what BertAdam leaves in p.grad), p (after the step; the proxies' too), m, v,
    and loss, terms (the six of dnph_cases.TERMS), lr (the rate each BertAdam group stepped with), next_lr, count, outs (the two codes
    and the two logit matrices in compute_loss's order, detached), perm / totals per modality (the assignment taken, the 24 totals of
    this run's own codes), norms (of every code row of both modalities and of every proxy row, before the step), labels, buffers (none)."""
    npd = np.float64 if dtype == torch.float64 else np.float32
    out = []
    with TS.DC.one_thread():
        t = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in cap["sd0"].items()}
        adam = [k for k in t if group_of(k) != "sgd"]
        m = {k: np.zeros(tuple(t[k].shape), npd) for k in adam}
        v = {k: np.zeros(tuple(t[k].shape), npd) for k in adam}
        for s in range(steps):
            image, ids, _, label, _ = cap["raw"][s % len(cap["raw"])]
            for x in t.values():
                x.grad = None
            clip = {k[len("backbone."):]: x for k, x in t.items() if k.startswith("backbone.")}
            fed = dict(clip, **{k: clip[k].unsqueeze(0).repeat(image.shape[0], 1, 1) for k in ("visual.proj", "text_projection")})
            x = {"img": enc.clip_image(fed, image.to(dtype)), "txt": enc.clip_text(fed, ids, None)}
            f, p, rec = {}, {}, {"perm": {}, "totals": {}}
            assigned = {}
            for i, mod in enumerate(MODS):
                P = {k: t["hash." + DN.HEAD_KEYS[k] % DN.MOD[mod]] for k in DN.HEAD_PARAMS}
                z = x[mod] @ P["hash_w"].T + P["hash_b"]
                f[mod] = torch.tanh(z * torch.as_tensor(masks[s][i]).to(dtype) / (1.0 - DROP_P))
                p[mod] = x[mod] @ P["pre_w"].T + P["pre_b"]
                own, rec["totals"][mod] = brute_force(f[mod].detach().numpy(), noises[s])
                rec["perm"][mod] = own if perms is None else int(perms[s][i])
                assigned[mod] = torch.as_tensor(noises[s][PERMS[rec["perm"][mod]]]).to(dtype)
            terms = DN.objective_terms(f["img"], f["txt"], p["img"], p["txt"], t[PROXIES], torch.as_tensor(label), MRG, NOISE_ALPHA,
                                       assigned["img"], assigned["txt"])
            terms[0].backward()
            rec.update({"loss": float(terms[0].detach()), "terms": terms.detach().double().numpy().copy(),
                        "outs": [a.detach().numpy().copy() for a in (f["img"], f["txt"], p["img"], p["txt"])],
                        "norms": np.concatenate([np.linalg.norm(a.detach().double().numpy(), axis=1) for a in (f["img"], f["txt"], t[PROXIES])]),
                        "labels": np.asarray(label).copy(), "lr": {}, "next_lr": {}, "count": s + 1, "buffers": {}})
            for kind in QUANTITIES[:2] + ("p",) + QUANTITIES[3:]:
                rec[kind] = {}
            for k in adam:
                if t[k].grad is None:
                    continue
                h = hyper_of(k)
                lr = AC.lr_f64(h, s)
                rec["lr"][group_of(k)], rec["next_lr"][group_of(k)] = lr, AC.lr_f64(h, s + 1)
                g = t[k].grad.numpy().copy()
                q, m[k], v[k], gc = AC.step_f64(t[k].detach().numpy(), g, m[k], v[k], lr, h)
                assert q.dtype == m[k].dtype == v[k].dtype == npd
                with torch.no_grad():
                    t[k].copy_(torch.from_numpy(q))
                rec["grad"][k], rec["clipped"][k], rec["p"][k] = pack(g), pack(np.asarray(gc)), q
                rec["m"][k], rec["v"][k] = pack(m[k].copy()), pack(v[k].copy())
            g = t[PROXIES].grad.numpy().copy()                                       # plain SGD, in `dtype`
            q = t[PROXIES].detach().numpy() - npd(PROXY_LR) * g
            assert q.dtype == npd
            with torch.no_grad():
                t[PROXIES].copy_(torch.from_numpy(q))
            rec["grad"][PROXIES], rec["p"][PROXIES] = g, q.copy()
            out.append(rec if keep is None else keep(s, rec))
    return out


def perms_of(records):
    return [(rec["perm"]["img"], rec["perm"]["txt"]) for rec in records]


# ---- conditions, sets, errors -------------------------------------------------------------------------------------------------
def check_conditions(r64, r32):
    """the conditions on the inputs, asserted on the float64 run with its own assignment (r32: the float32 run with its own) -> what
    was measured: (step, modality) -> (the permutation, second best total - best total, largest |total32 - total64| of any
    permutation, the float32 run's permutation), 'margin' -> (smallest gap, largest change) over the run, (step, 'norm') -> the
    smallest row norm, (step, 'labels') -> labels per row"""
    out, smallest, largest = {}, np.inf, 0.0
    for s, (a, b) in enumerate(zip(r64, r32)):
        for mod in MODS:
            tot = np.sort(a["totals"][mod])
            gap, change = float(tot[1] - tot[0]), float(np.abs(b["totals"][mod] - a["totals"][mod]).max())
            out[(s, mod)] = (a["perm"][mod], gap, change, b["perm"][mod])
            smallest, largest = min(smallest, gap), max(largest, change)
            assert a["perm"][mod] == int(np.argmin(a["totals"][mod])) and b["perm"][mod] == a["perm"][mod], ("float32 assigns otherwise", s, mod)
        out[(s, "norm")] = float(a["norms"].min())
        assert a["norms"].shape == (2 * B + C,) and out[(s, "norm")] >= MIN_NORM, ("a row near F.normalize's eps branch", s, out[(s, "norm")])
        out[(s, "labels")] = a["labels"].sum(1).astype(int).tolist()
        assert a["labels"].shape == (B, C) and min(out[(s, "labels")]) >= 1, ("a batch row without a label", s)
    out["margin"] = (smallest, largest)
    assert smallest > TOL_FACTOR * largest, ("the best assignment within TOL_FACTOR float32 changes of the second best", smallest, largest)
    return out


def condition_lines(what, cond):
    lines = []
    for key, v in cond.items():
        if key == "margin":
            lines.append("%s condition assignment  margin %.3e  noise %.3e  ratio %.1f" % (what, v[0], v[1], v[0] / v[1] if v[1] else np.inf))
        elif key[1] in MODS:
            lines.append("%s condition step %d %s permutation %s  second best - best %.3e  largest float32 change of a total %.3e  float32 takes %s"
                         % (what, key[0], key[1], PERMS[v[0]].tolist(), v[1], v[2], PERMS[v[3]].tolist()))
        else:
            lines.append("%s condition step %d %s %s" % (what, key[0], key[1], v))
    return lines


def no_grad_set(cap, r64):
    return tuple(sorted(set(cap["sd0"]) - set(r64[0]["grad"])))


def null_set(r64):
    return tuple(sorted(k for k in r64[0]["grad"] if all(float(np.abs(dense(rec["grad"][k])).max()) < NULL_G for rec in r64)))


def errors(rec, ref, sd0, null=(), places=None):
    """train_step_cases.errors (the proxies have grad and delta) and, on top, the six terms relative to the largest as (terms, '') and
    the two codes and two logit matrices as (codes, <name>).  places: the terms to look at (the port's loss_dict has three of them)"""
    out = TS.errors(rec, ref, sd0, null)
    places = list(range(len(TERMS))) if places is None else places
    out[("terms", "")] = rel_err(np.asarray(rec["terms"])[places], np.asarray(ref["terms"])[places])
    for name, a, b in zip(OUTS, rec["outs"], ref["outs"]):
        out[("codes", name)] = rel_err(a, b)
    return out


def yardstick(cap, r64, r32, null=(), places=None):
    """the float32 restatement against the float64 one on these very inputs, masks and assignments -> (per-step `errors`, their pool,
    per step the float32 run's max|g| of every null tensor)"""
    per = [errors(b, a, cap["sd0"], null, places) for a, b in zip(r64, r32)]
    return per, pool(per), [{n: float(np.abs(dense(b["grad"][n])).max()) for n in null} for b in r32]
