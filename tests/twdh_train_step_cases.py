"""Shared by tests/test_twdh_train_step_cpu.py and tests/test_gpu_twdh_train_step.py (not a test module): the whole training step of
TwDHTrainer.train_epoch_codes -- both CLIP towers, the DCMHT hash layer at long_dim bits, the short codes of both modalities through
the fixed transforms, the per-step tie draw, the hash-centre targets, the objective over the long code and every short code, the
backward through all of it (the long code receives its gradient both ways: directly, and from the short codes through the
transforms), BertAdam over the backbone and head groups -- restated for S steps in the dtype it is handed, the configuration of the
two cases, the conditions their inputs must meet, and the error measure.

The restatement composes only functions that a golden file pins to the reference: oracle.encode.clip_image / clip_text over a
state_dict of leaves (the projection repeated over the batch, as train_step_cases._forward feeds them), train_step_cases.dcmht_head
once per modality (BatchNorm with batch statistics for the image head, LayerNorm for the text head; train_step_cases.update_bn for
the running statistics and the batch count), twdh_cases.pair_softmax(long @ T_cat) for the short codes, twdh_cases.targets on the
batch's labels, the model's centres and that step's ties, the objective as twdh_cases.chain builds it (BCE through twdh_cases._BCE,
whose backward is (p - t) / max(p (1 - p), 1e-12) / n; the quantisation term 1 - mean((2 p - 1)^2); weights 1 and quan_alpha on the
long code and low_rate on every short term, each a mean over the two modalities), and bertadam_cases.step_f64 / lr_f64.  Parameters
are assigned to their optimiser group by name (backbone.* -> backbone_lr, hash.* -> lr), never read from the trainer.  Float64 is the
oracle; float32, with the parameters stored in float32 between the steps, is the yardstick.  Every run uses one CPU thread.

The ties.  TwDH.draw_ties draws from the CPU's global generator once per compute_loss; a test seeds torch.manual_seed(TIE_SEED + s)
before step s and `replay_ties` replays the reference's order from that seed (randint_like of a row of the long centre, then of
every short centre in key order, times 2 minus 1) inside torch.random.fork_rng, so that it leaves the global generator alone.

The cases.  Trainer settings of train_step_cases.config with TwDHTrainer: two blocks per tower, embed_dim 64, image_resolution 64,
max_word 32, B = 4, C = 6, train_num 8 (two batches in turn), shuffle off, dataset seed DATA_SEED, optimizer {lr 0.002, backbone_lr
0.0005, e 1e-3}, epochs = S = 5, each step its own train_epoch_codes call on one batch, so t_total = 5 and step 0 runs at rate 0;
synthetic transforms and centres, quan_alpha 0.5.  `rated`: lens (32, 8, 16), K_tot 56, streams start at bits 0, 32, 40, low_rate
0.3, head width N = 64 -- both ways into the long code's gradient.  `shipped`: lens (64, 4, 8, 16), K_tot 92, streams start at 0,
64, 68, 76 (inside target words), low_rate 0, the shipped value, N = 128 -- the short gradient is an exact zero and its kernel work
is skipped, yet the short terms of loss_dict are still computed.  Neither K_tot is a multiple of 32.

Conditions on the inputs (check_conditions, on the float64 run at every step; none involves the port).  1 relu: every fc2
pre-activation of both heads lies outside its near-tie bound (train_step_cases.tie_bound, ratio > 1).  2 no saturation: the smallest
p (1 - p) over the four probability matrices is at least P_FLOOR = 1e-3, so the -100 clamp and the 1e-12 floor stay inactive (those
belong to tests/test_gpu_twdh_loss.py).  3 ties: at least two of the five steps run on a batch with tie bits (an integer centre sum of
zero in a row that has labels) and in each of those steps the tie bits fall both ways; at least one step has none.  4 the float32
restatement's target bits equal the float64 run's.  DATA_SEED = TIE_SEED = 1814 meet all of them in both cases, so they stay.

Error measure.  That of train_step_cases (rel_err = max|x - f64| / max|f64| per tensor, parameters as delta = p - p_initial, tower
tensors pooled over the layers, the null set defined from the float64 run alone by NULL_G), with two more kinds: the four
probability matrices as (codes, img_long / img_short / txt_long / txt_short) and the terms vector relative to its largest entry as
(terms, '').

The null set's delta (null_delta_budget).  tests/test_gpu_train_step.py bounds |delta - delta64| of a null tensor by what BertAdam
can make of its gradient noise, sum_s lr_s max_{j<=s} max|g_j| / e.  That leaves out the rounding of the parameter as float32 stores
it, which DCMHT's noise (1e-7 and more, a budget of 4e-7 at step 1) hides and TwDH's, two hundred times smaller (its objective is
a mean over the B 2K entries of a code), does not: for backbone.visual.ln_post.bias (max|p| 0.056; the other two start at zero) the float32
restatement's own |delta - delta64| is 1.793e-9 at step 1 and 3.811e-9 at step 4 in both cases, while its noise accounts for at most
lr 0.19 max|g| / e = 4.1e-10 at step 1 (m_1 = 0.09 g_0 + 0.1 g_1); the old budget, 2.2e-9 at its own noise of 4.8e-9, holds it only
because the bound |m| <= max|g| is five times loose there, and a run with two thirds of that noise and the very same delta misses
it.  So the budget gains half an ulp of the stored parameter, 2^-24 max|p|, per step with a non-zero rate: 3.3e-9 per step here."""
import numpy as np
import torch

import bertadam_cases as AC
import train_step_cases as TS
import twdh_cases as TC
from oracle import encode as enc

STEPS = TS.STEPS
DATA_SEED = 1814                     # the dataset's seed: the first from 1814 on that meets the conditions of both cases
TIE_SEED = 1814                      # step s draws its ties after torch.manual_seed(TIE_SEED + s)
B, C = TS.B, TS.C
OPT_CFG, ADAM = TS.OPT_CFG, TS.ADAM
QUAN_ALPHA = 0.5
P_FLOOR = 1e-3
TOL_FACTOR = 4.0
NULL_G = TS.NULL_G
NULL_TWDH = TS.NULL_DCMHT            # the three biases in front of the image head's BatchNorm
QUANTITIES = TS.QUANTITIES
MODS = ("img", "txt")
CODES = ("img_long", "img_short", "txt_long", "txt_short")
CASES = {
    "rated": dict(lens=(32, 8, 16), low_rate=0.3),
    "shipped": dict(lens=(64, 4, 8, 16), low_rate=0),
}
rel_err = AC.rel_err
Rows, pack, dense = TS.Rows, TS.pack, TS.dense
group_of, hyper_of, kind_of, is_buffer = TS.group_of, TS.hyper_of, TS.kind_of, TS.is_buffer
null_set, quantity, pool, table = TS.null_set, TS.quantity, TS.pool, TS.table


# ---- configuration ------------------------------------------------------------------------------------------------------------
def config(case, out_dir, device, data_seed=DATA_SEED):
    c = CASES[case]
    cfg = TS.config("DCMHT", out_dir, device, data_seed)
    cfg["model"] = dict(cfg["model"], arch="TwDH", long_dim=c["lens"][0], trans_matrix="synthetic", short_dims=list(c["lens"][1:]),
                        long_center="synthetic", short_center="synthetic", num_classes=C, quan_alpha=QUAN_ALPHA, low_rate=c["low_rate"])
    cfg["run"]["arch"] = "TwDHTrainer"
    return cfg


def trainer(case, out_dir, device, data_seed=DATA_SEED):
    """the runner of a case, its log lines collected in `.lines`"""
    import types
    import xmh.models  # noqa: F401
    import xmh.runners  # noqa: F401
    from xmh.common.register import registry
    from xmh.utils.config import Config
    t = registry.get_runner_class("TwDHTrainer").from_config(cfg=Config(config(case, out_dir, device, data_seed)), autorun=False)
    t.lines = []
    t.logger = types.SimpleNamespace(info=t.lines.append)
    return t


def capture(t, case):
    """everything the restatement needs of a trainer, on the CPU: dict(sd0: the initial state_dict, raw: the loader's batches as it
    yields them, batches: (image, ids, labels) of each, keys: the short lengths as the model's keys in its order, lens, trans /
    long_center / short_center: copies of the model's constants, quan_alpha, low_rate)"""
    model = t.model
    sd0, raw = TS.capture(t)
    lens = CASES[case]["lens"]
    keys = list(model.trans)
    assert keys == [str(k) for k in lens[1:]] and list(model.short_center) == keys and model.long_dim == lens[0]
    assert tuple(model.long_center.shape) == (C, lens[0]) and all(tuple(model.short_center[k].shape) == (C, int(k)) for k in keys)
    assert all(tuple(model.trans[k].shape) == (2 * lens[0], 2 * int(k)) for k in keys)
    assert float(model.quan_alpha) == QUAN_ALPHA and float(model.low_rate) == float(CASES[case]["low_rate"])
    return dict(sd0=sd0, raw=raw, batches=TS.batches_of(raw), keys=keys, lens=lens, trans={k: model.trans[k].detach().cpu().clone() for k in keys},
                long_center=model.long_center.detach().cpu().clone(), short_center={k: model.short_center[k].detach().cpu().clone() for k in keys},
                quan_alpha=float(model.quan_alpha), low_rate=float(model.low_rate))


def offsets(lens):
    """the first target bit of every stream, and K_tot"""
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


# ---- the pieces ---------------------------------------------------------------------------------------------------------------
def replay_ties(cap, s, seed=TIE_SEED):
    """the ties TwDH.draw_ties returns after torch.manual_seed(seed + s): {"long" / key: +-1 fp32}; the global generator is left as
    it was"""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed + s)
        ties = {"long": torch.randint_like(cap["long_center"][0], 2)}
        for k in cap["keys"]:
            ties[k] = torch.randint_like(cap["short_center"][k][0], 2)
    return {k: v * 2 - 1 for k, v in ties.items()}


def centres_of(cap):
    return [cap["long_center"].numpy()] + [cap["short_center"][k].numpy() for k in cap["keys"]]


def ties_list(cap, ties):
    return [np.asarray(ties["long"])] + [np.asarray(ties[k]) for k in cap["keys"]]


def tie_places(labels, centres):
    """[B, K_tot] bool: the target bits the tie vector decides -- an integer centre sum of zero in a row that has labels"""
    lab = (np.asarray(labels) == 1)
    cen = np.concatenate([np.asarray(c) for c in centres], 1).astype(np.int64)[:lab.shape[1]]
    return ((lab.astype(np.int64) @ cen) == 0) & (lab.sum(1) > 0)[:, None]


def stream(lens, long, short, s):
    """the [B, 2 K_s] matrix of stream s of one modality"""
    o = offsets(lens)
    return long if s == 0 else short[:, 2 * (o[s] - lens[0]):2 * (o[s + 1] - lens[0])]


def objective(longs, shorts, bits, lens, quan_alpha, low_rate, dtype):
    """the objective as twdh_cases.chain builds it, on torch tensors with a graph: longs / shorts {"img" / "txt": [B, 2 K]} -> (the
    total with its graph, the terms vector [1 + 6 n] in the layout of xmh_twdh_loss, detached)"""
    o, n = offsets(lens), len(lens)
    per, means, total = {}, [], 0
    for s in range(n):
        for term in range(2):
            v = 0
            for m in MODS:
                p = stream(lens, longs[m], shorts[m], s)
                if term == 0:
                    x = TC._BCE.apply(p, TC.pair_targets(bits[:, o[s]:o[s + 1]], dtype))
                else:
                    x = 1 - ((2 * p - 1) ** 2).mean()
                per[(m, s, term)] = x
                v = v + x
            w = (1.0 if term == 0 else quan_alpha) if s == 0 else low_rate
            total = total + w * v / 2
            means.append(v / 2)
    vec = [total] + [per[(m, s, term)] for m in MODS for s in range(n) for term in range(2)] + means
    return total, torch.stack([x.detach() for x in vec])


def loss_dict_places(n):
    """the scalars of the terms vector that loss_dict reports, in the order All loss, Long NCE image / text, Long Quan image / text,
    then Short NCE, Quan per key in key order"""
    out = [0, 1, 1 + 2 * n, 2, 2 + 2 * n]
    for i in range(n - 1):
        out += [1 + 4 * n + 2 * (i + 1), 2 + 4 * n + 2 * (i + 1)]
    return out


def loss_dict_names(keys):
    return ["All", "Long.NCE.image", "Long.NCE.text", "Long.Quan.image", "Long.Quan.text"] + [x % k for k in keys for x in ("Short.%s.NCE", "Short.%s.Quan")]


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def run(cap, steps=STEPS, dtype=torch.float64, bits=None, masks=None, keep=None, tie_seed=TIE_SEED):
    """S training steps from cap["sd0"] on cap["batches"][s % 2] in `dtype`.  bits: per step the target bits [B, K_tot] to take in
    place of twdh_cases.targets of the replayed ties; masks: per step {"img" / "txt": [B, N] bool}, the relu decisions to take in
    place of z > 0.  -> list over the steps of `keep(s, record)` (the record itself without `keep`); a record holds, per parameter
    name, numpy arrays of `dtype`:
      grad (before clipping), clipped (what BertAdam leaves in p.grad), p (after the step), m, v (next_m / next_v),
    and loss, lr (the rate each group stepped with), next_lr (what get_lr() reports afterwards), count (BertAdam's step counter),
    buffers (BatchNorm's running_mean / running_var / num_batches_tracked), z / tie (fc2 pre-activations of both heads and their tie
    bound), masks (the relu decisions taken), terms (the vector of xmh_twdh_loss, 1 + 6 n), probs (the four probability matrices by
    CODES), bits (the target bits taken), ties (the replayed ties as one [K_tot] vector) and tie_places."""
    npd = np.float64 if dtype == torch.float64 else np.float32
    lens, keys = cap["lens"], cap["keys"]
    out = []
    with TS.DC.one_thread():
        sd0 = cap["sd0"]
        t = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd0.items() if v.is_floating_point() and not is_buffer(k)}
        buf = {k: (v.detach().to(dtype).clone() if v.is_floating_point() else int(v)) for k, v in sd0.items() if is_buffer(k)}
        m = {k: np.zeros(tuple(x.shape), npd) for k, x in t.items()}
        v = {k: np.zeros(tuple(x.shape), npd) for k, x in t.items()}
        T = torch.cat([cap["trans"][k] for k in keys], 1).to(dtype)
        centres = centres_of(cap)
        for s in range(steps):
            image, ids, labels = cap["batches"][s % len(cap["batches"])]
            for x in t.values():
                x.grad = None
            clip = {k[len("backbone."):]: x for k, x in t.items() if k.startswith("backbone.")}
            fed = dict(clip, **{k: clip[k].unsqueeze(0).repeat(image.shape[0], 1, 1) for k in ("visual.proj", "text_projection")})
            emb = {"img": enc.clip_image(fed, image.to(dtype)), "txt": enc.clip_text(fed, ids, None)}
            heads = {mod: {k[len("hash.%s_hash." % mod):]: x for k, x in t.items() if k.startswith("hash.%s_hash." % mod)} for mod in MODS}
            longs, aux = {}, {}
            for mod in MODS:
                longs[mod], aux[mod] = TS.dcmht_head(emb[mod], heads[mod], mod == "img", mask=None if masks is None else masks[s][mod])
            TS.update_bn(buf, aux["img"]["o"].detach())
            shorts = {mod: TC.pair_softmax(longs[mod] @ T) for mod in MODS}
            ties = replay_ties(cap, s, tie_seed)
            b = TC.targets(labels, centres, ties_list(cap, ties)) if bits is None else np.asarray(bits[s])
            total, terms = objective(longs, shorts, b, lens, cap["quan_alpha"], cap["low_rate"], dtype)
            total.backward()
            assert t["backbone.logit_scale"].grad is None
            rec = {"loss": float(total.detach()), "terms": terms.numpy().copy(), "bits": b.copy(), "lr": {}, "next_lr": {}, "count": s + 1,
                   "ties": np.concatenate([x.reshape(-1) for x in ties_list(cap, ties)]), "tie_places": tie_places(labels, centres),
                   "z": {mod: aux[mod]["z"].detach().double().numpy() for mod in MODS},
                   "tie": {mod: TS.tie_bound(aux[mod]["n"].detach().numpy(), heads[mod]["fc2.weight"].detach().numpy()) for mod in MODS},
                   "probs": {"img_long": longs["img"].detach().numpy().copy(), "img_short": shorts["img"].detach().numpy().copy(),
                             "txt_long": longs["txt"].detach().numpy().copy(), "txt_short": shorts["txt"].detach().numpy().copy()}}
            rec["masks"] = {mod: (rec["z"][mod] > 0) if masks is None else np.asarray(masks[s][mod]).copy() for mod in MODS}
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
                rec["grad"][k], rec["clipped"][k], rec["p"][k], rec["m"][k], rec["v"][k] = pack(g), pack(np.asarray(gc)), p, pack(m[k]), pack(v[k])
            rec["buffers"] = {k: (x.numpy().copy() if torch.is_tensor(x) else x) for k, x in buf.items()}
            out.append(rec if keep is None else keep(s, rec))
    return out


def bits_of(records):
    return [rec["bits"] for rec in records]


def masks_of(records):
    return [rec["masks"] for rec in records]


# ---- conditions, errors -------------------------------------------------------------------------------------------------------
def check_conditions(r64, r32_bits):
    """the conditions on the inputs, asserted on the float64 run at every step (r32_bits: the float32 restatement's target bits per
    step) -> what was measured: (step, "img" / "txt") -> (min|z|, min|z| / tie bound), (step, "p") -> the smallest p (1 - p),
    (step, "ties") -> (tie bits, of them set, target bits)"""
    out, tied = {}, []
    for s, rec in enumerate(r64):
        for mod in MODS:
            ratio = np.abs(rec["z"][mod]) / rec["tie"][mod]
            out[(s, mod)] = (float(np.abs(rec["z"][mod]).min()), float(ratio.min()))
            assert rec["z"][mod].shape == rec["probs"][mod + "_long"].shape and ratio.min() > 1.0, ("fc2 pre-activation inside its tie bound", s, mod, out[(s, mod)])
        out[(s, "p")] = min(float((p * (1 - p)).min()) for p in rec["probs"].values())
        assert out[(s, "p")] >= P_FLOOR, ("a saturated probability", s, out[(s, "p")])
        at = rec["tie_places"]
        n, up = int(at.sum()), int(rec["bits"][at].sum())
        out[(s, "ties")] = (n, up, int(at.size))
        assert np.array_equal(rec["bits"][at], np.broadcast_to(rec["ties"] > 0, at.shape)[at])
        if n:
            tied.append(s)
            assert 0 < up < n, ("the tie bits of a step fall one way only", s, n, up)
        assert np.array_equal(r32_bits[s], rec["bits"]), ("the float32 restatement's target bits differ", s)
    assert len(tied) >= 2 and len(tied) < len(r64), ("steps with tie bits", tied)
    return out


def condition_lines(what, cond):
    lines = []
    for (s, key), v in cond.items():
        if key == "p":
            lines.append("%s condition step %d smallest p (1 - p) %.4f" % (what, s, v))
        elif key == "ties":
            lines.append("%s condition step %d tie bits %d of %d, %d of them set" % (what, s, v[0], v[2], v[1]))
        else:
            lines.append("%s condition step %d %s min|z| %.3e = %.0f tie bounds" % (what, s, key, v[0], v[1]))
    return lines


def errors(rec, ref, sd0, null=(), places=None):
    """train_step_cases.errors, and the four code matrices as (codes, name) and the terms vector relative to its largest entry as
    (terms, ''); places: the scalars of the float64 terms vector that rec["terms"] holds (all of them without)"""
    out = TS.errors(rec, ref, sd0, null)
    want = ref["terms"] if places is None else ref["terms"][places]
    out[("terms", "")] = rel_err(rec["terms"], want)
    for k in CODES:
        out[("codes", k)] = rel_err(rec["probs"][k], ref["probs"][k])
    return out


def null_delta_budget(lrs, gs, p_max):
    """how far the delta of a null-set tensor may lie from the float64 delta after the steps 0 .. s: lrs / gs the rate and the run's
    max|g| of each of those steps, p_max the largest |p| the run stores.  The first part is the rule of tests/test_gpu_train_step.py,
    what BertAdam can make of the noise (|m| <= max|g|, |u| <= |m| / e); the second is the rounding of the float32 parameter as it is
    stored, half an ulp, at most 2^-24 |p|, once per step that moves it (the module's docstring: TwDH's noise is too small to hide it)"""
    noise = sum(lrs[j] * max(gs[:j + 1]) / ADAM["e"] for j in range(len(lrs)))
    return noise + sum(1 for lr in lrs if lr > 0) * 2.0 ** -24 * p_max


def yardstick(cap, r64, r32, null=()):
    """the float32 restatement against the float64 one on these very inputs and ties -> (per-step `errors`, their pool, per step the
    float32 run's max|g| of every null tensor)"""
    per = [errors(b, a, cap["sd0"], null) for a, b in zip(r64, r32)]
    return per, pool(per), [{n: float(np.abs(dense(b["grad"][n])).max()) for n in null} for b in r32]
