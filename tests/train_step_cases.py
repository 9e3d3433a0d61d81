"""Shared by tests/test_train_step_cpu.py, tests/test_gpu_train_step.py and tests/test_gpu_bertadam.py (not a test module): the whole
training step of the DCMHT and DSPH runners -- both CLIP towers, the hash heads, the loss, the backward through all of it, BertAdam
over the backbone and head groups, SGD over DSPH's proxies -- restated for S steps in the dtype it is handed, the configuration of
the two cases, the conditions their inputs must meet, and the error measure.

The restatement composes only functions that a golden file pins to the reference: oracle.encode.clip_image / clip_text over a
state_dict of leaves (as tower_grad_cases.run_restatement feeds them: the projection repeated over the batch), the DCMHT head
(`dcmht_head`: BatchNorm with batch statistics for the image head, LayerNorm for the text head), the DSPH head
tanh((x W^T + b) keep / (1 - p)), dcmht_loss_cases.terms / oracle.losses.hyp_terms, bertadam_cases.step_f64 / lr_f64, and torch's
SGD.  Parameters are assigned to their optimiser group by name here (backbone.* -> backbone_lr, hash.* -> lr, hyp.* -> SGD), not
read from the trainer.  Float64 is the oracle; float32, with the parameters stored in float32 between the steps, is the yardstick.
Every run uses one CPU thread.  Dropout keep masks are handed in and never drawn here.

The cases.  Trainer settings of tests/test_gpu_tower_grad.py::_trainer with two layers per tower (the hand-over between blocks is
part of what composes), shuffle off, optimizer {lr 0.002, backbone_lr 0.0005, e 1e-3} (both groups move visibly and a parameter
in the wrong group shows; e as argued above OPT_CFG of tests/test_gpu_bertadam.py), DSPH with hyp {lr 0.05, momentum 0.9,
weight_decay 0.0005}.  S = 5 steps on the loader's two batches in turn, each step its own train_epoch call with t_total = S, so the
first step runs at rate 0 (warm-up) and leaves every parameter unchanged while next_m / next_v are filled.

Error measure.  rel_err = max|x - f64| / max|f64| per tensor; parameters are compared as delta = p_after_step - p_initial (a step
moves a backbone weight by 1e-4 of its size: p itself would pass with the step missing).  A gradient that is identically zero in
exact arithmetic holds rounding noise only; the null set is defined from the float64 run alone (max|g64| < NULL_G at every step)
and its tensors get absolute bounds.

A record keeps gradients and moments of the token embedding by their non-zero rows (`Rows`): 49408 rows of which a batch touches a
hundred."""
import numpy as np
import torch

import bertadam_cases as AC
import dcmht_loss_cases as DC
import tower_grad_cases as TC
from oracle import encode as enc
from oracle import heads_train as HT
from oracle import losses as OL

ARCHS = {"DCMHT": "DCMHTTrainer", "DSPH": "DSPHTrainer"}
STEPS = 5
DATA_SEED = 1814                     # the dataset's seed: the first from 1814 on that meets the conditions of both cases
B, K, C = 4, 16, 6
OPT_CFG = {"lr": 0.002, "backbone_lr": 0.0005, "e": 1e-3}
HYP_CFG = {"lr": 0.05, "momentum": 0.9, "weight_decay": 0.0005}
HYP_MODEL = {"numclass": C, "alpha": 0.8, "threshold": 0.25}
ADAM = dict(warmup=0.1, t_total=STEPS, schedule="warmup_cosine", b1=0.9, b2=0.98, e=OPT_CFG["e"], weight_decay=0.2, max_grad_norm=1.0)
BN_MOMENTUM, NORM_EPS, DROP_P = 0.1, 1e-5, 0.2
GAP = DC.GAP
NULL_G = 1e-10
NULL_DCMHT = ("backbone.visual.ln_post.bias", "hash.img_hash.atten.in_proj_bias", "hash.img_hash.atten.out_proj.bias")
QUANTITIES = ("grad", "clipped", "delta", "m", "v")
BUFFERS = ("running_mean", "running_var", "num_batches_tracked")
rel_err = AC.rel_err


# ---- configuration ------------------------------------------------------------------------------------------------------------
def config(arch, out_dir, device, data_seed=DATA_SEED):
    small = "vision_layers=2,transformer_layers=2,vision_width=128,transformer_width=128,embed_dim=64,image_resolution=64"
    opt = dict(OPT_CFG, hyp=dict(HYP_CFG)) if arch == "DSPH" else dict(OPT_CFG)
    return {
        "model": dict({"arch": arch, "clip_path": "synthetic:1814:" + small}, **(HYP_MODEL if arch == "DSPH" else {})),
        "dataset": {"arch": "synthetic", "name": "synth", "num_classes": C, "retrieval_num": 16, "max_word": 32, "image_resolution": 64,
                    "seed": data_seed},
        "optimizer": opt,
        "run": {"arch": ARCHS[arch], "output_dim": K, "device": device, "batch_size": B, "num_workers": 0, "is_train": True, "query_num": 8,
                "train_num": 8, "epochs": STEPS, "shuffle": False, "save_dir": str(out_dir), "log_dir": str(out_dir), "seed": 1814},
    }


def trainer(arch, out_dir, device, data_seed=DATA_SEED):
    """the runner of a case, its log lines collected in `.lines`"""
    import types
    import xmh.models  # noqa: F401
    import xmh.runners  # noqa: F401
    from xmh.common.register import registry
    from xmh.utils.config import Config
    t = registry.get_runner_class(ARCHS[arch]).from_config(cfg=Config(config(arch, out_dir, device, data_seed)), autorun=False)
    t.lines = []
    t.logger = types.SimpleNamespace(info=t.lines.append)
    return t


def capture(t):
    """-> (initial state_dict on the CPU, the loader's batches as the loader yields them)"""
    sd0 = {k: v.detach().cpu().clone() for k, v in t.model.state_dict().items()}
    raw = list(t.train_loader)
    assert len(raw) == 2 and all(b[0].shape == (B, 3, 64, 64) and b[1].shape == (B, 32) and b[3].shape == (B, C) for b in raw)
    return sd0, raw


def batches_of(raw):
    return [(image, ids, label) for image, ids, _, label, _ in raw]


def group_of(name):
    return "backbone" if name.startswith("backbone.") else "hash" if name.startswith("hash.") else "hyp"


def hyper_of(name):
    return dict(ADAM, lr=OPT_CFG["backbone_lr" if group_of(name) == "backbone" else "lr"])


def is_buffer(name):
    return name.rsplit(".", 1)[-1] in BUFFERS


_TOWER_NAMES = {}


def kind_of(name):
    """tensor kind for pooling: tower tensors by tower_grad_cases.kind_of (layers pooled), heads and proxies by their own name"""
    if not name.startswith("backbone."):
        return name
    key = name[len("backbone."):]
    if not _TOWER_NAMES:
        for tower in ("img", "txt"):
            for tn in TC.tensor_names(tower, 8)[1:]:
                _TOWER_NAMES[TC.tensor_key(tower, tn)] = tower + "." + TC.kind_of(tn)
    return _TOWER_NAMES[key]


# ---- the pieces ---------------------------------------------------------------------------------------------------------------
def dcmht_head(x, t, bn, eps=NORM_EPS, mask=None):
    """one DCMHT modality head in train mode, in the dtype of x -> (probs [B, 2K], dict(z: the fc2 pre-activations, n: fc2's input,
    o: the normalisation's input)); t: the head's tensors under its own key names.  mask: the relu decisions to take ([B, 2K] bool)
    in place of z > 0, which is what None takes"""
    e = x.shape[1]
    F = torch.nn.functional
    o = F.linear(F.linear(x, t["atten.in_proj_weight"][2 * e:], t["atten.in_proj_bias"][2 * e:]), t["atten.out_proj.weight"],
                 t["atten.out_proj.bias"])
    if bn:
        n = (o - o.mean(0)) / torch.sqrt(o.var(0, unbiased=False) + eps) * t["norm.weight"] + t["norm.bias"]
    else:
        n = F.layer_norm(o, (e,), t["norm.weight"], t["norm.bias"], eps)
    z = F.linear(n, t["fc2.weight"], t["fc2.bias"])
    f = torch.relu(z) if mask is None else torch.where(torch.as_tensor(mask), z, torch.zeros_like(z))
    return torch.softmax(f.view(f.shape[0], -1, 2), -1).view(f.shape[0], -1), {"z": z, "n": n, "o": o}


def update_bn(buf, o, pre="hash.img_hash.norm."):
    """BatchNorm's running statistics and batch count after a train-mode forward on the normalisation's input o"""
    buf[pre + "running_mean"] = (1 - BN_MOMENTUM) * buf[pre + "running_mean"] + BN_MOMENTUM * o.mean(0)
    buf[pre + "running_var"] = (1 - BN_MOMENTUM) * buf[pre + "running_var"] + BN_MOMENTUM * o.var(0, unbiased=True)
    buf[pre + "num_batches_tracked"] += 1


def tie_bound(n, w):
    """oracle.heads_train: fp32 may put an fc2 pre-activation within this of zero on the other side of the relu"""
    n, w = np.asarray(n, np.float64), np.asarray(w, np.float64)
    return HT.TIE_FACTOR * HT.EPS32 * np.linalg.norm(n, axis=1)[:, None] * np.linalg.norm(w, axis=1)[None, :]


def dsph_head(x, w, b, keep, p=DROP_P):
    return torch.tanh(torch.nn.functional.linear(x, w, b) * keep / (1.0 - p))


def hyp_cosines(x, y, P, labels):
    """every cosine HyP compares with its threshold, float64 numpy: the code-proxy entries off the labels (both modalities) and the
    regulariser pairs of the three terms; nothing is left out"""
    F = torch.nn.functional
    x, y, P = x.detach().double(), y.detach().double(), P.detach().double()
    L = labels != 0
    nP = F.normalize(P, p=2, dim=1)
    out = {"neg": (F.normalize(x, p=2, dim=1) @ nP.T)[~L], "neg_t": (F.normalize(y, p=2, dim=1) @ nP.T)[~L]}
    M = L.sum(1) > 1
    Lm = L[M].double()
    pairs = (Lm @ Lm.T) == 0
    xm, ym = F.normalize(x[M], p=2, dim=1), F.normalize(y[M], p=2, dim=1)
    out.update({"reg": (xm @ xm.T)[pairs], "reg_t": (ym @ ym.T)[pairs], "reg_xt": (xm @ ym.T)[pairs]})
    return {k: v.numpy() for k, v in out.items()}


class Rows:
    """a matrix of which only a few rows are non-zero"""

    def __init__(self, a):
        self.shape, self.dtype = a.shape, a.dtype
        self.idx = np.flatnonzero(a.any(axis=1))
        self.val = a[self.idx].copy()

    def dense(self):
        a = np.zeros(self.shape, self.dtype)
        a[self.idx] = self.val
        return a


def pack(a):
    return Rows(a) if a.ndim == 2 and a.shape[0] > 4096 else a


def dense(a):
    return a.dense() if isinstance(a, Rows) else a


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def run(arch, sd0, batches, steps=STEPS, masks=None, dtype=torch.float64, keep=None):
    """S training steps from the initial state_dict `sd0` on batches[s % len(batches)] = (image, ids, labels), in `dtype`.  masks
    (DSPH): per step (keep_img, keep_txt), [B, K] of 0 / 1.  -> list over the steps of `keep(s, record)` (the record itself without
    `keep`); a record holds, per parameter name, numpy arrays of `dtype`:
      grad (before clipping), clipped (what BertAdam leaves in p.grad), p (after the step), m, v (next_m / next_v),
    and loss, lr (the rate each group stepped with), next_lr (what get_lr() reports afterwards), count (BertAdam's step counter),
    buffers (BatchNorm's running_mean / running_var / num_batches_tracked), proxy_buf (SGD's momentum buffer), and for the conditions
    z / tie (fc2 pre-activations of both DCMHT heads and their tie bound) and cos (hyp_cosines)."""
    np_dtype = np.float64 if dtype == torch.float64 else np.float32
    out = []
    with DC.one_thread():
        t = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd0.items() if v.is_floating_point() and not is_buffer(k)}
        buf = {k: (v.detach().to(dtype).clone() if v.is_floating_point() else int(v)) for k, v in sd0.items() if is_buffer(k)}
        adam = [k for k in t if group_of(k) != "hyp"]
        m = {k: np.zeros(tuple(t[k].shape), np_dtype) for k in adam}
        v = {k: np.zeros(tuple(t[k].shape), np_dtype) for k in adam}
        sgd = torch.optim.SGD([t["hyp.proxies"]], **HYP_CFG) if arch == "DSPH" else None
        for s in range(steps):
            image, ids, labels = batches[s % len(batches)]
            for x in t.values():
                x.grad = None
            rec = _forward(arch, t, buf, image.to(dtype), ids, labels, None if masks is None else masks[s], dtype)
            rec["loss_t"].backward()
            rec["loss"] = float(rec.pop("loss_t").detach())
            assert t["backbone.logit_scale"].grad is None
            for kind in QUANTITIES[:2] + ("p",) + QUANTITIES[3:]:
                rec[kind] = {}
            rec["lr"], rec["next_lr"] = {}, {}
            for k in adam:
                if t[k].grad is None:
                    continue
                h = hyper_of(k)
                g = t[k].grad.numpy().copy()
                rec["lr"][group_of(k)], rec["next_lr"][group_of(k)] = AC.lr_f64(h, s), AC.lr_f64(h, s + 1)
                p, m[k], v[k], gc = AC.step_f64(t[k].detach().numpy(), g, m[k], v[k], AC.lr_f64(h, s), h)
                assert p.dtype == m[k].dtype == v[k].dtype == np_dtype
                with torch.no_grad():
                    t[k].copy_(torch.from_numpy(p))
                rec["grad"][k], rec["clipped"][k], rec["p"][k], rec["m"][k], rec["v"][k] = pack(g), pack(np.asarray(gc)), p, pack(m[k]), pack(v[k])
            rec["count"] = s + 1
            if sgd is not None:
                rec["grad"]["hyp.proxies"] = t["hyp.proxies"].grad.numpy().copy()
                sgd.step()
                rec["p"]["hyp.proxies"] = t["hyp.proxies"].detach().numpy().copy()
                rec["proxy_buf"] = sgd.state[t["hyp.proxies"]]["momentum_buffer"].numpy().copy()
            rec["buffers"] = {k: (b.numpy().copy() if torch.is_tensor(b) else b) for k, b in buf.items()}
            out.append(rec if keep is None else keep(s, rec))
    return out


def _forward(arch, t, buf, image, ids, labels, mask, dtype):
    clip = {k[len("backbone."):]: x for k, x in t.items() if k.startswith("backbone.")}
    n = image.shape[0]
    fed = dict(clip, **{k: clip[k].unsqueeze(0).repeat(n, 1, 1) for k in ("visual.proj", "text_projection")})
    e_img, e_txt = enc.clip_image(fed, image), enc.clip_text(fed, ids, None)
    heads = {mod: {k[len("hash.%s_hash." % mod):]: x for k, x in t.items() if k.startswith("hash.%s_hash." % mod)} for mod in ("img", "txt")}
    rec = {}
    if arch == "DCMHT":
        pi, ai = dcmht_head(e_img, heads["img"], True)
        pt, at = dcmht_head(e_txt, heads["txt"], False)
        update_bn(buf, ai["o"].detach())
        rec["z"] = {mod: a["z"].detach().double().numpy() for mod, a in (("img", ai), ("txt", at))}
        rec["tie"] = {mod: tie_bound(a["n"].detach().numpy(), heads[mod]["fc2.weight"].detach().numpy()) for mod, a in (("img", ai), ("txt", at))}
        rec["loss_t"] = DC.terms(pi, pt, labels, K, "euclidean")[0]
    else:
        ci = dsph_head(e_img, heads["img"]["fc.weight"], heads["img"]["fc.bias"], mask[0].to(dtype))
        ct = dsph_head(e_txt, heads["txt"]["fc.weight"], heads["txt"]["fc.bias"], mask[1].to(dtype))
        rec["cos"] = hyp_cosines(ci, ct, t["hyp.proxies"], labels)
        rec["loss_t"] = OL.hyp_terms(ci, ct, t["hyp.proxies"], labels, HYP_MODEL["threshold"], HYP_MODEL["alpha"])["loss"]
    return rec


# ---- conditions, null set, errors ---------------------------------------------------------------------------------------------
def check_conditions(arch, r64):
    """the conditions on the inputs, asserted on the float64 run at every step -> what was measured"""
    out = {}
    for s, rec in enumerate(r64):
        if arch == "DCMHT":
            for mod in ("img", "txt"):
                ratio = np.abs(rec["z"][mod]) / rec["tie"][mod]
                out[(s, mod)] = (float(np.abs(rec["z"][mod]).min()), float(ratio.min()))
                assert rec["z"][mod].shape == (B, 2 * K) and ratio.min() > 1.0, ("fc2 pre-activation inside its tie bound", s, mod, out[(s, mod)])
        else:
            for key, c in rec["cos"].items():
                gap = float(np.abs(c - HYP_MODEL["threshold"]).min()) if c.size else float("inf")
                out[(s, key)] = (int(c.size), gap)
                assert gap >= GAP, ("HyP cosine within GAP of the threshold", s, key, gap)
            assert rec["cos"]["neg"].size == rec["cos"]["neg_t"].size > 0
    return out


def null_set(r64):
    names = [k for k in r64[0]["grad"]]
    return tuple(sorted(k for k in names if all(float(np.abs(dense(rec["grad"][k])).max()) < NULL_G for rec in r64)))


def quantity(rec, kind, name, sd0):
    """a record's tensor of one quantity as a dense numpy array; delta = p - p_initial in the record's dtype"""
    if kind == "delta":
        p = rec["p"][name]
        return p - sd0[name].numpy().astype(p.dtype)
    return dense(rec[kind][name])


def errors(rec, ref, sd0, null=()):
    """rel_err of every tensor of a record against the float64 record: {(quantity, name): e}; proxies have grad and delta, their
    momentum buffer goes as (buf, hyp.proxies), buffers as (buffer, name), the loss as (loss, '')"""
    out = {("loss", ""): abs(rec["loss"] - ref["loss"]) / (abs(ref["loss"]) or 1.0)}
    for kind in QUANTITIES:
        for name in ref[kind] if kind != "delta" else ref["p"]:
            if name not in null:
                out[(kind, name)] = rel_err(quantity(rec, kind, name, sd0), quantity(ref, kind, name, sd0))
    if "proxy_buf" in ref:
        out[("buf", "hyp.proxies")] = rel_err(rec["proxy_buf"], ref["proxy_buf"])
    for name, b in ref["buffers"].items():
        if not isinstance(b, int):
            out[("buffer", name)] = rel_err(rec["buffers"][name], b)
    return out


def pool(per_step):
    """list over steps of `errors` -> {(quantity, kind): the largest over the steps and layers}"""
    out = {}
    for errs in per_step:
        for (q, name), e in errs.items():
            key = (q, kind_of(name) if name else "")
            out[key] = max(out.get(key, 0.0), e)
    return out


def yardstick(arch, sd0, batches, r64, masks=None, null=()):
    """the float32 restatement against the float64 one on these very inputs -> (per-step `errors`, their pool, per step the float32
    run's max|g| of every null tensor)"""
    def keep(s, rec):
        return errors(rec, r64[s], sd0, null), {n: float(np.abs(dense(rec["grad"][n])).max()) for n in null}
    got = run(arch, sd0, batches, len(r64), masks, torch.float32, keep)
    return [g[0] for g in got], pool([g[0] for g in got]), [g[1] for g in got]


def cpu_masks(seed=7, steps=STEPS):
    """DSPH keep masks for the CPU module: p = 0.2, seeded"""
    g = torch.Generator().manual_seed(seed)
    return [tuple((torch.rand(B, K, generator=g) >= DROP_P) for _ in range(2)) for _ in range(steps)]


def table(what, e_ref, e_port=None):
    """the lines of the e_port / e_ref table (e_ref alone without a port)"""
    lines = []
    for key in sorted(e_ref):
        if e_port is None:
            lines.append("%s %-6s %-40s e_ref %.2e" % (what, key[0], key[1], e_ref[key]))
        elif key in e_port:
            ratio = e_port[key] / e_ref[key] if e_ref[key] > 0 else (0.0 if e_port[key] == 0 else float("inf"))
            lines.append("%s %-6s %-40s e_port %.2e  e_ref %.2e  ratio %.2f" % (what, key[0], key[1], e_port[key], e_ref[key], ratio))
    return lines
