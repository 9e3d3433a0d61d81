"""Shared by tests/test_umoed_train_step_cpu.py and tests/test_gpu_umoed_train_step.py (not a test module): the whole training step of
UMoEDTrainer.train_epoch_decoder (the shared _train_epoch over UMoED.forward_train) -- both CLIP towers with their token outputs, the image
tokens with the cls row first, the ONE decoder head (`hash_module`, fusion) called twice, on the 5 image tokens and then on the 32 text
tokens that include the padded rows, each call with its own keep masks at the six dropout sites of every layer, the pairwise objective, the
backward through all of it (the head's 1 + 19 layers + 2 parameter gradients are the sum of the two calls'), BertAdam over the backbone and
head groups -- restated for S steps in the dtype it is handed, the configuration of the two cases, the conditions their inputs must meet,
and the error measure.  Built on tests/dimch_train_step_cases.py, whose helpers it uses and does not copy.

The restatement composes only functions that a golden file pins to the reference: oracle.encode.clip_image / clip_text with
return_patches=True over a state_dict of leaves, fed as dimch_train_step_cases.run feeds them (the projections repeated over the batch; the
text call takes no key padding mask and every one of the 32 token rows is read), umoed_train_cases.forward_train once per modality over the
same head leaves with that call's keep masks and the configuration's p (its probe of the ReLU pre-activations kept),
umoed_cases.objective_terms with the configuration's constants (its probe kept), umoed_cases.linear_subspace_bits for the codes, and
bertadam_cases.step_f64 / lr_f64.  Parameters are assigned to their optimiser group by name (backbone.* -> backbone_lr, hash.* -> lr), never
read from the trainer.  Float64 is the oracle; float32, with the parameters stored in float32 between the steps, is the yardstick.  Every
run uses one CPU thread.  Keep masks are handed in and never drawn here: before step s the head's generator is
torch.Generator(device).manual_seed(MASK_SEED + s), and `draw_masks` replays the head's two bernoulli_(1 - p) draws of that step, image
then text, on an identically seeded generator of the same device, then cuts each flat buffer into the six sections of every layer
(umoed_train_cases.keep_shapes; umoed_train_cases.flat_keep of the cut is the buffer again).

The cases.  Trainer settings of train_step_cases: B = 4, C = 6, train_num 12 so that three batches cycle, max_word 32, image_resolution 64,
shuffle off, optimizer {lr 0.002, backbone_lr 0.0005, e 1e-3}, epochs = S = 5, each step its own train_epoch_decoder call on one batch, so
t_total = 5 and step 0 runs at rate 0; batches 0 and 1 come round again at steps 3 and 4.  Both cases: fusion, MoE, linear_subspace with
concatenate, unif_alpha 0.8, token_triplet_margin 0.1, triplet_alpha 1 (the reference's configuration).  `small`: one block per tower at
embed_dim = hidden_dim 64, output_dim 4 over setDim 4 (V = 2), one decoder layer of one head, 2 x 2 expert slots, dim_feedforward 24,
dropout 0.3, extreme with extreme_T 0.3, the head as the module's own init laws leave it (what a real run starts from).  `deep`: two blocks
per tower at 128, output_dim 24 over setDim 6 (V = 16: a 24-bit code that is no multiple of 16), two layers of two heads, 3 x 5 slots,
dim_feedforward 40, dropout 0 (no mask is drawn), the plain-cosine route (extreme False), and the head's state_dict strictly loaded from
umoed_cases.head_params(spec, HEAD_SEED) before anything is captured: under the module's own init the experts' weights have the bound
1 / sqrt(F d), the Soft-MoE branch barely moves the residual stream and a wrong expert or phi gradient would sit in the noise.

Conditions on the inputs (check_conditions; none involves the port), asserted on the float64 run.  For every kink the margin is the float64
distance from the kink, the noise the largest |float32 - float64| of that same quantity over the steps, and margin > TOL_FACTOR = 4 noise
is asked.  1 every ReLU pre-activation of every layer and both calls; besides margin >= RELU_GAP max|pre| of its tensor
(umoed_train_cases' guard), and the float32 run takes every float64 decision.  2 the hinge argument of every live triplet (`kinks`, whose
smallest is checked against objective_terms' own probe), guard 1e-5.  3 every similarity under the clamp, guard 1e-5.  4 the gap between
the two largest logits of every embeds row, and umoed_cases.head_gap >= HEAD_GAP, so that every code bit can be compared.  5 each of the two
triplet terms has a live summand (above 1e-16, the reference's count) at every step.  6 every batch row has a label.  7 with p = 0.3 every
mask section keeps a share in (0.5, 0.9), the image and the text masks differ and so do those of different steps.  8 no tensor's max|g64|
over the run lies between NULL_G and 1e3 NULL_G.  9 so that the yardstick cannot hide a failure, the float32 restatement's worst
per-tensor gradient error is at most GRAD_CAP = 1e-4 at every step.

Error measure.  That of train_step_cases: rel_err = max|x - f64| / max|f64| per tensor, parameters as delta = p - p_initial, pooled per
quantity and tensor kind over steps and layers (`kind_of`: tower tensors by train_step_cases.kind_of, head tensors by
umoed_train_cases.kind, the layer index removed); the four head outputs go as (codes, <name>), the five terms relative to the largest as
(terms, '').

Three kinds are pooled wider than that, because the float32 yardstick of one such tensor cannot carry a factor of 4 (the problem the MITH
and DIMCH modules describe): (a) grad, clipped, m and v of the head's bias-like tensors (every bias and the LayerNorm gains: sums over all
B M rows with cancellation) pool as hash.hash_module.<bias>; (b) the delta of all head tensors pools as hash.hash_module (biases start at
zero, their delta is -lr m / (sqrt(v) + e) alone, and where sqrt(v) is of the size of e = 1e-3 an error of m that is small against max|m|
is divided by it); (c) m and v of the text tower pool as txt.<tower> (the token embedding's rows that one batch touches once, and biases
behind 32 token rows of which most are padding).  The figures: on the inputs and the device's masks of `small`, two float32 runs of this
very restatement on two CPUs (the MI355X host's and another) give, a tensor kind at a time, for m of classifier.bias 1.02e-5 and 7.86e-5,
of norm2.bias 1.01e-5 and 5.71e-5, of norm3.bias 1.03e-5 and 5.26e-5, for v of the token embedding 1.98e-6 and 1.05e-5, of the text
tower's mlp.c_fc.bias 6.35e-6 and 2.68e-5 -- factors of 4 to 8, where the port's own errors (2.06e-5, 1.80e-5, 1.71e-5, 6.33e-6, 1.15e-5)
are 1.7 to 3.2 times the one and 0.3 to 0.6 times the other; as first written, a kind per tensor, the module passed with its worst ratio
at 3.21 (v of the token embedding), which rested on that accident.  Pooled as above the same two runs give 1.15e-5 and 7.86e-5 (m) and
1.15e-5 and 3.68e-5 (grad) for (a), 5.73e-5 and 5.73e-5 for (b), 5.2e-6 and 1.40e-5 (m), 8.3e-6 and 2.72e-5 (v) for (c), and the port's
worst ratio against the smaller of each is 1.79.  What is left of the disagreement is no accident of one tensor: the second CPU's float32
run as a whole leaves the float64 trajectory further at step 3 of `small` (its worst gradient error there is 3.7e-5 against 7.0e-6; the
median disagreement over the 200 kinds of `small` is 1.22, 38 of them above 2, all with the second CPU the larger; `deep`: median 1.12, none
above 1.9), so no pooling removes it, and the smaller yardsticks, which are the MI355X host's, are the ones the figures of
tests/test_gpu_umoed_train_step.py are measured against.  The factor stays 4."""
import re

import numpy as np
import torch

import bertadam_cases as AC
import dimch_train_step_cases as DS
import train_step_cases as TS
import umoed_cases as UC
import umoed_train_cases as UT
from oracle import encode as enc

STEPS = TS.STEPS
DATA_SEED = 1821                     # the dataset's seed: the first from 1814 on that meets the conditions of both cases (see
                                     # tests/test_umoed_train_step_cpu.py for what the skipped ones missed)
MASK_SEED = 1814                     # the head's generator is seeded MASK_SEED + s before step s
HEAD_SEED = 1814                     # `deep`: umoed_cases.head_params(spec, HEAD_SEED) is loaded into the head
B, C, TRAIN_NUM = DS.B, DS.C, DS.TRAIN_NUM
OPT_CFG, ADAM = TS.OPT_CFG, TS.ADAM
TOL_FACTOR = 4.0
NULL_G = TS.NULL_G
GRAD_CAP = 1e-4
QUANTITIES = TS.QUANTITIES
MODS = ("img", "txt")
TERMS = UC.TERMS
OUTS = ("img_embeds", "img_hash", "txt_embeds", "txt_hash")
GUARD = {"hinge": 1e-5, "clamp": 1e-5}                                # umoed_cases.guarded's
HEAD = "hash.hash_module."
_CLIP = "vision_layers=%d,transformer_layers=%d,vision_width=128,transformer_width=128,embed_dim=%d,image_resolution=64"
_CONSTS = dict(token_triplet_margin=0.1, triplet_alpha=1.0, unif_alpha=0.8)
CASES = {
    "small": dict(clip=_CLIP % (1, 1, 64), E=64, K=4, setDim=4, heads=1, layers=1, n=2, p=2, F=24, dropout=0.3, load_head=False,
                  consts=dict(_CONSTS, extreme=True, extreme_T=0.3)),
    "deep": dict(clip=_CLIP % (2, 2, 128), E=128, K=24, setDim=6, heads=2, layers=2, n=3, p=5, F=40, dropout=0.0, load_head=True,
                 consts=dict(_CONSTS, extreme=False, extreme_T=0.3)),
}
rel_err = AC.rel_err
Rows, pack, dense = TS.Rows, TS.pack, TS.dense
table = TS.table
group_of, hyper_of = DS.group_of, DS.hyper_of
no_grad_set, null_set, quantity = DS.no_grad_set, DS.null_set, DS.quantity
assert CASES["small"]["consts"] == UC.CONFIG and set(CASES["deep"]["consts"]) == set(UC.CONST_KEYS)
assert (OPT_CFG["lr"], OPT_CFG["backbone_lr"], OPT_CFG["e"]) == (0.002, 0.0005, 1e-3) and STEPS == 5


# ---- configuration ------------------------------------------------------------------------------------------------------------
def spec_of(case, T=None):
    """the head of a case in the keys of umoed_cases / umoed_train_cases (p: slots per expert); T: the token rows of one call"""
    c = CASES[case]
    return dict(B=B, T=T, E=c["E"], d=c["E"], heads=c["heads"], M=c["setDim"], layers=c["layers"], n=c["n"], p=c["p"], F=c["F"],
                V=2 ** (c["K"] // c["setDim"]), moe=True, hash_func="linear_subspace")


def config(case, out_dir, device, data_seed=DATA_SEED):
    c = CASES[case]
    k = c["consts"]
    return {
        "model": {"arch": "UMoED", "clip_path": "synthetic:1814:" + c["clip"], "setDim": c["setDim"], "dropout": c["dropout"],
                  "extreme": k["extreme"], "extreme_T": k["extreme_T"], "triplet": True, "distance_mode": "cosine", "MoE": True, "fusion": True,
                  "num_experts": c["n"], "slots_per_expert": c["p"], "hash_func": "linear_subspace", "merge_func": "concatenate",
                  "decoder_heads": c["heads"], "decoder_layers": c["layers"], "hidden_dim": c["E"], "dim_feedforward": c["F"], "seed": 1814,
                  "distance": {"mode": "pairwise"}, "chamfer": {n: k[n] for n in ("unif_alpha", "token_triplet_margin")},
                  "hash_pars": {"triplet_alpha": k["triplet_alpha"], "triplet_margin": 0.3}},
        "dataset": {"arch": "synthetic", "name": "synth", "num_classes": C, "retrieval_num": 16, "max_word": 32, "image_resolution": 64,
                    "seed": data_seed},
        "optimizer": dict(OPT_CFG),
        "run": {"arch": "UMoEDTrainer", "output_dim": c["K"], "device": device, "batch_size": B, "num_workers": 0, "is_train": True,
                "query_num": 8, "train_num": TRAIN_NUM, "epochs": STEPS, "shuffle": False, "save_dir": str(out_dir), "log_dir": str(out_dir),
                "seed": 1814},
    }


def trainer(case, out_dir, device, data_seed=DATA_SEED):
    """the runner of a case, its log lines collected in `.lines`; in `deep` the head's state_dict strictly loaded from
    umoed_cases.head_params"""
    import types
    import xmh.models  # noqa: F401
    import xmh.runners  # noqa: F401
    from xmh.common.register import registry
    from xmh.utils.config import Config
    t = registry.get_runner_class("UMoEDTrainer").from_config(cfg=Config(config(case, out_dir, device, data_seed)), autorun=False)
    t.lines = []
    t.logger = types.SimpleNamespace(info=t.lines.append)
    if CASES[case]["load_head"]:
        P = UC.head_params(spec_of(case), HEAD_SEED)
        t.model.hash.hash_module.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in P.items()}, strict=True)
    return t


def capture(t, case):
    """everything the restatement needs of a trainer, on the CPU: dict(case, sd0: the parameters by name, raw: the loader's batches as it
    yields them, consts / p: of the configuration, spec: spec_of, T: token rows per call)"""
    c = CASES[case]
    sd0 = {n: p.detach().cpu().clone() for n, p in t.model.named_parameters()}
    raw = list(t.train_loader)
    assert len(raw) == TRAIN_NUM // B == 3
    for image, ids, kpm, label, index in raw:
        assert image.shape == (B, 3, 64, 64) and ids.shape == (B, 32) and label.shape == (B, C) and index.shape == (B,)
    assert sorted(int(i) for b in raw for i in b[4]) == list(range(TRAIN_NUM))
    spec = spec_of(case)
    shapes = UC.head_shapes(spec)
    assert sorted(HEAD + k for k in shapes) == sorted(n for n in sd0 if n.startswith("hash.")) and len(shapes) == 1 + 19 * c["layers"] + 2
    assert all(tuple(sd0[HEAD + k].shape) == tuple(s) for k, s in shapes.items())
    head = t.model.hash.hash_module
    assert t.model.hash.fusion and float(head.dropout_p) == c["dropout"] and head.code_width == c["K"]
    assert all(n.startswith("backbone.") or n.startswith(HEAD) for n in sd0)
    return dict(case=case, sd0=sd0, raw=raw, consts=dict(c["consts"]), p=c["dropout"], spec=spec, T={"img": 5, "txt": 32})


_BIAS_LIKE = re.compile(r"(bias|norm\d\.weight)$")


def kind_of(name, quantity=None):
    """tensor kind for pooling: tower tensors by train_step_cases.kind_of, head tensors by umoed_train_cases.kind (no layer index); pooled
    wider, for the reason in the module's docstring: the delta of the head's tensors as one kind, and its bias-like tensors as one kind in
    the other quantities"""
    if not name.startswith("hash."):
        kind = TS.kind_of(name)
        return "txt.<tower>" if quantity in ("m", "v") and kind.startswith("txt.") else kind
    if quantity == "delta":
        return HEAD[:-1]
    if quantity in ("grad", "clipped", "m", "v") and _BIAS_LIKE.search(name):
        return HEAD + "<bias>"
    return UT.kind(name)


def pool(per_step):
    """list over steps of `errors` -> {(quantity, kind): the largest over the steps, the layers and the tensors of a kind}"""
    out = {}
    for errs in per_step:
        for (q, name), e in errs.items():
            key = (q, kind_of(name, q) if name else "")
            out[key] = max(out.get(key, 0.0), e)
    return out


# ---- keep masks ---------------------------------------------------------------------------------------------------------------
def split_keep(flat, spec):
    """the head's one buffer -> [layers][6] uint8 arrays in umoed_train_cases.keep_shapes' shapes"""
    flat = np.asarray(flat, np.uint8).reshape(-1)
    shapes = UT.keep_shapes(spec)
    out, at = [], 0
    for _ in range(spec["layers"]):
        layer = []
        for s in shapes:
            n = int(np.prod(s))
            layer.append(flat[at:at + n].reshape(s).copy())
            at += n
        out.append(layer)
    assert at == flat.size, (at, flat.size)
    assert np.array_equal(UT.flat_keep(out), flat)
    return out


def draw_masks(cap, device="cpu", steps=STEPS, seed=MASK_SEED):
    """per step (masks of the image call, masks of the text call), each [layers][6] uint8 numpy, or None for a case without dropout:
    the head's own two torch.empty(n, uint8).bernoulli_(1 - p, generator=g) draws, image then text, g = torch.Generator(device) seeded
    seed + s"""
    if cap["p"] <= 0.0:
        return None
    out = []
    for s in range(steps):
        g = torch.Generator(device=device).manual_seed(seed + s)
        step = []
        for mod in MODS:
            spec = dict(cap["spec"], T=cap["T"][mod])
            n = sum(int(np.prod(x)) for x in UT.keep_shapes(spec)) * spec["layers"]
            flat = torch.empty(n, dtype=torch.uint8, device=device).bernoulli_(1.0 - cap["p"], generator=g)
            step.append(split_keep(flat.cpu().numpy(), spec))
        out.append(tuple(step))
    return out


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def kinks(e_img, e_txt, labels, cst):
    """the arguments of the objective's kinks from the two embeds (numpy, computed in their dtype), for the conditions: dict(hinge: the
    two [B, B, B] arrays of D[a][p] - D[a][n] + margin, NaN where the triplet is not live (mask 0 or weight 0), clamp: the dot
    products [B, M, B] under clamp(min=0), live: per direction the number of summands above 1e-16) -- the operations of
    umoed_cases.objective_terms / triplet_term, whose probe `run` checks the smallest of each against"""
    F = torch.nn.functional
    e_img, e_txt = torch.as_tensor(e_img), torch.as_tensor(e_txt)
    dtype = e_img.dtype
    lab = torch.as_tensor(labels).to(dtype)
    x, y = F.normalize(e_img, dim=-1), F.normalize(e_txt, dim=-1)
    a, b = (torch.softmax(x / cst["extreme_T"], dim=-1), torch.softmax(y / cst["extreme_T"], dim=-1)) if cst["extreme"] else (x, y)
    dots = torch.einsum("btl,ktl->btk", a, b)
    D = (1 - dots.clamp(min=0)).mean(dim=1)
    n = D.shape[0]
    so = lab @ lab.t()
    sim = (so > 0).to(dtype)
    ideal = torch.sort(so, dim=1, descending=True)[0]
    Z = ((2 ** ideal - 1) / torch.log2(torch.arange(0.0, n) + 2).repeat(n, 1)).sum(1).reshape(-1, 1)
    w = (2 ** so - 1) / Z
    mask = sim.unsqueeze(2) * (1 - sim.unsqueeze(1))
    weight = w.unsqueeze(2) - w.unsqueeze(1)
    live = (mask > 0) & (weight != 0)
    hinge, count = [], []
    for Dd in (D, D.t()):
        t = Dd.unsqueeze(2) - Dd.unsqueeze(1) + cst["token_triplet_margin"]
        hinge.append(torch.where(live, t, torch.full_like(t, float("nan"))).double().numpy())
        count.append(int((weight * mask * t).clamp(0).gt(1e-16).sum()))
    return {"hinge": hinge, "clamp": [dots.double().numpy()], "live": count}


def run(cap, masks, steps=STEPS, dtype=torch.float64, keep=None, detach=None):
    """S training steps from cap["sd0"] on cap["raw"][s % 3] in `dtype`.  masks: draw_masks' list, or None (no dropout).  detach: "img"
    or "txt" cuts that call's embeds off the graph before the objective (what is left is the other call's contribution).  -> list over
    the steps of `keep(s, record)` (the record itself without `keep`); a record holds, per parameter name, numpy arrays of `dtype`:
      grad (before clipping), clipped (what BertAdam leaves in p.grad), p (after the step), m, v (next_m / next_v),
    and loss, terms (the five of umoed_cases.TERMS), lr (the rate each group stepped with), next_lr (what get_lr() reports afterwards),
    count (BertAdam's step counter), outs (the four head outputs in compute_loss's order, detached), pre (per modality the ReLU
    pre-activations of every layer, float64 numpy), probe (objective_terms' probe), trace (`kinks`), labels, buffers (none)."""
    npd = np.float64 if dtype == torch.float64 else np.float32
    cst, out = cap["consts"], []
    with TS.DC.one_thread():
        t = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in cap["sd0"].items()}
        W = {k: t[HEAD + k] for k in UC.head_shapes(cap["spec"])}
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
                probe = []
                e = UT.forward_train(tokens[mod], W, dict(cap["spec"], T=cap["T"][mod]), None if masks is None else masks[s][i], cap["p"], probe)
                o[mod + "_embeds"], o[mod + "_hash"] = e, UC.linear_subspace_bits(e.detach())
                pre[mod] = [z.double().numpy().copy() for z in probe]
                assert len(probe) == cap["spec"]["layers"]
            probe = {}
            e_i, e_t = (o[mod + "_embeds"].detach() if detach == mod else o[mod + "_embeds"] for mod in MODS)
            terms = UC.objective_terms(e_i, e_t, torch.as_tensor(label), cst, probe)
            terms[0].backward()
            trace = kinks(o["img_embeds"].detach(), o["txt_embeds"].detach(), label, cst)
            if "hinge" in probe:                                                         # absent: no live triplet (the conditions refuse it)
                assert abs(np.nanmin(np.abs(np.stack(trace["hinge"]))) - probe["hinge"]) <= 1e-6 * probe["hinge"] + 1e-12
            else:
                assert np.isnan(np.stack(trace["hinge"])).all()
            assert abs(np.abs(trace["clamp"][0]).min() - probe["clamp"]) <= 1e-6 * probe["clamp"] + 1e-12
            rec = {"loss": float(terms[0].detach()), "terms": terms.detach().double().numpy().copy(), "outs": [o[k].detach().numpy().copy() for k in OUTS],
                   "pre": pre, "probe": probe, "trace": trace, "labels": np.asarray(label).copy(), "lr": {}, "next_lr": {}, "count": s + 1,
                   "buffers": {}}
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


# ---- conditions, errors -------------------------------------------------------------------------------------------------------
def _top_gap(e):
    top = np.sort(np.asarray(e, np.float64), axis=-1)
    return top[..., -1] - top[..., -2]


def check_conditions(cap, r64, r32, masks):
    """the conditions on the inputs, asserted on the float64 run (r32: the float32 run on the same masks) -> what was measured:
    kink name -> (margin, noise) over the run (hinge, clamp, gap_<mod>, relu_<mod>_<layer>), (step, 'live') -> the two live counts,
    (step, 'relu') -> decisions that differ in float32, (step, 'labels') -> labels per row, (step, 'head_gap') -> umoed_cases.head_gap
    of the two embeds, (step, 'kept') -> the smallest and largest kept share of a mask section, 'grad_cap' -> the float32 run's worst
    per-tensor gradient error at each step"""
    out = {}
    for k in ("hinge", "clamp"):
        out[k] = DS._margin_noise([a for r in r64 for a in r["trace"][k]], [a for r in r32 for a in r["trace"][k]])
    for i, mod in enumerate(MODS):
        out["gap_" + mod] = DS._margin_noise([_top_gap(r["outs"][2 * i]) for r in r64], [_top_gap(r["outs"][2 * i]) for r in r32])
        for layer in range(cap["spec"]["layers"]):
            key = "relu_%s_%d" % (mod, layer)
            out[key] = DS._margin_noise([r["pre"][mod][layer] for r in r64], [r["pre"][mod][layer] for r in r32])
            for s, r in enumerate(r64):
                z = np.abs(r["pre"][mod][layer])
                assert z.min() >= UT.RELU_GAP * z.max(), ("a ReLU pre-activation inside umoed_train_cases' guard", s, key, z.min(), z.max())
    for s, (a, b) in enumerate(zip(r64, r32)):
        live = [int(x) for x in a["trace"]["live"]]
        out[(s, "live")] = live
        assert len(live) == 2 and min(live) >= 1, ("a triplet term without a live summand", s, live)
        out[(s, "relu")] = sum(int(((x > 0) != (y > 0)).sum()) for mod in MODS for x, y in zip(a["pre"][mod], b["pre"][mod]))
        assert out[(s, "relu")] == 0, ("the float32 restatement takes another ReLU decision", s, out[(s, "relu")])
        out[(s, "labels")] = a["labels"].sum(1).astype(int).tolist()
        assert a["labels"].shape == (B, C) and min(out[(s, "labels")]) >= 1, ("a batch row without a label", s)
        out[(s, "head_gap")] = [UC.head_gap(a["outs"][0]), UC.head_gap(a["outs"][2])]
        assert min(out[(s, "head_gap")]) >= UC.HEAD_GAP, ("two largest logits of a row inside umoed_cases' guard", s, out[(s, "head_gap")])
        assert all(np.array_equal(x, y) for x, y in zip(a["outs"][1::2], b["outs"][1::2])), ("the float32 restatement has another code", s)
    if cap["p"] > 0.0:
        assert masks is not None and len(masks) >= len(r64)
        for s, step in enumerate(masks[:len(r64)]):
            shares = [float(sec.mean()) for call in step for layer in call for sec in layer]
            out[(s, "kept")] = [min(shares), max(shares)]
            assert 0.5 < min(shares) and max(shares) < 0.9, ("a mask section's kept share outside (0.5, 0.9)", s, out[(s, "kept")])
            assert all(not np.array_equal(step[0][y][j], step[1][y][j]) for y in range(cap["spec"]["layers"]) for j in (0, 1, 3, 4, 5)), \
                ("the image and the text call share a mask section", s)                       # section 2 differs in shape: [.., M, T]
            if s:
                assert all(not np.array_equal(UT.flat_keep(step[i]), UT.flat_keep(masks[s - 1][i])) for i in range(2)), ("two steps share a mask", s)
    else:
        assert masks is None
    for k, (margin, noise) in [(k, v) for k, v in out.items() if isinstance(k, str)]:
        assert margin > TOL_FACTOR * noise, ("a kink within TOL_FACTOR float32 differences", k, margin, noise)
        assert margin >= GUARD.get(k, 0.0), ("a kink inside umoed_cases' guard", k, margin, GUARD[k])
    for k in r64[0]["grad"]:
        big = max(float(np.abs(dense(rec["grad"][k])).max()) for rec in r64)
        assert not NULL_G <= big <= 1e3 * NULL_G, ("a tensor between null and not null", k, big)
    null = null_set(r64)
    out["grad_cap"] = [max(rel_err(dense(b["grad"][k]), dense(a["grad"][k])) for k in a["grad"] if k not in null) for a, b in zip(r64, r32)]
    assert max(out["grad_cap"]) <= GRAD_CAP, ("the float32 restatement's gradient error is above the cap", out["grad_cap"])
    return out


def condition_lines(what, cond):
    lines = []
    for key, v in cond.items():
        if key == "grad_cap":
            lines.append("%s condition grad_cap  float32 worst gradient error per step %s  cap %.0e" % (what, " ".join("%.2e" % e for e in v), GRAD_CAP))
        elif isinstance(key, str):
            lines.append("%s condition %-12s margin %.3e  noise %.3e  ratio %.1f  guard %.0e" % (what, key, v[0], v[1], v[0] / v[1] if v[1] else np.inf,
                                                                                             GUARD.get(key, 0.0)))
        else:
            lines.append("%s condition step %d %s %s" % (what, key[0], key[1], v))
    return lines


def errors(rec, ref, sd0, null=()):
    """train_step_cases.errors and, on top, the five terms relative to the largest as (terms, '') and the four head outputs as
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
