"""Cases and restatement of DNPH's training objective (reference models/DNPH/loss/loss.py:12-33, models/DNPH/DNPH.py:72-99) and of
its head, shared by tests/test_dnph_cpu.py, tests/test_gpu_dnph_loss.py, tests/test_gpu_dnph_train.py and tools/make_golden_dnph.py.

The restatement is written from the reference's expressions, in torch on the CPU with torch's autograd for the gradients, with the
dtype as a parameter: float64 is the truth the GPU tests compare with, float32 on the same inputs is the yardstick (e_ref).

  objective   u = normalize(cat(f_img, f_txt)), q = normalize(P); D = sum_k (u - q)^2 (a sum of squared differences, as the kernel
              forms it; the reference's torch.cdist ** 2 is the same number) + mrg on the rows' own classes;
              p_loss = mean_n sum_c -l log_softmax(-D); d_loss_m = CE(p_m, argmax l); noise_m = mean_b sum_k f_m noise_m;
              loss = p_loss + d_loss_img + d_loss_txt - noise_alpha (noise_img + noise_txt)
              -> terms [6] (loss, p_loss, d_loss_img, d_loss_txt, noise_img, noise_txt) and the gradients of up * loss
  head        tanh(keep * (x W^T + b) / (1 - p)) and x Wp^T + bp per modality, then the objective (chain)

Error rule (tests/test_gpu_tower_grad.py's): per tensor e = max|got - f64| / max|f64|; the port must stay within TOL_FACTOR *
max(pool, e_ref), e_ref the float32 restatement's e on the same inputs and pool the largest e_ref of that tensor kind over CASES."""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

TOL_FACTOR = 4.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dnph.npz")
GOLDEN_CASES = {"small": dict(B=7, K=16, C=5, Cp=80, seed=5201), "mid": dict(B=37, K=48, C=33, Cp=80, seed=5202)}

# name -> B, K, C (proxies), Cp (class logits), mrg, noise_alpha, upstream.  B = 1, 37, 65, 257: one row, less than a wave of rows, a
# wave and one, more than one 256-row chunk of the proxy blocks (2B = 514: three chunks); K = 16, 48, 130: less than a wave of
# columns, not a multiple of 64, more than two lanes' worth; C = 1, 24, 32, 33, 80: one class, label-word edges; Cp = C and 80 > C.
# zero: row 2 of the image codes is all zero (F.normalize's eps branch: its gradient is du / 1e-12).
CASES = {
    "b1_k16_c1": dict(B=1, K=16, C=1, Cp=1, mrg=1.0, alpha=0.1, up=1.0, seed=5101),
    "b37_k48_c24": dict(B=37, K=48, C=24, Cp=80, mrg=1.0, alpha=0.1, up=0.37, seed=5102),
    "b65_k130_c32": dict(B=65, K=130, C=32, Cp=32, mrg=1.0, alpha=1.0, up=2.5, seed=5103),
    "b37_k16_c33": dict(B=37, K=16, C=33, Cp=80, mrg=0.5, alpha=0.1, up=1.0, seed=5104),
    "b257_k48_c80": dict(B=257, K=48, C=80, Cp=80, mrg=1.0, alpha=0.1, up=1.0, seed=5105),
    "b65_k16_c33_zero": dict(B=65, K=16, C=33, Cp=33, mrg=1.0, alpha=0.1, up=1.0, seed=5106, zero=True),
    "b37_k48_c24_mrg50": dict(B=37, K=48, C=24, Cp=80, mrg=50.0, alpha=0.1, up=1.0, seed=5107),
}
TERMS = ("loss", "p_loss", "d_loss_img", "d_loss_txt", "noise_img", "noise_txt")
GRADS = ("g_f_img", "g_f_txt", "g_p_img", "g_p_txt", "g_P")
KINDS = ("term", "g_f", "g_p", "g_P", "nz_f")        # nz_f: a code gradient with the eps-branch row zeroed on both sides
ZERO_ROW = 2


def rel_err(got, want):
    """max|got - want| / max|want| (absolute where the reference tensor is identically zero)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = np.abs(want).max() if want.size else 0.0
    return float(np.abs(got - want).max() / (scale if scale > 0 else 1.0)) if want.size else 0.0


# ---- restatement -------------------------------------------------------------------------------------------------------------------
def objective_terms(f_img, f_txt, p_img, p_txt, P, labels, mrg, alpha, noise_img=None, noise_txt=None):
    """torch tensors of one dtype (labels: 0 / 1 of any dtype) -> the six terms, a tensor with a graph"""
    dtype = f_img.dtype
    lab = (torch.as_tensor(labels) == 1).to(dtype)
    u = F.normalize(torch.cat((f_img, f_txt), 0), p=2, dim=-1)
    q = F.normalize(P, p=2, dim=-1)
    D = ((u[:, None, :] - q[None, :, :]) ** 2).sum(-1)
    l2 = torch.cat((lab, lab), 0)
    D = D + mrg * l2
    p_loss = torch.sum(-l2 * F.log_softmax(-D, 1), -1).mean()
    t = torch.argmax(lab, -1)
    d_img, d_txt = F.cross_entropy(p_img, t), F.cross_entropy(p_txt, t)
    zero = torch.zeros((), dtype=dtype)
    n_img = zero if noise_img is None else (f_img * noise_img.to(dtype)).sum(-1).mean()
    n_txt = zero if noise_txt is None else (f_txt * noise_txt.to(dtype)).sum(-1).mean()
    loss = p_loss + (d_img + d_txt) - alpha * (n_img + n_txt)
    return torch.stack([loss, p_loss, d_img, d_txt, n_img, n_txt])


def objective(c, dtype, mrg=None, alpha=None, up=None, noise=True):
    """case dict (numpy inputs) -> {terms..., g_*: gradients of up * loss} as float64 numpy, computed in `dtype`"""
    leaves = {k: torch.tensor(c[k]).to(dtype).requires_grad_(True) for k in ("f_img", "f_txt", "p_img", "p_txt", "P")}
    ns = [torch.tensor(c[k]) if noise else None for k in ("noise_img", "noise_txt")]
    terms = objective_terms(*[leaves[k] for k in ("f_img", "f_txt", "p_img", "p_txt", "P")], torch.tensor(c["labels"]),
                            c["mrg"] if mrg is None else mrg, c["alpha"] if alpha is None else alpha, *ns)
    (terms[0] * (c["up"] if up is None else up)).backward()
    out = {k: terms[i].detach().double().numpy().reshape(1) for i, k in enumerate(TERMS)}
    for g, k in zip(GRADS, ("f_img", "f_txt", "p_img", "p_txt", "P")):
        out[g] = leaves[k].grad.double().numpy()
    return expand(c, out)


def expand(c, vals):
    """what is compared: every term and gradient as it is and, in a case with the all-zero image row, g_f_img again with that row
    zeroed (nz_f_img): the row's du / 1e-12 sets the whole tensor's scale, the other rows are then checked at their own"""
    out = dict(vals)
    if c.get("zero") and vals.get("g_f_img") is not None:
        nz = np.array(vals["g_f_img"], np.float64)
        nz[ZERO_ROW] = 0
        out["nz_f_img"] = nz
    return {k: v for k, v in out.items() if v is not None}


def kind_of(key):
    return "term" if key in TERMS else next(k for k in KINDS if key.startswith(k))


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def draw(B, K, C, Cp, seed, zero=False, **rest):
    """float32 / integer numpy inputs.  Rows by design (where B allows): row 0 has no label, row 1 every label; with `zero`, row 2 of
    the image codes is all zero.  The codes are tanh outputs, the logits of unit-ish scale, the proxies randn / 8 as constructed."""
    rng = np.random.default_rng(seed)
    labels = (rng.random((B, C)) < 0.15).astype(np.int64)
    labels[np.arange(B), rng.integers(0, C, B)] = 1
    if B >= 3:
        labels[0] = 0
        labels[1] = 1
    f = {m: np.tanh(rng.standard_normal((B, K)) * 1.5).astype(np.float32) for m in ("img", "txt")}
    if zero:
        f["img"][ZERO_ROW] = 0.0
    p = {m: (rng.standard_normal((B, Cp)) * 2.0).astype(np.float32) for m in ("img", "txt")}
    P = (rng.standard_normal((C, K)) / 8.0).astype(np.float32)
    noise = {m: (rng.integers(0, 2, (B, K)) * 2 - 1).astype(np.float32) for m in ("img", "txt")}
    return dict(rest, B=B, K=K, C=C, Cp=Cp, seed=seed, zero=zero, labels=labels, f_img=f["img"], f_txt=f["txt"], p_img=p["img"], p_txt=p["txt"],
                P=P, noise_img=noise["img"], noise_txt=noise["txt"])


@functools.lru_cache(maxsize=None)
def build(name):
    return dict(draw(**CASES[name]), name=name)


@functools.lru_cache(maxsize=None)
def reference(name, dtype=torch.float64):
    return objective(build(name), dtype)


@functools.lru_cache(maxsize=None)
def e_ref(name):
    """per tensor: the float32 restatement's error against the float64 one"""
    r64, r32 = reference(name, torch.float64), reference(name, torch.float32)
    return {k: rel_err(r32[k], r64[k]) for k in r64}


@functools.lru_cache(maxsize=None)
def pool():
    """per tensor kind, the largest e_ref over CASES"""
    out = {k: 0.0 for k in KINDS}
    for name in CASES:
        for key, e in e_ref(name).items():
            out[kind_of(key)] = max(out[kind_of(key)], e)
    return out


def compare(what, got, ref64, own):
    """prints e, the yardstick and their ratio for every tensor of `got`, then asserts e <= TOL_FACTOR * max(pool, e_ref) -> worst ratio"""
    rows = []
    for key, g in got.items():
        yard = max(pool().get(kind_of(key), 0.0), own.get(key, 0.0))
        e = rel_err(g, ref64[key])
        rows.append((key, e, yard))
        print("%-22s %-11s e %.3e  yardstick %.3e  ratio %.2f  bound %.3e" % (what, key, e, yard, e / yard if yard else float("inf"),
                                                                               TOL_FACTOR * yard))
    for key, e, yard in rows:
        assert np.asarray(got[key]).shape == ref64[key].shape, (what, key)
        assert e <= TOL_FACTOR * yard, (what, key, e, yard)
    return max((e / yard if yard else float("inf")) for _, e, yard in rows)


# ---- the chain head -> objective ------------------------------------------------------------------------------------------------------
HEAD_PARAMS = ("hash_w", "hash_b", "pre_w", "pre_b")
HEAD_KEYS = {"hash_w": "%s_hash.fc.weight", "hash_b": "%s_hash.fc.bias", "pre_w": "%s_pre.fc.weight", "pre_b": "%s_pre.fc.bias"}
MOD = {"img": "image", "txt": "text"}


def draw_head(seed, K, E, Cp=80):
    """parameters of one modality's two layers away from their initial values, float32"""
    rng = np.random.default_rng(seed)
    u = lambda shape, a: ((rng.random(shape) * 2.0 - 1.0) * a).astype(np.float32)      # noqa: E731
    a = 1.0 / np.sqrt(E)
    return {"hash_w": u((K, E), 1.5 * a), "hash_b": u((K,), 0.1), "pre_w": u((Cp, E), 2.0 * a), "pre_b": u((Cp,), 0.1)}


def chain(x, Pm, keep, P, labels, noises, mrg, alpha, p_drop, dtype):
    """x / Pm / keep / noises: {"img" / "txt": embeddings [B, E] / head parameters / keep mask [B, K] / assigned noise [B, K]}, numpy.
    The whole chain in `dtype` with torch's autograd -> dict: loss, g_x_<m>, g_<param>_<m>, g_P (float64 numpy)"""
    xs = {m: torch.tensor(x[m]).to(dtype).requires_grad_(True) for m in x}
    Ps = {m: {k: torch.tensor(v).to(dtype).requires_grad_(True) for k, v in Pm[m].items()} for m in Pm}
    Pt = torch.tensor(P).to(dtype).requires_grad_(True)
    f, p = {}, {}
    for m in ("img", "txt"):
        z = xs[m] @ Ps[m]["hash_w"].T + Ps[m]["hash_b"]
        f[m] = torch.tanh(z * torch.tensor(keep[m]).to(dtype) / (1.0 - p_drop))
        p[m] = xs[m] @ Ps[m]["pre_w"].T + Ps[m]["pre_b"]
    terms = objective_terms(f["img"], f["txt"], p["img"], p["txt"], Pt, torch.tensor(labels), mrg, alpha, torch.tensor(noises["img"]),
                            torch.tensor(noises["txt"]))
    terms[0].backward()
    out = {"loss": terms[0].detach().reshape(1), "g_P": Pt.grad}
    for m in ("img", "txt"):
        out["g_x_" + m] = xs[m].grad
        for k in HEAD_PARAMS:
            out["g_%s_%s" % (k, m)] = Ps[m][k].grad
    out = {k: v.double().numpy() for k, v in out.items()}
    out["f_img"], out["f_txt"] = f["img"].detach().double().numpy(), f["txt"].detach().double().numpy()
    return out
