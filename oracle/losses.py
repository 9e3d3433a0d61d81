"""TEST INFRASTRUCTURE ONLY -- CPU restatement of the DCMHT loss (reference models/DCMHT/DCMHT.py:72-155) in float64 torch,
and its gradient with respect to the two code matrices by autograd over that restatement (what loss.backward() of
runners/DCMHT/runner.py:124 produces); pinned against the reference's own `our_loss` / its backward by
tests/golden/loss_dcmht.npz (oracle/make_golden_loss.py).  Below it, the same for DSPH's HyP loss (hyp_*, tests/golden/loss_dsph.npz) and
MITH's training objective (mith_*, tests/golden/loss_mith.npz), each with the reader of its fixture.  Only tests/, the golden writers
and oracle/heads_train.py may import this module; it imports neither the reference nor the package."""
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle.fixtures import GOLDEN

DCMHT_CASES = ["b40_k16_euclid", "b40_k64_cos", "b96_k64_euclid", "b17_k32_euclid_nolabels"]
DCMHT_TERMS = ["loss", "intra_pos", "intra_neg", "inter_pos_i", "inter_neg_i", "inter_pos_t", "inter_neg_t", "quan_i", "quan_t"]


def label_sim(labels):
    """common/calc_utils.py:8-10"""
    l = labels.double()
    return (l @ l.t() > 0).double()


def similarity_loss(a, b, lsim, output_dim, vartheta=0.75, threshold=0.1, similarity_function="euclidean"):
    """models/DCMHT/DCMHT.py:72-98 -> (positive_loss, negative_loss)"""
    a, b = a.double(), b.double()
    if similarity_function == "euclidean":
        s = torch.cdist(a, b, p=2.0, compute_mode="donot_use_mm_for_euclid_dist")        # :78 (the reference's cdist may take the mm route)
        pos = s * lsim                                                                    # :81
        neg = s * (1 - lsim)                                                              # :82
        m = float(output_dim * 2 * vartheta) ** 0.5                                       # :83
        neg = neg.clip(max=m)                                                             # :84
        neg = m * (1 - lsim) - neg                                                        # :85
        return pos.pow(2).mean(), neg.pow(2).mean()                                       # :87-88
    s = (a / a.norm(dim=-1, keepdim=True)) @ (b / b.norm(dim=-1, keepdim=True)).t()       # calc_utils.py:38-49
    s = s.clip(min=threshold).clip(max=1 - threshold)                                     # :93
    l = (-lsim * torch.log(s) - (1 - lsim) * torch.log(1 - s)).mean()                    # :94
    return l, l


def soft_argmax_hash_loss(code):
    """:100-105"""
    return 1 - (2 * code.double() - 1).pow(2).mean()


def our_loss(image, text, labels, output_dim, vartheta=0.75, threshold=0.1, quan_alpha=0.001, similarity_function="euclidean"):
    """:107-149 -> dict of the nine scalars"""
    ls = label_sim(labels)
    kw = dict(output_dim=output_dim, vartheta=vartheta, threshold=threshold, similarity_function=similarity_function)
    ip, in_ = similarity_loss(image, text, ls, **kw)
    pi, ni = similarity_loss(image, image, ls, **kw)
    pt, nt = similarity_loss(text, text, ls, **kw)
    qi, qt = soft_argmax_hash_loss(image), soft_argmax_hash_loss(text)
    loss = (pt + pi + ni + nt) + (ip + in_) + quan_alpha * (qi + qt) / 2
    return {"loss": loss, "intra_pos": ip, "intra_neg": in_, "inter_pos_i": pi, "inter_neg_i": ni, "inter_pos_t": pt, "inter_neg_t": nt,
            "quan_i": qi, "quan_t": qt}


def our_loss_grad(image, text, labels, output_dim, **kw):
    """(d loss / d image, d loss / d text) in float64: autograd over our_loss above (runners/DCMHT/runner.py:124 loss.backward())"""
    img = image.double().clone().requires_grad_(True)
    txt = text.double().clone().requires_grad_(True)
    our_loss(img, txt, labels, output_dim, **kw)["loss"].backward()
    return img.grad, txt.grad


def load_dcmht(name):
    g = np.load(os.path.join(GOLDEN, "loss_dcmht.npz"))
    img, txt = torch.from_numpy(g[name + "_img"]), torch.from_numpy(g[name + "_txt"])
    labels = torch.from_numpy(g[name + "_labels"]) if name + "_labels" in g.files else None
    K, cos, vartheta, threshold, alpha = g[name + "_meta"]
    return img, txt, labels, int(K), "cosine" if cos else "euclidean", float(vartheta), float(threshold), float(alpha), g[name + "_ref"]


def load_dcmht_grads(name):
    g = np.load(os.path.join(GOLDEN, "loss_dcmht.npz"))
    return g[name + "_gimg"], g[name + "_gtxt"]


# ---- DSPH: the HyP loss (reference models/DSPH/loss/HyP.py:18-70) ---------------------------------------------------------------
HYP_CASES = ["b100_k16_c80", "b64_k128_c80", "b64_k16_c80_alpha0", "b48_k16_c80_single", "b48_k16_c80_shared", "b40_k16_c80_zero_row",
             "b24_k16_c24_nolabels"]
HYP_TERMS = ["loss", "pos", "neg", "pos_t", "neg_t", "reg", "reg_t", "reg_xt"]          # the order of xmh_hyp_loss's out8


def hyp_terms(x, y, P, labels, threshold, alpha):
    """The reference expression restated in the caller's dtype (float64 for an oracle): a dict of HYP_TERMS, differentiable.  `labels`
    [B, C] holds 0/1; nonzero counts as 1."""
    L = labels != 0
    zero = torch.zeros((), dtype=x.dtype)
    nP = F.normalize(P, p=2, dim=1)
    cos, cos_t = F.normalize(x, p=2, dim=1) @ nP.T, F.normalize(y, p=2, dim=1) @ nP.T
    p_num, n_num = L.sum().to(x.dtype), (~L).sum().to(x.dtype)
    t = {"pos": torch.where(L, 1 - cos, zero).sum() / p_num, "neg": torch.where(~L, F.relu(cos - threshold), zero).sum() / n_num,
         "pos_t": torch.where(L, 1 - cos_t, zero).sum() / p_num, "neg_t": torch.where(~L, F.relu(cos_t - threshold), zero).sum() / n_num}
    t["reg"] = t["reg_t"] = t["reg_xt"] = zero
    if alpha > 0:
        M = L.sum(1) > 1
        Lm = L[M].to(x.dtype)
        pairs = (Lm @ Lm.T) == 0
        Z = int(pairs.sum())
        if Z > 0:
            xm, ym = F.normalize(x[M], p=2, dim=1), F.normalize(y[M], p=2, dim=1)
            for key, sim in (("reg", xm @ xm.T), ("reg_t", ym @ ym.T), ("reg_xt", xm @ ym.T)):
                t[key] = torch.where(pairs, alpha * F.relu(sim - threshold), zero).sum() / Z
    t["loss"] = t["pos"] + t["neg"] + t["pos_t"] + t["neg_t"] + t["reg"] + t["reg_t"] + t["reg_xt"]
    return t


def hyp_oracle(x, y, P, labels, threshold, alpha):
    """float64 terms (numpy [8], HYP_TERMS order) and the gradients of the loss with respect to x, y, P (float64 numpy)"""
    x, y, P = (torch.as_tensor(v).double().requires_grad_(True) for v in (x, y, P))
    t = hyp_terms(x, y, P, torch.as_tensor(labels), threshold, alpha)
    t["loss"].backward()
    return np.array([float(t[k].detach()) for k in HYP_TERMS]), x.grad.numpy(), y.grad.numpy(), P.grad.numpy()


def load_hyp(name):
    """x, y, proxies, labels (None: the reference's identity default), threshold, alpha, loss, (gx, gy, gproxies)"""
    g = np.load(os.path.join(GOLDEN, "loss_dsph.npz"))
    K, C, alpha, threshold = g[name + "_meta"]
    labels = g[name + "_labels"] if name + "_labels" in g.files else None
    return (g[name + "_x"], g[name + "_y"], g[name + "_proxies"], labels, float(threshold), float(alpha), float(g[name + "_loss"]),
            (g[name + "_gx"], g[name + "_gy"], g[name + "_gproxies"]))


# ---- MITH: the training objective (reference models/MITH/MITH.py:116-232) -------------------------------------------------------
MITH_CASES = ["consecutive", "clamp", "sign0", "float_sim", "weights", "odd"]
MITH_INPUTS = ["res_img_cls", "res_txt_cls", "img_cls_hash", "txt_cls_hash", "tokens_hash_i", "tokens_hash_t", "trans_tokens_i",
               "trans_tokens_t"]
MITH_WEIGHTS = ["hyper_tokens_intra", "hyper_distill", "hyper_info_nce", "hyper_cls_inter", "hyper_quan", "hyper_alpha", "hyper_lambda"]
MITH_TERMS = ["loss", "intra_i", "intra_t", "i2t", "t2i", "quan_i", "quan_t", "nce_cls", "nce_tokens", "distillation"]   # out10


def mith_terms(xs, Y, S, w, tau=0.07):
    """The reference expression restated in the inputs' dtype (float64 for an oracle): the MITH_TERMS as a list, differentiable in xs.
    Y is the one buffer after the step's row write.  sign() is taken on fp32 codes, op for op, as the reference takes it."""
    rc_i, rc_t, c_i, c_t, t_i, t_t, T_i, T_t = xs
    lam = w["hyper_lambda"]

    def bayes(b):
        s = 0.5 * (Y @ b.T).clamp(min=-64, max=64)
        return -torch.mean(S * s - torch.log(1 + torch.exp(s)))

    def nce(s):                                   # s [n, m, m] logits; rows and columns against the diagonal
        n, m = s.shape[0], s.shape[1]
        tgt = torch.arange(m).repeat(n)
        return 0.5 * (F.cross_entropy(s.reshape(n * m, m), tgt) + F.cross_entropy(s.transpose(1, 2).reshape(n * m, m), tgt))

    f = [t.detach().float() for t in (c_i, t_i, c_t, t_t)]
    Bs = torch.sign((f[0] * lam + f[1] * (1 - lam)) + (f[2] * lam + f[3] * (1 - lam))).to(c_i.dtype)
    B, K = c_i.shape
    t = [None, bayes(t_i), bayes(t_t), bayes(c_t), bayes(c_i),
         ((c_i * 0.5 + t_i * 0.5 - Bs) ** 2).sum() / B / K, ((c_t * 0.5 + t_t * 0.5 - Bs) ** 2).sum() / B / K,
         nce((rc_i @ rc_t.T / tau)[None]), nce(torch.bmm(T_i.permute(1, 0, 2), T_t.permute(1, 2, 0)) / tau)]
    t.append(w["hyper_distill"] * (((c_i.detach() - t_i) ** 2).sum() + ((c_t.detach() - t_t) ** 2).sum()
                                   + 0.1 * (((c_i - t_i.detach()) ** 2).sum() + ((c_t - t_t.detach()) ** 2).sum())) / B)
    t[0] = (w["hyper_tokens_intra"] * (t[1] + t[2]) + w["hyper_cls_inter"] * (t[3] + t[4]) + w["hyper_quan"] * (t[5] + t[6])
            + w["hyper_info_nce"] * (t[7] + w["hyper_alpha"] * t[8]) + t[9])
    return t


def mith_oracle(xs, Y, S, w):
    """float64 terms (numpy [10], MITH_TERMS order) and the eight gradients of the loss (float64 numpy)"""
    xs = [torch.as_tensor(np.asarray(x)).double().requires_grad_(True) for x in xs]
    t = mith_terms(xs, torch.as_tensor(np.asarray(Y)).double(), torch.as_tensor(np.asarray(S)).double(), w)
    t[0].backward()
    return np.array([float(v.detach()) for v in t]), [x.grad.numpy() for x in xs]


def load_mith(name):
    """(N, B, K, D, weights dict, buf0, [step dicts with the inputs list, indexs, label_sim, buf, terms, grads list])"""
    g = np.load(os.path.join(GOLDEN, "loss_mith.npz"))
    meta = g[name + "_meta"]
    N, B, K, D, steps = (int(v) for v in meta[:5])
    w = dict(zip(MITH_WEIGHTS, (float(v) for v in meta[5:])))
    out = []
    for s in range(steps):
        p = "%s_s%d_" % (name, s)
        out.append({"inputs": [g[p + k] for k in MITH_INPUTS], "indexs": g[p + "indexs"], "label_sim": g[p + "label_sim"], "buf": g[p + "buf"],
                    "terms": g[p + "terms"], "grads": [g[p + "g_" + k] for k in MITH_INPUTS]})
    return N, B, K, D, w, g[name + "_buf0"], out
