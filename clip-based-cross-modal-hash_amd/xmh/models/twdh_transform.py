"""The stage that makes TwDH's short-code transforms (reference runners/TwDH/transform_matrix_generation/: model.py:6-24,
train.py:44-96 and 141-176).  ``TwDH`` loads one fixed ``[2*long, 2*short]`` matrix per short length; this module
trains such a matrix from the label rows of a training split and the two hash centres, and checks whether a matrix is lossless.

The recipe.  M is fp32 [2L, 2S], drawn by ``np.random.uniform(-1, 1)``.  Per batch of label rows, ``t_long`` and ``t_short`` are the
hash-centre targets of the rows (xmh_twdh_targets over the two streams long, short; one tie vector per centre and batch, long
first -- ``TwDH.draw_ties``' order for one key; a row without a label gets all bits 0).  ``p = pair_softmax(hash_convert(t_long) . M)``
and ``loss = hash + bce + lasso`` with ``hash = 1 - mean_{b,s}((p[b,2s] - p[b,2s+1])^2)``, ``bce = nn.BCELoss()(p,
hash_convert(t_short))`` and ``lasso = alpha |M|_1``.  The optimiser is ``xmh.optim.BertAdam`` (warmup_cosine, b1 0.9, b2 0.98,
e 1e-6, max_grad_norm 1, t_total = batches per epoch x post_epochs).  The loader shuffles and keeps the last partial batch.  After
every epoch the matrix is saved and checked: argmax over each pair of ``hash_convert(long_center) . M`` must equal
``short_center > 0`` for every class and bit (equal logits give bit 0); when it does, ``<short>_zeros.pkl`` is saved too and the
run stops.  Where the reference's script is undefined (it cannot run as shipped): the epoch count is ``post_epochs``, labels are
all that is read of the dataset, and files are ``torch.save`` of a CPU fp32 tensor at ``<save_dir>/<long>/<short>.pkl``, the layout
``TwDH.from_config`` reads.

``TransformObjective`` is the ``Spec`` of the objective for the ``Objective`` bridge: xmh_twdh_trans_loss forward,
xmh_twdh_trans_grad backward.  There is no CPU fallback."""
import collections
import math
import os

import numpy as np
import torch

from .. import retrieval as R
from .._lib import check, current_stream, lib, ptr
from ..optim import BertAdam
from .objective import Objective, Spec, need_cuda
from .twdh import _check_center


def _pack(consts, aux, ts):
    L, S, alpha = consts
    targets, = aux
    B = targets.shape[0]
    return (B, L, S), (ptr(ts[0]), ptr(targets), B, L, S, alpha)


# forward = xmh_twdh_trans_loss -> fp32 [4] (total, hash, bce, lasso; element 0 carries the gradient), backward = xmh_twdh_trans_grad
TransformObjective = Spec(lib.xmh_twdh_trans_loss, lib.xmh_twdh_trans_grad, _pack, lib.xmh_twdh_trans_ws_bytes,
                          "TwDH transform: B=%d L=%d S=%d outside B <= 4096, L + S <= 4096", out_len=4, terms=4)


def transform_loss(M, targets, L, S, alpha=1e-3):
    """(loss, terms): the objective of the matrix M [2L, 2S] against the packed targets [B, ceil((L + S) / 32)] int32 of
    ``transform_targets``; ``loss`` is a 0-dim fp32 device tensor, differentiable in M, ``terms`` the detached fp32 [4] (total, hash,
    bce, lasso)"""
    need_cuda(M, targets)
    if M.dim() != 2 or tuple(M.shape) != (2 * L, 2 * S):
        raise ValueError("TwDH transform: a matrix of shape %s where [%d, %d] (2 * long, 2 * short) is expected" % (tuple(M.shape), 2 * L, 2 * S))
    Tw = (L + S + 31) // 32
    if targets.dim() != 2 or targets.shape[1] != Tw or targets.dtype != torch.int32 or not targets.is_contiguous():
        raise ValueError("TwDH transform: targets of shape %s (%s) where contiguous int32 [B, %d] is expected for a matrix of shape %s"
                         % (tuple(targets.shape), targets.dtype, Tw, tuple(M.shape)))
    out = Objective.apply(TransformObjective, (int(L), int(S), float(alpha)), (targets,), M)
    return out[0], out.detach()


def _centres(long_center, short_center):
    """the two centres checked, as one int8 [C, L + S] (the layout ``TwDH._constants`` builds)"""
    lc = _check_center(torch.as_tensor(long_center).detach().cpu().float(), "long_center")
    sc = _check_center(torch.as_tensor(short_center).detach().cpu().float(), "short_center")
    if lc.shape[0] != sc.shape[0]:
        raise ValueError("TwDH transform: a long centre of shape %s and a short centre of shape %s (the class counts differ)"
                         % (tuple(lc.shape), tuple(sc.shape)))
    return torch.cat([lc, sc], 1).to(torch.int8).contiguous(), lc.shape[1], sc.shape[1]


def transform_targets(lab, C, centres, tie):
    """xmh_twdh_targets for the two streams: lab [B, ceil(C / 32)] packed label rows, centres int8 [C, L + S], tie int8 [L + S], all on
    the device -> int32 [B, ceil((L + S) / 32)]"""
    B, K = lab.shape[0], centres.shape[1]
    targets = torch.empty(B, (K + 31) // 32, dtype=torch.int32, device=centres.device)
    check(lib.xmh_twdh_targets(ptr(lab), C, ptr(centres), ptr(tie), B, K, ptr(targets), current_stream()), "xmh_twdh_targets")
    return targets


def _device_of(t):
    if torch.is_tensor(t) and t.is_cuda:
        return t.device
    if not torch.cuda.is_available():
        raise RuntimeError("the TwDH transform stage needs a CUDA/HIP device; there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def _fidelity_device(trans, centres, L, S):
    """xmh_twdh_trans_check -> the device int32 [1 + C * ceil(S / 32)] (count, bitmap); no synchronisation"""
    C, Sw = centres.shape[0], (S + 31) // 32
    wrong = torch.empty(1 + C * Sw, dtype=torch.int32, device=trans.device)
    check(lib.xmh_twdh_trans_check(ptr(trans), ptr(centres), C, L, S, ptr(wrong), current_stream()), "xmh_twdh_trans_check")
    return wrong


def transform_fidelity(long_center, short_center, trans):
    """(n_wrong, wrong [C, S] bool): the class / bit pairs at which argmax over the pairs of ``hash_convert(long_center) . trans``
    differs from ``short_center > 0`` (xmh_twdh_trans_check; equal logits give bit 0).  A lossless transform has n_wrong == 0."""
    centres, L, S = _centres(long_center, short_center)
    trans = torch.as_tensor(trans)
    if trans.dim() != 2 or tuple(trans.shape) != (2 * L, 2 * S):
        raise ValueError("TwDH transform: a matrix of shape %s for a long centre of shape %s and a short centre of shape %s ([%d, %d] is "
                         "expected)" % (tuple(trans.shape), (centres.shape[0], L), (centres.shape[0], S), 2 * L, 2 * S))
    dev = _device_of(trans)
    with torch.cuda.device(dev):
        M = trans.detach().to(dev, torch.float32).contiguous()
        raw = _fidelity_device(M, centres.to(dev), L, S).cpu()
    C, Sw = centres.shape[0], (S + 31) // 32
    words = raw[1:].numpy().view(np.uint32).reshape(C, Sw)
    bits = ((words[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(C, Sw * 32)[:, :S].astype(bool)
    return int(raw[0]), torch.from_numpy(bits)


Generated = collections.namedtuple("Generated", "matrix lossless epoch terms")


def generate_transform(labels, long_center, short_center, *, batch_size=200, post_epochs=100, post_lr=1e-3, alpha=1e-3, weight_decay=0.2,
                       warmup=0.1, init=None, batches=None, ties=None, save_dir=None, logger=None):
    """Train one transform by the recipe above.  labels [N, C] (a class is set where the entry equals 1), long_center [C, L] and
    short_center [C, S] of +-1.  Returns ``Generated(matrix, lossless, epoch, terms)``: the CPU fp32 [2L, 2S] matrix, whether it
    passed the check, the (0-based) epoch after which the run stopped, and the per-epoch means of (total, hash, bce, lasso) as a
    float64 [epochs run, 4] array.

    ``init`` (a [2L, 2S] matrix), ``batches`` (``batches[epoch]``: the index tensors of that epoch's batches, in order) and ``ties``
    (``ties[step]``: the pair (long tie [L], short tie [S]) of +-1 of that global step) replay stored draws.  Without them the matrix
    comes from ``np.random.uniform``, the order from one ``torch.randperm(N)`` per epoch on the CPU generator (the last partial batch
    is kept) and the ties from two ``torch.randint_like`` calls per batch, long first.  The draws are the reference's, but a
    ``DataLoader`` consumes the generator in its own way: bit-equal random consumption with the reference's loader is not promised.

    Nothing is read back per step.  Per epoch one read is made: the check's count together with the epoch's loss terms, which are
    accumulated on the device.  With ``save_dir`` the matrix is saved after every epoch as ``<save_dir>/<L>/<S>.pkl`` and, once
    lossless, as ``<S>_zeros.pkl``."""
    centres, L, S = _centres(long_center, short_center)
    labels = torch.as_tensor(labels)
    C = centres.shape[0]
    if labels.dim() != 2 or labels.shape[1] != C or labels.shape[0] == 0:
        raise ValueError("TwDH transform: labels of shape %s for hash centres of shape %s (one column per class is expected)"
                         % (tuple(labels.shape), (C, L + S)))
    N = labels.shape[0]
    if batch_size <= 0 or post_epochs <= 0:
        raise ValueError("TwDH transform: batch_size %r and post_epochs %r must be positive" % (batch_size, post_epochs))
    dev = _device_of(labels)
    if init is None:
        init = torch.from_numpy(np.random.uniform(low=-1, high=1, size=(2 * L, 2 * S))).float()      # model.py:13
    init = torch.as_tensor(init)
    if tuple(init.shape) != (2 * L, 2 * S):
        raise ValueError("TwDH transform: an initial matrix of shape %s for centres of shape %s and %s ([%d, %d] is expected)"
                         % (tuple(init.shape), (C, L), (C, S), 2 * L, 2 * S))
    say = (logger.info if hasattr(logger, "info") else logger) if logger is not None else (lambda *_: None)
    with torch.cuda.device(dev):
        M = torch.nn.Parameter(init.detach().to(dev, torch.float32).clone().contiguous())
        centres = centres.to(dev)
        lab = R.pack_labels((labels == 1).to(torch.uint8).to(dev))                    # every row once; a batch gathers its rows
        per_epoch = len(batches[0]) if batches is not None else math.ceil(N / batch_size)
        opt = BertAdam([M], lr=post_lr, warmup=warmup, schedule="warmup_cosine", b1=0.9, b2=0.98, e=1e-6,
                       t_total=per_epoch * post_epochs, weight_decay=weight_decay, max_grad_norm=1.0)
        out_dir = None
        if save_dir is not None:
            out_dir = os.path.join(save_dir, str(L))
            os.makedirs(out_dir, exist_ok=True)
        history, lossless, step, epoch = [], False, 0, 0
        for epoch in range(post_epochs):
            if batches is not None:
                order = [torch.as_tensor(b, dtype=torch.int64) for b in batches[epoch]]
            else:
                perm = torch.randperm(N)
                order = [perm[i:i + batch_size] for i in range(0, N, batch_size)]
            acc = torch.zeros(4, dtype=torch.float64, device=dev)
            for idx in order:
                if ties is not None:
                    tl, ts = ties[step]
                else:                                                                  # train.py:46, once per centre and batch
                    tl = torch.randint_like(torch.empty(L), 2) * 2 - 1
                    ts = torch.randint_like(torch.empty(S), 2) * 2 - 1
                tie = torch.cat([torch.as_tensor(tl).reshape(-1), torch.as_tensor(ts).reshape(-1)]).to(torch.int8)
                if tie.numel() != L + S:
                    raise ValueError("TwDH transform: %d tie entries for %d + %d target bits" % (tie.numel(), L, S))
                tie = (tie if tie.is_cuda else tie.pin_memory()).to(dev, non_blocking=True)
                rows = lab.index_select(0, (idx if idx.is_cuda else idx.pin_memory()).to(dev, non_blocking=True))
                loss, terms = transform_loss(M, transform_targets(rows, C, centres, tie), L, S, alpha)
                opt.zero_grad()
                loss.backward()
                opt.step()
                acc += terms
                step += 1
            wrong = _fidelity_device(M.detach(), centres, L, S)
            read = torch.cat([wrong[:1].double(), acc / len(order)]).cpu()             # the epoch's one read
            lossless = int(read[0]) == 0
            history.append(read[1:].numpy())
            say("epoch %d: loss %.6f hash %.6f bce %.6f lasso %.6f, %d wrong bits of %d"
                % ((epoch,) + tuple(history[-1]) + (int(read[0]), C * S)))
            if out_dir is not None:
                torch.save(M.detach().cpu(), os.path.join(out_dir, "%d.pkl" % S))
                if lossless:
                    torch.save(M.detach().cpu(), os.path.join(out_dir, "%d_zeros.pkl" % S))
            if lossless:
                say("find a lossless transform matrix!")
                break
        return Generated(M.detach().cpu(), lossless, epoch, np.stack(history))
