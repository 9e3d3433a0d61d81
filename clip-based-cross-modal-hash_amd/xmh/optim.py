"""``BertAdam``: the optimiser every config of the reference names (models/common/optimizer.py:25-167), as ONE fused
multi-tensor step in HIP (csrc/xmh_optim.hip).

Same constructor, the same six ``ValueError`` checks, ``SCHEDULES``, ``get_lr()`` and state keys (``step``, ``next_m``,
``next_v``), so a state dict saved by the reference's class loads here and the other way round.  It is not AdamW: no bias
correction, every parameter's gradient clipped by its own L2 norm (the clipped gradient stays in ``p.grad``), the decay
added to the update, a step counter per parameter (``grad is None``: neither moves nor ages) and the rate scaled by a
warm-up schedule of ``step / t_total``.

``step()`` describes the tensors that have a gradient in a table (xmh_bertadam_tensor) and a chunk map on the host, uploads
each only when it differs from what the device holds (non-blocking, out of a ring of pinned staging buffers that are not
rewritten before the copy reading them has completed) and makes one C call, two launches, on the current stream.  It never
synchronises with the host.  There is no CPU fallback: a parameter or gradient that is not a dense contiguous fp32 CUDA
tensor raises with the parameter's index.  One optimiser is stepped from one stream at a time.
"""
from __future__ import annotations

import math

import numpy as np
import torch
from torch.optim import Optimizer
from torch.optim.optimizer import required

from .common.register import registry


def warmup_cosine(x, warmup=0.002):
    if x < warmup:
        return x / warmup
    return 0.5 * (1.0 + math.cos(math.pi * x))


def warmup_constant(x, warmup=0.002):
    """rises linearly over ``warmup`` of the training steps, 1 afterwards"""
    if x < warmup:
        return x / warmup
    return 1.0


def warmup_linear(x, warmup=0.002):
    """triangular: the peak at ``warmup``, zero from ``t_total`` steps on"""
    if x < warmup:
        return x / warmup
    return max((x - 1.) / (warmup - 1.), 0)


SCHEDULES = {
    "warmup_cosine": warmup_cosine,
    "warmup_constant": warmup_constant,
    "warmup_linear": warmup_linear,
}

# include/xmh.h: xmh_bertadam_tensor (72 bytes) and xmh_bertadam_chunk_ref (16 bytes)
TENSOR_DTYPE = np.dtype([("p", "<i8"), ("g", "<i8"), ("m", "<i8"), ("v", "<i8"), ("numel", "<i8"), ("lr", "<f4"), ("b1", "<f4"),
                         ("b2", "<f4"), ("one_minus_b1", "<f4"), ("one_minus_b2", "<f4"), ("e", "<f4"), ("weight_decay", "<f4"),
                         ("max_grad_norm", "<f4")])
CHUNK_DTYPE = np.dtype([("start", "<i8"), ("tensor", "<i4"), ("first_chunk", "<i4")])
assert TENSOR_DTYPE.itemsize == 72 and CHUNK_DTYPE.itemsize == 16

_RING = 8                                                    # staging slots before step() waits for the oldest copy


class _Mirror:
    """A byte array on the device and what it currently holds.  ``put`` uploads only when the content differs: a non-blocking copy
    from a pinned staging slot whose previous copy has completed (the slot's event says so; a busy ring grows up to _RING)."""

    def __init__(self):
        self.dev = None
        self.held = None
        self.slots = []                                      # [pinned uint8 tensor, event or None]

    def _slot(self, nbytes):
        for s in self.slots:
            if s[1] is None or s[1].query():
                break
        else:
            if len(self.slots) < _RING:
                s = [None, None]
                self.slots.append(s)
            else:                                            # every copy still in flight: wait for the oldest one only
                s = self.slots.pop(0)
                self.slots.append(s)
                s[1].synchronize()
        if s[0] is None or s[0].numel() < nbytes:
            s[0] = torch.empty(max(4096, 2 * nbytes), dtype=torch.uint8, pin_memory=True)
        return s

    def put(self, host: np.ndarray, device):
        raw = host.view(np.uint8).reshape(-1)
        if self.held is not None and self.dev.device == device and self.held.shape == raw.shape and np.array_equal(self.held, raw):
            return self.dev
        n = raw.shape[0]
        if self.dev is None or self.dev.device != device or self.dev.numel() < n:
            self.dev = torch.empty(max(4096, 2 * n), dtype=torch.uint8, device=device)
        s = self._slot(n)
        s[0][:n].copy_(torch.from_numpy(raw))
        self.dev[:n].copy_(s[0][:n], non_blocking=True)
        if s[1] is None:
            s[1] = torch.cuda.Event()
        s[1].record(torch.cuda.current_stream(device))
        self.held = raw.copy()
        return self.dev


@registry.register_optimizer("BertAdam")
class BertAdam(Optimizer):
    """BERT's Adam with the weight-decay fix (reference models/common/optimizer.py:50-167).

    lr; warmup: share of t_total spent warming up, -1 = none; t_total: steps of the schedule, -1 = constant rate; schedule: a key of
    SCHEDULES; b1, b2, e: Adam's; weight_decay; max_grad_norm: per-parameter clipping norm, -1 = none."""

    def __init__(self, params, lr=required, warmup=-1, t_total=-1, schedule="warmup_linear", b1=0.9, b2=0.999, e=1e-6,
                 weight_decay=0.01, max_grad_norm=1.0):
        if lr is not required and lr < 0.0:
            raise ValueError("Invalid learning rate: {} - should be >= 0.0".format(lr))
        if schedule not in SCHEDULES:
            raise ValueError("Invalid schedule parameter: {}".format(schedule))
        if not 0.0 <= warmup < 1.0 and not warmup == -1:
            raise ValueError("Invalid warmup: {} - should be in [0.0, 1.0[ or -1".format(warmup))
        if not 0.0 <= b1 < 1.0:
            raise ValueError("Invalid b1 parameter: {} - should be in [0.0, 1.0[".format(b1))
        if not 0.0 <= b2 < 1.0:
            raise ValueError("Invalid b2 parameter: {} - should be in [0.0, 1.0[".format(b2))
        if not e >= 0.0:
            raise ValueError("Invalid epsilon value: {} - should be >= 0.0".format(e))
        defaults = dict(lr=lr, schedule=schedule, warmup=warmup, t_total=t_total, b1=b1, b2=b2, e=e, weight_decay=weight_decay,
                        max_grad_norm=max_grad_norm)
        super().__init__(params, defaults)

    def _mirrors(self):
        """device copies of the table and the chunk map; made on first use (an unpickled optimiser starts without them)"""
        if "_table" not in self.__dict__:
            self._table, self._map = _Mirror(), _Mirror()
            self._map_key, self._map_host = None, None
        return self._table, self._map

    @staticmethod
    def _scheduled(group, step):
        if group["t_total"] != -1:
            return group["lr"] * SCHEDULES[group["schedule"]](step / group["t_total"], group["warmup"])
        return group["lr"]

    def get_lr(self):
        lr = []
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                state = self.state[p]
                if len(state) == 0:
                    return [0]
                lr.append(self._scheduled(group, state["step"]))
        return lr

    @staticmethod
    def _check(t, index, what, device):
        if t.is_sparse:
            raise RuntimeError("BertAdam: %s of parameter %d is sparse (Adam does not support sparse gradients)" % (what, index))
        if not t.is_cuda:
            raise RuntimeError("BertAdam: %s of parameter %d is on %s: the step runs on the GPU only, there is no CPU fallback"
                               % (what, index, t.device))
        if t.dtype != torch.float32:
            raise RuntimeError("BertAdam: %s of parameter %d is %s, fp32 only" % (what, index, t.dtype))
        if not t.is_contiguous():
            raise RuntimeError("BertAdam: %s of parameter %d is not contiguous" % (what, index))
        if device is not None and t.device != device:
            raise RuntimeError("BertAdam: %s of parameter %d is on %s, the others on %s" % (what, index, t.device, device))

    def _chunk_map(self, numels, chunk):
        key = (chunk,) + tuple(numels)
        if key != self._map_key:
            n = np.asarray(numels, dtype=np.int64)
            counts = (n + chunk - 1) // chunk
            first = np.concatenate(([0], np.cumsum(counts)[:-1])) if len(n) else np.zeros(0, np.int64)
            cm = np.empty(int(counts.sum()), dtype=CHUNK_DTYPE)
            cm["tensor"] = np.repeat(np.arange(len(n), dtype=np.int32), counts)
            cm["first_chunk"] = np.repeat(first, counts).astype(np.int32)
            cm["start"] = (np.arange(len(cm), dtype=np.int64) - cm["first_chunk"]) * chunk
            self._map_key, self._map_host = key, cm
        return self._map_host

    @torch.no_grad()
    def step(self, closure=None):
        """One optimisation step.  closure (optional) re-evaluates the model and returns the loss."""
        from . import _lib
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()

        rows, states, device, index = [], [], None, -1
        for group in self.param_groups:
            hyper = (float(group["b1"]), float(group["b2"]), 1.0 - group["b1"], 1.0 - group["b2"], float(group["e"]),
                     float(group["weight_decay"]), float(group["max_grad_norm"]))
            for p in group["params"]:
                index += 1
                grad = p.grad
                if grad is None or p.numel() == 0:
                    continue
                self._check(p, index, "the data", device)
                device = p.device
                self._check(grad, index, "the gradient", device)
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = 0
                    state["next_m"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    state["next_v"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                m, v = state["next_m"], state["next_v"]
                if m.shape != p.shape or v.shape != p.shape:
                    raise RuntimeError("BertAdam: the state of parameter %d has another shape than the parameter" % index)
                self._check(m, index, "next_m", device)
                self._check(v, index, "next_v", device)
                rows.append((p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(),
                             self._scheduled(group, state["step"])) + hyper)
                states.append(state)
        if not rows:
            return loss

        chunk = int(_lib.lib.xmh_bertadam_chunk())
        table = np.array(rows, dtype=TENSOR_DTYPE)           # doubles are rounded to fp32 here, once
        m_table, m_map = self._mirrors()
        cmap = self._chunk_map([r[4] for r in rows], chunk)
        with torch.cuda.device(device):
            d_table = m_table.put(table, device)
            d_map = m_map.put(cmap, device)
            nws = _lib.lib.xmh_bertadam_ws_bytes(len(table), len(cmap))
            ws = _lib.workspace(nws, device)
            _lib.check(_lib.lib.xmh_bertadam_step(_lib.ptr(d_table), len(table), _lib.ptr(d_map), len(cmap), _lib.ptr(ws), nws,
                                                  _lib.current_stream()), "xmh_bertadam_step")
        for state in states:
            state["step"] += 1
        return loss
