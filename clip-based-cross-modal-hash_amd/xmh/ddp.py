"""``GradReducer``: the gradient all-reduce of distributed training, what the reference gets from
``DistributedDataParallel(find_unused_parameters=True)`` (runners/base.py:98-118).

Every gradient of a step travels in ONE flat fp32 bucket and one collective: ``reduce()`` packs ``p.grad / world_size`` of every
parameter into the bucket in one launch (csrc/xmh_bucket.hip), all-reduces the bucket with SUM and hands every parameter a VIEW of
its range as ``p.grad`` (Python assignment, no launch).  BertAdam and torch's SGD read ``p.grad.data_ptr()`` and clip in place, so
they work on the views as on any gradient.

Layout of the bucket (``bucket_layout``): tensor i at ``offset[i]``, a multiple of 64 floats, in the order of the parameter list;
behind the last tensor, at ``tail`` (again a multiple of 64), the FLAG TAIL: one float per tensor, 1.0 where this rank had a
gradient, 0.0 where ``p.grad`` was None (the kernel then writes zeros for the tensor).  After the SUM the tail holds, per parameter,
the number of ranks that had a gradient: a parameter with 0 there keeps ``.grad = None`` on every rank, so the optimiser neither
moves nor ages it (CLIP's ``logit_scale``), exactly as in one process -- without a second collective.  A parameter some ranks had
a gradient for gets the sum over those ranks divided by the world size, as DistributedDataParallel gives.

The bucket and the device tables are allocated once; the table is uploaded again only when a gradient's address or presence
changes (``optim._Mirror``).  Reading the tail back is one small device-to-host copy per step -- the one host synchronisation of
``reduce()``, the counterpart of DistributedDataParallel's own copy of its used-parameter map under find_unused_parameters.
There is no CPU fallback: a gradient that is not a dense contiguous fp32 tensor on the parameters' device raises.
"""
from __future__ import annotations

import numpy as np
import torch
from torch import distributed as dist

from .optim import CHUNK_DTYPE, _Mirror

ALIGN = 64                                                   # floats: every tensor and the tail start on a 256-byte boundary

# include/xmh.h: xmh_bucket_tensor (40 bytes)
BUCKET_DTYPE = np.dtype([("t", "<i8"), ("offset", "<i8"), ("numel", "<i8"), ("flag_at", "<i8"), ("flag", "<f4"), ("reserved", "<i4")])
assert BUCKET_DTYPE.itemsize == 40


def _up(n: int) -> int:
    return (int(n) + ALIGN - 1) // ALIGN * ALIGN


def bucket_layout(numels):
    """-> (offsets [n], tail, total): the first element of every tensor, of the flag tail, and the bucket's length in floats"""
    offsets, at = [], 0
    for n in numels:
        if int(n) < 1:
            raise ValueError("bucket_layout: a tensor of %d elements (leave empty tensors out)" % int(n))
        offsets.append(at)
        at = _up(at + int(n))
    return offsets, at, at + _up(len(offsets))


def chunk_map(numels, chunk: int) -> np.ndarray:
    """xmh_bertadam_chunk_ref rows: the chunks of tensor 0, then of tensor 1, ... (include/xmh.h)"""
    n = np.asarray(list(numels), dtype=np.int64)
    counts = (n + chunk - 1) // chunk
    first = np.concatenate(([0], np.cumsum(counts)[:-1])) if len(n) else np.zeros(0, np.int64)
    cm = np.empty(int(counts.sum()), dtype=CHUNK_DTYPE)
    cm["tensor"] = np.repeat(np.arange(len(n), dtype=np.int32), counts)
    cm["first_chunk"] = np.repeat(first, counts).astype(np.int32)
    cm["start"] = (np.arange(len(cm), dtype=np.int64) - cm["first_chunk"]) * chunk
    return cm


def bucket_table(pointers, numels, flags=True) -> np.ndarray:
    """xmh_bucket_tensor rows for tensors at `pointers` (an address, or None / 0: no tensor on this rank) in bucket_layout's places;
    flags: whether the rows carry the flag tail (pack of gradients) or not (the parameter broadcast)"""
    offsets, tail, _ = bucket_layout(numels)
    table = np.zeros(len(offsets), dtype=BUCKET_DTYPE)
    table["t"] = [int(p or 0) for p in pointers]
    table["offset"], table["numel"] = offsets, [int(n) for n in numels]
    table["flag_at"] = tail + np.arange(len(offsets), dtype=np.int64) if flags else -1
    table["flag"] = (table["t"] != 0).astype(np.float32) if flags else 0.0
    return table


def _check(t: torch.Tensor, index: int, what: str, device) -> None:
    if t.is_sparse or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.device != device:
        raise RuntimeError("GradReducer: %s of parameter %d is %s %s on %s%s: the bucket takes dense contiguous fp32 tensors on %s, "
                           "there is no CPU fallback" % (what, index, "sparse" if t.is_sparse else "dense", t.dtype, t.device,
                                                         "" if t.is_sparse or t.is_contiguous() else ", not contiguous", device))


class GradReducer:
    """model: the parameters are ``model.parameters()`` with ``requires_grad`` and at least one element, in module order -- the same
    list on every rank (checked once with a small all-reduce); world_size: the divisor; group: the process group (None: the default)."""

    def __init__(self, model, world_size: int, group=None):
        from . import _lib
        self.params = [p for p in model.parameters() if p.requires_grad and p.numel() > 0]
        if not self.params:
            raise ValueError("GradReducer: the model has no parameter that requires a gradient")
        self.world_size, self.group = int(world_size), group
        self.device = self.params[0].device
        for i, p in enumerate(self.params):
            _check(p.detach(), i, "the data", self.device)
        self.numels = [p.numel() for p in self.params]
        self.offsets, self.tail, self.total = bucket_layout(self.numels)
        self.chunk = int(_lib.lib.xmh_bertadam_chunk())
        self._cmap = chunk_map(self.numels, self.chunk)
        self.flat = torch.zeros(self.total, dtype=torch.float32, device=self.device)
        self.views = [self.flat[o:o + n].view(p.shape) for o, n, p in zip(self.offsets, self.numels, self.params)]
        self._table, self._map = _Mirror(), _Mirror()
        self._key, self._host = None, None
        self.collectives = 0                                 # all-reduces and broadcasts of the bucket so far
        self._same_everywhere()

    def _same_everywhere(self):
        """the parameter list has the same length and total size on every rank, or the bucket's ranges would not line up"""
        mine = torch.tensor([len(self.params), sum(self.numels)], dtype=torch.int64, device=self.device)
        low, high = mine.clone(), mine.clone()
        dist.all_reduce(low, op=dist.ReduceOp.MIN, group=self.group)
        dist.all_reduce(high, op=dist.ReduceOp.MAX, group=self.group)
        if not (torch.equal(low, mine) and torch.equal(high, mine)):
            raise RuntimeError("GradReducer: this rank has %d parameters of %d elements, the ranks between them %s to %s"
                               % (int(mine[0]), int(mine[1]), low.tolist(), high.tolist()))

    def _call(self, pack: bool, table: np.ndarray, scale: float = 1.0):
        from . import _lib
        with torch.cuda.device(self.device):
            d_table, d_map = self._table.put(table, self.device), self._map.put(self._cmap, self.device)
            if pack:
                _lib.check(_lib.lib.xmh_bucket_pack(_lib.ptr(d_table), len(table), _lib.ptr(d_map), len(self._cmap), scale,
                                                    _lib.ptr(self.flat), _lib.current_stream()), "xmh_bucket_pack")
            else:
                _lib.check(_lib.lib.xmh_bucket_unpack(_lib.ptr(d_table), len(table), _lib.ptr(d_map), len(self._cmap), _lib.ptr(self.flat),
                                                      _lib.current_stream()), "xmh_bucket_unpack")

    @torch.no_grad()
    def broadcast_parameters(self, src: int = 0):
        """every rank takes rank `src`'s parameters (DistributedDataParallel does this at construction): pack, one broadcast, unpack"""
        table = bucket_table([p.data_ptr() for p in self.params], self.numels, flags=False)
        self._call(True, table)
        dist.broadcast(self.flat, src=src, group=self.group)
        self.collectives += 1
        self._call(False, table)
        self._key = None

    @torch.no_grad()
    def reduce(self):
        """after ``loss.backward()``: every ``p.grad`` becomes the mean over the ranks (a rank without one counts as zero), a view of
        the bucket; a parameter no rank had a gradient for keeps ``.grad = None``"""
        grads = [p.grad for p in self.params]
        for i, g in enumerate(grads):
            if g is not None:
                _check(g, i, "the gradient", self.device)
        key = tuple(0 if g is None else g.data_ptr() for g in grads)
        if key != self._key:
            self._key, self._host = key, bucket_table(key, self.numels)
        self._call(True, self._host, 1.0 / self.world_size)
        dist.all_reduce(self.flat, op=dist.ReduceOp.SUM, group=self.group)
        self.collectives += 1
        had = self.flat[self.tail:self.tail + len(self.params)].cpu().numpy() > 0.0
        for p, view, some in zip(self.params, self.views, had):
            p.grad = view if some else None
