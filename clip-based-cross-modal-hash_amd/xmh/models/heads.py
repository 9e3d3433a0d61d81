"""Hash heads of the in-scope methods, parameters under the reference's key names, forward in libxmh.so.

  DCMHT  models/DCMHT/hash/hash.py:15-82   MHA on a length-1 sequence == out_proj(v_proj(x)) (softmax over one key
         is 1), BatchNorm1d (image) / LayerNorm (text), fc2, relu, pair softmax
  DSPH   models/DSPH/hash/hash.py:6-45     tanh(dropout(fc(x))) (dropout is identity in eval)

The switch between the two paths of a head is ``self.training`` alone (what the reference's ``change_state`` sets):

  .eval()   the inference path (xmh_head_dcmht / xmh_head_dsph on the precision-tagged weight planes), under no_grad whatever
            ``requires_grad`` says: no autograd graph behind its output.
  .train()  xmh_head_grad.hip behind torch.autograd: exact-fp32 forward with batch statistics / dropout that keeps
            what backward reads, backward to every parameter of the head and to the embeddings.  Frozen parameters
            (``requires_grad=False``) get no gradient and their products are not launched.  Under ``torch.no_grad()`` the same
            train forward runs (batch statistics, running buffers updated) and nothing is kept.

Modules are constructed in train mode, as every nn.Module is.  Before the train path existed a BatchNorm (image) head or a DSPH
head in that state raised, while a LayerNorm (text) DCMHT head silently ran the inference path; now all of them take the train
path until ``.eval()`` is called -- every caller that encodes (the models' ``from_config(...).eval()``, the runners) does call it.
"""
from __future__ import annotations

import ctypes

import torch
import torch.nn as nn

from .. import _lib, ops
from .._lib import check, current_stream, lib, ptr
from . import clip as _clip


class DCMHTModalityHash(nn.Module):
    def __init__(self, inputDim=512, outputDim=64, num_heads=8, layernorm=True):
        super().__init__()
        self.bit = outputDim
        self.atten = nn.MultiheadAttention(inputDim, num_heads=num_heads, batch_first=True)
        self.norm = nn.LayerNorm(inputDim) if layernorm else nn.BatchNorm1d(inputDim)
        self.fc2 = nn.Linear(inputDim, outputDim * 2)
        # distributed training: the process group over whose ranks a BatchNorm head takes its batch statistics, what the
        # reference gets from convert_sync_batchnorm; None: the local batch, the fused calls
        self.sync_group = None

    def _synced(self) -> bool:
        return getattr(self, "sync_group", None) is not None and isinstance(self.norm, nn.BatchNorm1d)

    def _gather_stats(self, row: torch.Tensor):
        """the statistics rows of all ranks in rank order [W, len] (one small all-gather), and this rank's index"""
        from torch import distributed as dist
        world, rank = dist.get_world_size(self.sync_group), dist.get_rank(self.sync_group)
        table = torch.empty(world, row.numel(), dtype=row.dtype, device=row.device)
        dist.all_gather(list(table.unbind(0)), row, group=self.sync_group)
        return table, world, rank

    def _desc(self, precision: int, keep: list):
        E = self.atten.in_proj_weight.shape[1]
        bn = isinstance(self.norm, nn.BatchNorm1d)
        small = [ops._f32c(t.detach()).contiguous() for t in ((self.norm.weight, self.norm.bias, self.norm.running_mean, self.norm.running_var)
                                                              if bn else (self.norm.weight, self.norm.bias))]
        keep.extend(small)
        return _lib.DcmhtHead(_clip._linear_desc(self.atten.in_proj_weight[2 * E:3 * E], self.atten.in_proj_bias[2 * E:3 * E], precision, keep),
                              _clip._linear_desc(self.atten.out_proj.weight, self.atten.out_proj.bias, precision, keep),
                              int(bn), float(self.norm.eps), small[0].data_ptr(), small[1].data_ptr(),
                              small[2].data_ptr() if bn else None, small[3].data_ptr() if bn else None,
                              _clip._linear_desc(self.fc2.weight, self.fc2.bias, precision, keep))

    def _native(self, data: torch.Tensor) -> torch.Tensor:
        """xmh_head_dcmht: the five launches below from one C call."""
        data = ops._f32c(data).contiguous()
        B, E = data.shape
        desc, precision = _clip._cached_desc(self, self._desc, params=list(self.parameters()) + list(self.buffers()), slot="dcmht")
        nbytes = lib.xmh_head_workspace_bytes(B, E, precision)
        ws = _clip._workspace(nbytes, data.device)
        probs = torch.empty(B, self.fc2.weight.shape[0], dtype=torch.float32, device=data.device)
        check(lib.xmh_head_dcmht(ctypes.byref(desc), ptr(data), B, precision, ptr(probs), None, None, ptr(ws), nbytes, current_stream()),
              "xmh_head_dcmht")
        return probs

    def forward(self, data: torch.Tensor) -> torch.Tensor:
        return self._train(data) if self.training else self._infer(data)

    def _train_args(self):
        """(xmh_dcmht_train, the tensors it points into) for the parameters as they are now"""
        E = self.atten.in_proj_weight.shape[1]
        bn = isinstance(self.norm, nn.BatchNorm1d)
        ts = [_param(t) for t in (self.atten.in_proj_weight, self.atten.in_proj_bias, self.atten.out_proj.weight, self.atten.out_proj.bias,
                                  self.norm.weight, self.norm.bias, self.fc2.weight, self.fc2.bias)]
        run = [None, None]
        momentum = 0.0
        if bn and self.norm.track_running_stats:
            if self.norm.momentum is None:
                raise NotImplementedError("BatchNorm1d(momentum=None) (cumulative average) is not built; the reference uses 0.1")
            run, momentum = [_param(self.norm.running_mean), _param(self.norm.running_var)], float(self.norm.momentum)
        h = _lib.DcmhtTrain(ts[0].data_ptr() + 2 * E * E * 4, ts[1].data_ptr() + 2 * E * 4, ts[2].data_ptr(), ts[3].data_ptr(),
                            ts[4].data_ptr(), ts[5].data_ptr(), run[0].data_ptr() if run[0] is not None else None,
                            run[1].data_ptr() if run[1] is not None else None, ts[6].data_ptr(), ts[7].data_ptr(), int(bn),
                            float(self.norm.eps), momentum)
        return h, ts + run

    def _train_forward(self, data: torch.Tensor):
        """xmh_head_dcmht_train_forward -> (probs, x as the kernels read it, the saved buffer)"""
        if data.dim() != 2:
            raise ValueError("a DCMHT head in train mode takes [B, E] embeddings, got %s" % (tuple(data.shape),))
        x = ops._f32c(data.detach()).contiguous()
        B, E = x.shape
        N = self.fc2.weight.shape[0]
        bn = isinstance(self.norm, nn.BatchNorm1d)
        synced = self._synced()
        if bn and B == 1 and not synced:                     # across ranks one local row is legal: the library refuses a global batch of one
            raise ValueError("Expected more than 1 value per channel when training, got input size %s" % (tuple(data.shape),))
        h, keep = self._train_args()
        nws = ctypes.c_size_t(0)
        nsaved = lib.xmh_head_dcmht_train_bytes(B, E, N, ctypes.byref(nws))
        saved, ws = _clip._workspace(nsaved, x.device), _clip._workspace(nws.value, x.device)
        probs = torch.empty(B, N, dtype=torch.float32, device=x.device)
        if synced:                                           # statistics -> all-gather of one small double row per rank -> the rest
            row = torch.empty(lib.xmh_head_dcmht_stats_len(E), dtype=torch.float64, device=x.device)
            check(lib.xmh_head_dcmht_train_forward_stats(ctypes.byref(h), ptr(x), B, E, N, ptr(saved), nsaved, ptr(ws), nws.value, ptr(row),
                                                         current_stream()), "xmh_head_dcmht_train_forward_stats")
            table, world, _ = self._gather_stats(row)
            check(lib.xmh_head_dcmht_train_forward_apply(ctypes.byref(h), ptr(x), B, E, N, ptr(table), world, ptr(probs), ptr(saved), nsaved,
                                                         ptr(ws), nws.value, current_stream()), "xmh_head_dcmht_train_forward_apply")
        else:
            check(lib.xmh_head_dcmht_train_forward(ctypes.byref(h), ptr(x), B, E, N, ptr(probs), ptr(saved), nsaved, ptr(ws), nws.value,
                                                   current_stream()), "xmh_head_dcmht_train_forward")
        if bn and self.norm.track_running_stats and self.norm.num_batches_tracked is not None:
            self.norm.num_batches_tracked.add_(1)
        del keep
        return probs, x, saved

    def _train(self, data: torch.Tensor) -> torch.Tensor:
        params = (self.atten.in_proj_weight, self.atten.in_proj_bias, self.atten.out_proj.weight, self.atten.out_proj.bias,
                  self.norm.weight, self.norm.bias, self.fc2.weight, self.fc2.bias)
        if torch.is_grad_enabled() and (data.requires_grad or any(p.requires_grad for p in params)):
            return _DCMHTTrain.apply(self, data, *params)
        return self._train_forward(data)[0]

    @torch.no_grad()
    def _infer(self, data: torch.Tensor) -> torch.Tensor:
        if _clip.NATIVE_FORWARD and data.dim() == 2:
            return self._native(data)
        E = data.shape[1]
        wv, bv = self.atten.in_proj_weight[2 * E:3 * E], self.atten.in_proj_bias[2 * E:3 * E]
        v = ops.gemm_nt(data, wv, bv)
        o = ops.gemm_nt(v, self.atten.out_proj.weight, self.atten.out_proj.bias)
        if isinstance(self.norm, nn.BatchNorm1d):
            n = ops.affine_cols(o, self.norm.running_mean, self.norm.running_var, self.norm.weight, self.norm.bias, self.norm.eps)
        else:
            n = ops.layernorm(o, self.norm.weight, self.norm.bias, self.norm.eps)
        f = ops.gemm_nt(n, self.fc2.weight, self.fc2.bias, act=ops.ACT_RELU)
        return ops.pair_softmax(f)


def _param(t: torch.Tensor) -> torch.Tensor:
    """a parameter or buffer as the train kernels read it: fp32, contiguous, on the device, in place (no copy: the running statistics
    are written through this pointer and the gradients must have the parameter's own layout)"""
    t = t.detach()
    if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
        raise RuntimeError("train-mode heads need contiguous fp32 CUDA/HIP parameters (got %s %s); there is no CPU fallback"
                           % (t.dtype, t.device))
    return t


class _DCMHTTrain(torch.autograd.Function):
    """forward = xmh_head_dcmht_train_forward, backward = xmh_head_dcmht_backward.  The q and k thirds of in_proj_weight /
    in_proj_bias receive exact zeros (softmax over one key: their gradient is mathematically zero)."""

    @staticmethod
    def forward(ctx, mod, data, *params):
        probs, x, saved = mod._train_forward(data)
        ctx.mod, ctx.meta = mod, (data.shape, data.dtype)
        ctx.versions = [p._version for p in params]
        ctx.save_for_backward(x, saved)
        return probs

    @staticmethod
    @torch.autograd.function.once_differentiable      # the gradient kernels are not themselves differentiable: fail loudly on double backward
    def backward(ctx, g):
        x, saved = ctx.saved_tensors
        mod = ctx.mod
        h, keep = mod._train_args()
        params = keep[:8]
        if [p._version for p in params] != ctx.versions:
            raise RuntimeError("a parameter of the DCMHT head was modified in place between forward and backward")
        B, E = x.shape
        N = params[6].shape[0]
        need = ctx.needs_input_grad
        gp = [(torch.zeros_like(p) if i < 2 else torch.empty_like(p)) if need[2 + i] else None for i, p in enumerate(params)]
        gx = torch.empty_like(x) if need[1] else None
        off = (2 * E * E * 4, 2 * E * 4)                                        # the v third of in_proj_weight / in_proj_bias
        grads = _lib.DcmhtGrads(*[None if t is None else t.data_ptr() + (off[i] if i < 2 else 0) for i, t in enumerate(gp)],
                                None if gx is None else gx.data_ptr())
        up = g.detach().float().contiguous()
        nws = ctypes.c_size_t(0)
        nsaved = lib.xmh_head_dcmht_train_bytes(B, E, N, ctypes.byref(nws))
        ws = _clip._workspace(nws.value, x.device)
        if mod._synced():
            row = torch.empty(lib.xmh_head_dcmht_stats_len(E), dtype=torch.float64, device=x.device)
            check(lib.xmh_head_dcmht_backward_stats(ctypes.byref(h), ptr(x), ptr(up), B, E, N, ptr(saved), nsaved, ctypes.byref(grads), 0,
                                                    ptr(ws), nws.value, ptr(row), current_stream()), "xmh_head_dcmht_backward_stats")
            table, world, rank = mod._gather_stats(row)
            check(lib.xmh_head_dcmht_backward_apply(ctypes.byref(h), ptr(x), B, E, N, ptr(table), world, rank, ptr(saved), nsaved,
                                                    ctypes.byref(grads), 0, ptr(ws), nws.value, current_stream()),
                  "xmh_head_dcmht_backward_apply")
        else:
            check(lib.xmh_head_dcmht_backward(ctypes.byref(h), ptr(x), ptr(up), B, E, N, ptr(saved), nsaved, ctypes.byref(grads), 0, ptr(ws),
                                              nws.value, current_stream()), "xmh_head_dcmht_backward")
        if gx is not None:
            gx = gx.reshape(ctx.meta[0]).to(ctx.meta[1])
        return (None, gx, *gp)


class _DSPHTrain(torch.autograd.Function):
    """forward = xmh_head_dsph_train_forward, backward = xmh_head_dsph_backward; `keep` is the uint8 keep mask or None"""

    @staticmethod
    def forward(ctx, mod, data, weight, bias, keep):
        y, x = mod._train_forward(data, keep)
        ctx.p, ctx.meta = float(mod.drop_out.p), (data.shape, data.dtype)
        ctx.version = weight._version
        ctx.save_for_backward(x, y, weight, keep)           # y is an output: autograd notices if the caller writes into it
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, y, weight, keep = ctx.saved_tensors
        w = _param(weight)
        if weight._version != ctx.version:
            raise RuntimeError("fc.weight of the DSPH head was modified in place between forward and backward")
        B, E = x.shape
        K = w.shape[0]
        need = ctx.needs_input_grad
        gx = torch.empty_like(x) if need[1] else None
        gw = torch.empty_like(w) if need[2] else None
        gb = torch.empty(K, dtype=torch.float32, device=x.device) if need[3] else None
        up = g.detach().float().contiguous()
        ws = _clip._workspace(B * K * 4, x.device)
        check(lib.xmh_head_dsph_backward(ptr(w), ptr(x), ptr(y), ptr(keep), ctx.p, ptr(up), B, E, K, ptr(gw), ptr(gb), ptr(gx), 0,
                                         ptr(ws), ws.numel(), current_stream()), "xmh_head_dsph_backward")
        if gx is not None:
            gx = gx.reshape(ctx.meta[0]).to(ctx.meta[1])
        return None, gx, gw, gb, None


class DCMHTHashLayer(nn.Module):
    def __init__(self, feature_size=512, outputDim=64, num_heads=8, batch_first=True, hash_func_="softmax"):
        super().__init__()
        if hash_func_ != "softmax":
            raise NotImplementedError("DCMHT is configured with hash_func: softmax in every shipped config")
        self.img_hash = DCMHTModalityHash(feature_size, outputDim, num_heads, layernorm=False)
        self.txt_hash = DCMHTModalityHash(feature_size, outputDim, num_heads, layernorm=True)

    def encode_img(self, embeds):
        return self.img_hash(embeds)

    def encode_txt(self, embeds):
        return self.txt_hash(embeds)

    def forward(self, img_embeds, txt_embeds):
        return self.encode_img(img_embeds), self.encode_txt(txt_embeds)


_DRAW = object()                              # DSPHLinearHash._train(keep=...): draw the mask (None means "no dropout")


class DSPHLinearHash(nn.Module):
    def __init__(self, inputDim=512, outputDim=64):
        super().__init__()
        self.fc = nn.Linear(inputDim, outputDim)
        self.drop_out = nn.Dropout(p=0.2)
        self.generator = None                 # torch.Generator of the module's device for the dropout masks; None: the global one

    def forward(self, data):
        return self._train(data) if self.training else self._infer(data)

    def draw_keep_mask(self, B: int, device):
        """the dropout keep mask of one train-mode forward, uint8 [B, K] on the device, or None when p == 0.  Drawn here, not in
        the library, with ``torch.rand(..., generator=self.generator) >= p`` on the device (``self.generator``: a torch.Generator
        of that device, default None = the device's global one), so a seeded run is reproducible.  The stream differs from
        nn.Dropout's own Philox consumption: bit-identity with the reference's masks is not a goal, their distribution is."""
        p = float(self.drop_out.p)
        if p <= 0.0:
            return None
        if p >= 1.0:
            raise ValueError("dropout p = %g: nothing would be kept" % p)
        K = self.fc.weight.shape[0]
        return (torch.rand(B, K, device=device, generator=self.generator) >= p).view(torch.uint8)   # bool: one 0 / 1 byte each

    def _train_forward(self, data, keep):
        """xmh_head_dsph_train_forward -> (y, x as the kernels read it)"""
        if data.dim() != 2:
            raise ValueError("a DSPH head in train mode takes [B, E] embeddings, got %s" % (tuple(data.shape),))
        x = ops._f32c(data.detach()).contiguous()
        B, E = x.shape
        w, b = _param(self.fc.weight), _param(self.fc.bias)
        y = torch.empty(B, w.shape[0], dtype=torch.float32, device=x.device)
        check(lib.xmh_head_dsph_train_forward(ptr(w), ptr(b), ptr(x), ptr(keep), float(self.drop_out.p) if keep is not None else 0.0,
                                              B, E, w.shape[0], ptr(y), current_stream()), "xmh_head_dsph_train_forward")
        return y, x

    def _train(self, data, keep=_DRAW):
        """train-mode forward; `keep` overrides the drawn mask (uint8 [B, K], or None for no dropout) -- tests replay stored masks"""
        if keep is _DRAW:
            keep = self.draw_keep_mask(data.shape[0], data.device)
        elif keep is not None:
            keep = keep.to(device=data.device, dtype=torch.uint8).contiguous()
        if torch.is_grad_enabled() and (data.requires_grad or self.fc.weight.requires_grad or self.fc.bias.requires_grad):
            return _DSPHTrain.apply(self, data, self.fc.weight, self.fc.bias, keep)
        return self._train_forward(data, keep)[0]

    @torch.no_grad()
    def _infer(self, data):
        if _clip.NATIVE_FORWARD and data.dim() == 2:
            data = ops._f32c(data).contiguous()
            B, E = data.shape
            desc, precision = _clip._cached_desc(self, lambda prec, keep: _clip._linear_desc(self.fc.weight, self.fc.bias, prec, keep), slot="dsph")
            nbytes = lib.xmh_head_workspace_bytes(B, E, precision)
            ws = _clip._workspace(nbytes, data.device)
            out = torch.empty(B, self.fc.weight.shape[0], dtype=torch.float32, device=data.device)
            check(lib.xmh_head_dsph(ctypes.byref(desc), ptr(data), B, precision, ptr(out), None, None, None, None, ptr(ws), nbytes,
                                    current_stream()), "xmh_head_dsph")
            return out
        return ops.gemm_nt(data, self.fc.weight, self.fc.bias, act=ops.ACT_TANH)


class DSPHHashLayer(nn.Module):
    def __init__(self, inputDim=512, outputDim=64):
        super().__init__()
        self.img_hash = DSPHLinearHash(inputDim, outputDim)
        self.txt_hash = DSPHLinearHash(inputDim, outputDim)

    def encode_img(self, embeds):
        return self.img_hash(embeds)

    def encode_txt(self, embeds):
        return self.txt_hash(embeds)

    def forward(self, img_embeds, txt_embeds):
        return self.encode_img(img_embeds), self.encode_txt(txt_embeds)


# ---- DNPH (reference models/DNPH/hash/hash.py) -----------------------------------------------------------------------------------------
def _weights_init_kaiming(fc: nn.Linear) -> nn.Linear:
    """the Linear branch of the reference's ``weights_init_kaiming`` (models/common/hash.py:5-10)"""
    nn.init.kaiming_uniform_(fc.weight, mode="fan_out")
    nn.init.constant_(fc.bias, 0.0)
    return fc


def _linear_f32(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """x w^T + b as the exact-fp32 product (xmh_gemm_nt_f32 at XMH_PREC_F32), whatever the package's precision mode is: the
    class-prediction layers feed a cross-entropy, in training only -> (y, x as the kernel read it)"""
    if x.dim() != 2:
        raise ValueError("a DNPH prediction layer takes [B, E] embeddings, got %s" % (tuple(x.shape),))
    x = ops._f32c(x.detach()).contiguous()
    w, b = _param(weight), _param(bias)
    B, E = x.shape
    N = w.shape[0]
    y = torch.empty(B, N, dtype=torch.float32, device=x.device)
    check(lib.xmh_gemm_nt_f32(ptr(x), E, ptr(w), E, ptr(b), None, 0, ptr(y), N, B, N, E, ops.ACT_NONE, ops.PREC_F32, current_stream()),
          "xmh_gemm_nt_f32")
    return y, x


class _LinearTrain(torch.autograd.Function):
    """forward = xmh_gemm_nt_f32 (exact fp32), backward = xmh_linear_backward"""

    @staticmethod
    def forward(ctx, data, weight, bias):
        y, x = _linear_f32(data, weight, bias)
        ctx.meta, ctx.version = (data.shape, data.dtype), weight._version
        ctx.save_for_backward(x, weight)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable      # the gradient kernels are not themselves differentiable: fail loudly on double backward
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        w = _param(weight)
        if weight._version != ctx.version:
            raise RuntimeError("fc.weight of a DNPH prediction layer was modified in place between forward and backward")
        B, E = x.shape
        N = w.shape[0]
        need = ctx.needs_input_grad
        gx = torch.empty_like(x) if need[0] else None
        gw = torch.empty_like(w) if need[1] else None
        gb = torch.empty(N, dtype=torch.float32, device=x.device) if need[2] else None
        up = g.detach().float().contiguous()
        check(lib.xmh_linear_backward(ptr(w), ptr(x), ptr(up), B, E, N, ptr(gw), ptr(gb), ptr(gx), 0, None, 0, current_stream()),
              "xmh_linear_backward")
        if gx is not None:
            gx = gx.reshape(ctx.meta[0]).to(ctx.meta[1])
        return gx, gw, gb


class DNPHLinearHash(DSPHLinearHash):
    """reference LinearHash of DNPH (:9-19): DSPH's Linear / Dropout(0.2) / tanh head, ``fc`` initialised by weights_init_kaiming"""

    def __init__(self, inputDim=512, outputDim=64):
        super().__init__(inputDim, outputDim)
        _weights_init_kaiming(self.fc)


class DNPHPreLayer(nn.Module):
    """reference Pre_Layer (:22-30): the class-prediction layer, ``fc`` [nb_class, inputdim].  With a graph to build (a parameter or
    the input requires grad, grad mode on) the forward goes through ``_LinearTrain``; otherwise it is the same product with nothing
    kept.  There is no dropout or normalisation: .train() / .eval() compute the same numbers."""

    def __init__(self, inputdim=512, nb_class=80):
        super().__init__()
        self.fc = _weights_init_kaiming(nn.Linear(inputdim, nb_class))

    def forward(self, data):
        if torch.is_grad_enabled() and (data.requires_grad or self.fc.weight.requires_grad or self.fc.bias.requires_grad):
            return _LinearTrain.apply(data, self.fc.weight, self.fc.bias)
        return _linear_f32(data, self.fc.weight, self.fc.bias)[0]


class DNPHHashLayer(nn.Module):
    """reference HashLayer of DNPH (:32-67) under its attribute names, so that a reference checkpoint loads strictly: two outputs per
    modality, the code (``image_hash`` / ``text_hash``) and the class logits (``image_pre`` / ``text_pre``).  The reference's model
    never hands ``num_classes`` on, so the prediction layers have 80 outputs whatever ``numclass`` is."""

    def __init__(self, inputDim=512, outputDim=64, num_classes=80):
        super().__init__()
        self.image_hash = DNPHLinearHash(inputDim=inputDim, outputDim=outputDim)
        self.text_hash = DNPHLinearHash(inputDim=inputDim, outputDim=outputDim)
        self.image_pre = DNPHPreLayer(inputdim=inputDim, nb_class=num_classes)
        self.text_pre = DNPHPreLayer(inputdim=inputDim, nb_class=num_classes)

    @staticmethod
    def _encode(hash_mod, pre_mod, embeds, keep):
        code = hash_mod._train(embeds, keep) if hash_mod.training and keep is not _DRAW else hash_mod(embeds)
        return code, pre_mod(embeds)

    def encode_img(self, embeds, keep=_DRAW):
        """-> (hash, pre); `keep` replays a stored dropout mask in train mode (uint8 [B, K], or None for no dropout)"""
        return self._encode(self.image_hash, self.image_pre, embeds, keep)

    def encode_txt(self, embeds, keep=_DRAW):
        return self._encode(self.text_hash, self.text_pre, embeds, keep)

    def quantization(self, code):
        """reference :53-54, tanh_hash; called by nothing, in the reference or here (the heads apply their own tanh)"""
        return torch.tanh(code)

    def forward(self, img_embeds, txt_embeds):
        img_hash, img_pre = self.encode_img(img_embeds)
        txt_hash, txt_pre = self.encode_txt(txt_embeds)
        return img_hash, txt_hash, img_pre, txt_pre
