"""CLIP ViT-B/32 image and text towers executed by libxmh.so.

The ``nn.Module`` tree below exists to hold parameters under the reference's state_dict key names
(``visual.conv1.weight``, ``transformer.resblocks.3.attn.in_proj_weight`` ... -- SURVEY 8c), so reference
checkpoints load with ``load_state_dict``; none of its torch ``forward`` methods is ever called.  The forward
pass is the kernel chain of SURVEY 2.2:

  image: im2col -> GEMM(conv1) -> cls/pos/ln_pre -> 12 x [LN, GEMM qkv, attention, GEMM out + residual,
         LN, GEMM c_fc + QuickGELU, GEMM c_proj + residual] -> ln_post -> GEMM proj
         (reference models/CLIP/model.py:232-268, :167-197)
  text : embed + pos -> 12 blocks with the causal mask (+ key padding mask) -> ln_final -> GEMM
         text_projection -> EOS row (reference :373-396)

Differences, deliberate: activations are token-major [B, L, D] (the reference permutes to LND); attention weights
are not materialised (no in-scope caller consumes them); with ``return_patches=False`` ln_post / the projection run
on the cls / EOS row only (the reference projects every token and then discards all but one, :257-265)."""
from __future__ import annotations

import ctypes
import os
import weakref
from collections import OrderedDict

import torch
import torch.nn as nn

from .. import _lib, ops
from .._lib import check, current_stream, lib, ptr

# The towers run through the whole-tower entry points of libxmh.so (xmh_vit_b32_forward / xmh_text_forward /
# xmh_clip_blocks_forward: one C call enqueues the ~150 launches).  XMH_FORWARD=ops keeps the per-primitive chain below
# (the same kernels in the same order, enqueued from Python) -- the tests run both and compare them bit for bit.
TEXT_PACKING = os.environ.get("XMH_TEXT_PACKING", "1") != "0"     # module switch (tests flip it): run the text tower without its padding rows
NATIVE_FORWARD = os.environ.get("XMH_FORWARD", "native") != "ops"



def _transposed(module, name: str) -> torch.Tensor:
    """`x @ proj` runs as gemm_nt(x, proj^T): keep ONE contiguous transpose per parameter version (a fresh copy per forward
    would defeat the fp16 weight cache of ops.gemm_nt and cost a host sync each time)."""
    p = getattr(module, name)
    key = (p.data_ptr(), p._version)
    cache = module.__dict__.setdefault("_xmh_transposed", {})
    hit = cache.get(name)
    if hit is None or hit[0] != key:
        hit = (key, p.detach().t().contiguous())
        cache[name] = hit
    return hit[1]


def _addr(t):
    return None if t is None else t.data_ptr()


def _linear_desc(W: torch.Tensor, bias, precision: int, keep: list) -> "_lib.Linear":
    """xmh_linear of a [N, K] weight; `keep` collects every tensor whose address goes into the descriptor."""
    W2 = ops._f32c(W.detach())
    W2 = W2 if W2.is_contiguous() else W2.contiguous()
    hi = lo = None
    if precision != ops.PREC_F32X and W2.shape[1] % 32 == 0:
        hi, lo = ops._half_weight(W2)
    b = None if bias is None else ops._f32c(bias.detach())
    keep.extend((W2, hi, lo, b))
    return _lib.Linear(_addr(W2), _addr(hi), _addr(lo), _addr(b), W2.shape[0], W2.shape[1])


def _blocks_desc(blocks, precision: int, keep: list):
    arr = (_lib.ClipBlock * len(blocks))()
    for i, blk in enumerate(blocks):
        ln = [ops._f32c(t.detach()) for t in (blk.ln_1.weight, blk.ln_1.bias, blk.ln_2.weight, blk.ln_2.bias)]
        keep.extend(ln)
        arr[i] = _lib.ClipBlock(_addr(ln[0]), _addr(ln[1]), _addr(ln[2]), _addr(ln[3]),
                                _linear_desc(blk.attn.in_proj_weight, blk.attn.in_proj_bias, precision, keep),
                                _linear_desc(blk.attn.out_proj.weight, blk.attn.out_proj.bias, precision, keep),
                                _linear_desc(blk.mlp.c_fc.weight, blk.mlp.c_fc.bias, precision, keep),
                                _linear_desc(blk.mlp.c_proj.weight, blk.mlp.c_proj.bias, precision, keep))
    return arr


_descriptors = weakref.WeakKeyDictionary()     # module -> {slot: (key, descriptor, tensors it points into)}; not in the module's
                                                # __dict__: ctypes structs holding pointers cannot be deep-copied / pickled


def _cached_desc(module, build, params=None, slot="tower"):
    """descriptor of `module`'s weights for the current precision, rebuilt when any parameter moved or changed in place."""
    precision = ops._precision
    key = (precision,) + tuple((p.data_ptr(), p._version) for p in (module.parameters() if params is None else params))
    slots = _descriptors.setdefault(module, {})
    hit = slots.get(slot)
    if hit is None or hit[0] != key:
        keep = []
        hit = (key, build(precision, keep), keep)
        slots[slot] = hit
    return hit[1], precision


_workspace = _lib.workspace                      # the name heads.py and mith.py know it by


class _Block(nn.Module):
    def __init__(self, width: int, heads: int):
        super().__init__()
        self.attn = nn.MultiheadAttention(width, heads)
        self.ln_1 = nn.LayerNorm(width)
        self.mlp = nn.Sequential(OrderedDict([("c_fc", nn.Linear(width, width * 4)), ("gelu", nn.Identity()),
                                              ("c_proj", nn.Linear(width * 4, width))]))
        self.ln_2 = nn.LayerNorm(width)
        self.heads = heads

    def run(self, x: torch.Tensor, causal: bool, kpm) -> torch.Tensor:
        h = ops.layernorm(x, self.ln_1.weight, self.ln_1.bias)
        qkv = ops.gemm_nt(h, self.attn.in_proj_weight, self.attn.in_proj_bias)
        a = ops.attention(qkv, self.heads, causal=causal, key_padding_mask=kpm)
        x = ops.gemm_nt(a, self.attn.out_proj.weight, self.attn.out_proj.bias, residual=x, out=x)
        h = ops.layernorm(x, self.ln_2.weight, self.ln_2.bias)
        f = ops.gemm_nt(h, self.mlp.c_fc.weight, self.mlp.c_fc.bias, act=ops.ACT_QUICKGELU)
        return ops.gemm_nt(f, self.mlp.c_proj.weight, self.mlp.c_proj.bias, residual=x, out=x)


class Transformer(nn.Module):
    def __init__(self, width: int, layers: int, heads: int):
        super().__init__()
        self.width, self.layers = width, layers
        self.resblocks = nn.Sequential(*[_Block(width, heads) for _ in range(layers)])

    def run(self, x: torch.Tensor, causal: bool = False, key_padding_mask=None) -> torch.Tensor:
        """x [B, L, D] fp32 on the GPU; updated in place and returned."""
        if not NATIVE_FORWARD or not x.is_contiguous() or x.dtype != torch.float32:
            for blk in self.resblocks:
                x = blk.run(x, causal, key_padding_mask)
            return x
        B, L, D = x.shape
        blocks, precision = _cached_desc(self, lambda prec, keep: _blocks_desc(list(self.resblocks), prec, keep))
        kpm = None if key_padding_mask is None else key_padding_mask.to(device=x.device, dtype=torch.uint8).contiguous()
        nbytes = lib.xmh_clip_workspace_bytes(B, L, D, 0, 0, precision)
        ws = _workspace(nbytes, x.device)
        check(lib.xmh_clip_blocks_forward(blocks, len(self.resblocks), D, self.resblocks[0].heads if len(self.resblocks) else 1,
                                          ptr(x), B, L, int(causal), ptr(kpm), precision, ptr(ws), nbytes, current_stream()),
              "xmh_clip_blocks_forward")
        return x


    # per-layer record of xmh_clip_blocks_forward_saved (include/xmh.h): field -> width in units of D
    # (the C side states the same layout once, in csrc/xmh_clip_record.h: saved_record)
    SAVED_FIELDS = (("x_in", 1), ("ln1", 1), ("qkv", 3), ("attn", 1), ("x_mid", 1), ("ln2", 1), ("fc_pre", 4), ("fc_act", 4))

    def run_saved(self, x: torch.Tensor, causal: bool = False, key_padding_mask=None):
        """The forward of `run` with the activations a backward pass of the blocks (models/CLIP/model.py:167-197) reads kept per
        layer: returns (x, saved) with x updated in place exactly as `run` leaves it and saved = one dict per layer
        of [B, L, n*D] fp32 views into one device buffer (16 * B*L*D floats per layer).  Native executor only."""
        if not x.is_cuda or not x.is_contiguous() or x.dtype != torch.float32 or x.dim() != 3:
            raise ValueError("run_saved takes a contiguous fp32 [B, L, D] tensor on the GPU")
        B, L, D = x.shape
        layers = len(self.resblocks)
        blocks, precision = _cached_desc(self, lambda prec, keep: _blocks_desc(list(self.resblocks), prec, keep))
        kpm = None if key_padding_mask is None else key_padding_mask.to(device=x.device, dtype=torch.uint8).contiguous()
        nbytes = lib.xmh_clip_workspace_bytes(B, L, D, 0, 0, precision)
        ws = _workspace(nbytes, x.device)
        sbytes = lib.xmh_clip_saved_bytes(B, L, D, layers)
        buf = torch.empty(sbytes // 4, dtype=torch.float32, device=x.device)
        check(lib.xmh_clip_blocks_forward_saved(blocks, layers, D, self.resblocks[0].heads if layers else 1, ptr(x), B, L, int(causal),
                                                ptr(kpm), precision, ptr(ws), nbytes, ptr(buf), sbytes, current_stream()),
              "xmh_clip_blocks_forward_saved")
        saved, per_layer, md = [], 16 * B * L * D, B * L * D
        for i in range(layers):
            rec, off = {}, i * per_layer
            for name, n in self.SAVED_FIELDS:
                rec[name] = buf[off:off + n * md].view(B, L, n * D)
                off += n * md
            saved.append(rec)
        return x, saved

    # the twelve parameters of a block in the member order of xmh_clip_block_grads (include/xmh.h)
    @staticmethod
    def _train_params(blk):
        return (blk.ln_1.weight, blk.ln_1.bias, blk.attn.in_proj_weight, blk.attn.in_proj_bias, blk.attn.out_proj.weight,
                blk.attn.out_proj.bias, blk.ln_2.weight, blk.ln_2.bias, blk.mlp.c_fc.weight, blk.mlp.c_fc.bias, blk.mlp.c_proj.weight,
                blk.mlp.c_proj.bias)

    def run_train(self, x: torch.Tensor, causal: bool = False, key_padding_mask=None) -> torch.Tensor:
        """The block stack in exact fp32 behind torch.autograd: x [B, L, D] is copied, never written; the result carries
        a graph whose backward is ONE call of xmh_clip_blocks_backward over the record xmh_clip_blocks_forward_saved kept.  Gradients
        go to exactly the parameters with requires_grad (and to x if it requires grad).  With nothing to differentiate -- under
        no_grad, or nothing requires grad -- this is `run` in exact mode on a copy, and no record is kept."""
        if not x.is_cuda or x.dim() != 3:
            raise ValueError("run_train takes a [B, L, D] tensor on the GPU; there is no CPU fallback")
        params = [p for blk in self.resblocks for p in self._train_params(blk)]
        kpm = None if key_padding_mask is None else key_padding_mask.to(device=x.device, dtype=torch.uint8).contiguous()
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params)):
            return _BlocksTrain.apply(self, bool(causal), kpm, x, *params)
        return _train_forward(self, x, bool(causal), kpm, params, keep_record=False)[0]


def _exact_desc(tr, params, keep: list):
    """xmh_clip_block array over the parameters IN PLACE (fp32 weights only: no operand planes, nothing cached across steps)"""
    for p in params:
        if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
            raise RuntimeError("run_train needs contiguous fp32 CUDA/HIP parameters (got %s %s); there is no CPU fallback" % (p.dtype, p.device))
    arr = (_lib.ClipBlock * len(tr.resblocks))()
    for i in range(len(tr.resblocks)):
        l1w, l1b, qw, qb, ow, ob, l2w, l2b, fw, fb, pw, pb = (p.detach() for p in params[12 * i:12 * i + 12])
        lin = lambda w, b: _lib.Linear(w.data_ptr(), None, None, b.data_ptr(), w.shape[0], w.shape[1])      # noqa: E731
        arr[i] = _lib.ClipBlock(l1w.data_ptr(), l1b.data_ptr(), l2w.data_ptr(), l2b.data_ptr(), lin(qw, qb), lin(ow, ob), lin(fw, fb), lin(pw, pb))
    keep.extend(params)
    return arr


def _train_forward(tr, x, causal, kpm, params, keep_record=True):
    """-> (y, record buffer or None): exact-mode forward on a copy of x"""
    y = x.detach().to(torch.float32).contiguous()
    y = y.clone() if y.data_ptr() == x.data_ptr() else y
    B, L, D = y.shape
    layers = len(tr.resblocks)
    heads = tr.resblocks[0].heads if layers else 1
    keep = []
    blocks = _exact_desc(tr, params, keep)
    nbytes = lib.xmh_clip_workspace_bytes(B, L, D, 0, 0, ops.PREC_F32X)
    ws = _workspace(nbytes, y.device)
    if not keep_record:
        check(lib.xmh_clip_blocks_forward(blocks, layers, D, heads, ptr(y), B, L, int(causal), ptr(kpm), ops.PREC_F32X, ptr(ws), nbytes,
                                          current_stream()), "xmh_clip_blocks_forward")
        return y, None
    sbytes = lib.xmh_clip_saved_bytes(B, L, D, layers)
    buf = torch.empty(max(sbytes // 4, 1), dtype=torch.float32, device=y.device)
    check(lib.xmh_clip_blocks_forward_saved(blocks, layers, D, heads, ptr(y), B, L, int(causal), ptr(kpm), ops.PREC_F32X, ptr(ws), nbytes,
                                            ptr(buf), sbytes, current_stream()), "xmh_clip_blocks_forward_saved")
    return y, buf


class _BlocksTrain(torch.autograd.Function):
    """forward = xmh_clip_blocks_forward_saved (exact mode), backward = xmh_clip_blocks_backward"""

    @staticmethod
    def forward(ctx, tr, causal, kpm, x, *params):
        y, buf = _train_forward(tr, x, causal, kpm, params)
        ctx.tr, ctx.causal, ctx.kpm, ctx.meta = tr, causal, kpm, (x.shape, x.dtype)
        ctx.save_for_backward(buf, *params)             # saved parameters: autograd notices an in-place change before backward
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable      # the gradient kernels are not themselves differentiable
    def backward(ctx, g):
        buf, *params = ctx.saved_tensors
        tr = ctx.tr
        B, L, D = ctx.meta[0]
        layers = len(tr.resblocks)
        need = ctx.needs_input_grad
        gp = [torch.empty_like(p) if need[4 + i] else None for i, p in enumerate(params)]
        grads = (_lib.ClipBlockGrads * max(layers, 1))()
        for i in range(layers):
            grads[i] = _lib.ClipBlockGrads(*[_addr(t) for t in gp[12 * i:12 * i + 12]])
        dy = g.detach().to(torch.float32).contiguous()
        dy = dy.clone() if dy.data_ptr() == g.data_ptr() else dy      # updated in place: never the caller's tensor
        keep = []
        blocks = _exact_desc(tr, params, keep)
        nbytes = lib.xmh_clip_blocks_backward_ws_bytes(B, L, D)
        ws = _workspace(nbytes, dy.device)
        check(lib.xmh_clip_blocks_backward(blocks, layers, D, tr.resblocks[0].heads if layers else 1, B, L, int(ctx.causal), ptr(ctx.kpm),
                                           ptr(buf), buf.numel() * 4 if layers else 0, ptr(dy), int(need[3]), grads, 0, ptr(ws), nbytes,
                                           current_stream()), "xmh_clip_blocks_backward")
        gx = dy.reshape(ctx.meta[0]).to(ctx.meta[1]) if need[3] else None
        return (None, None, None, gx, *gp)


# ---- the two towers behind torch.autograd --------------------------------------------------------------------------
def _tower_params_ok(params, who):
    for p in params:
        if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
            raise RuntimeError("%s needs contiguous fp32 CUDA/HIP parameters (got %s %s); there is no CPU fallback" % (who, p.dtype, p.device))


def _block_params(tr):
    return [p for blk in tr.resblocks for p in Transformer._train_params(blk)]


def _grad_structs(layers, gp_blocks):
    grads = (_lib.ClipBlockGrads * max(layers, 1))()
    for i in range(layers):
        grads[i] = _lib.ClipBlockGrads(*[_addr(t) for t in gp_blocks[12 * i:12 * i + 12]])
    return grads


def _upstream(g):
    g = g.detach().to(torch.float32)
    return g if g.is_contiguous() else g.contiguous()


_VIT_OWN = 8       # conv1, class_embedding, positional_embedding, ln_pre w/b, ln_post w/b, proj; the blocks' parameters follow


def _vit_params(vis):
    return [vis.conv1.weight, vis.class_embedding, vis.positional_embedding, vis.ln_pre.weight, vis.ln_pre.bias, vis.ln_post.weight,
            vis.ln_post.bias, vis.proj] + _block_params(vis.transformer)


def _vit_exact_desc(vis, params, keep):
    """xmh_vit_weights over the parameters IN PLACE; only `x @ proj` needs a copy (the descriptor holds proj transposed)"""
    _tower_params_ok(params, "encode_image_train")
    conv, cls, pos, lpw, lpb, low, lob, proj = (p.detach() for p in params[:_VIT_OWN])
    tr = vis.transformer
    blocks = _exact_desc(tr, params[_VIT_OWN:], keep)
    proj_t = proj.t().contiguous()
    keep.extend((proj_t, blocks))
    keep.extend(params[:_VIT_OWN])
    width = conv.shape[0]
    heads = tr.resblocks[0].heads if len(tr.resblocks) else max(width // 64, 1)
    return _lib.VitWeights(vis.input_resolution, vis.patch_size, width, heads, len(tr.resblocks), proj.shape[1],
                           _lib.Linear(conv.data_ptr(), None, None, None, width, conv[0].numel()), cls.data_ptr(), pos.data_ptr(), lpw.data_ptr(),
                           lpb.data_ptr(), low.data_ptr(), lob.data_ptr(), _lib.Linear(proj_t.data_ptr(), None, None, None, proj.shape[1], width), blocks)


def _vit_sizes(vis, B):
    L, width = vis.positional_embedding.shape
    return L, width, 3 * vis.patch_size ** 2, vis.proj.shape[1], len(vis.transformer.resblocks)


class _VitTrain(torch.autograd.Function):
    """forward = xmh_vit_train_forward, backward = xmh_vit_backward"""

    @staticmethod
    def forward(ctx, vis, image, *params):
        B = image.shape[0]
        L, width, conv_k, out_dim, layers = _vit_sizes(vis, B)
        keep = []
        desc = _vit_exact_desc(vis, params, keep)
        sbytes = lib.xmh_vit_train_saved_bytes(B, L, width, layers)
        nbytes = lib.xmh_vit_train_ws_bytes(B, L, width, conv_k, out_dim)
        buf = torch.empty(max(sbytes // 4, 1), dtype=torch.float32, device=image.device)
        ws = _workspace(nbytes, image.device)
        out = torch.empty(B, out_dim, dtype=torch.float32, device=image.device)
        check(lib.xmh_vit_train_forward(ctypes.byref(desc), ptr(image), B, ptr(out), ptr(buf), sbytes, ptr(ws), nbytes, current_stream()),
              "xmh_vit_train_forward")
        ctx.vis = vis
        ctx.save_for_backward(image, buf, *params)      # saved parameters: autograd notices an in-place change before backward
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        image, buf, *params = ctx.saved_tensors
        vis = ctx.vis
        B = image.shape[0]
        L, width, conv_k, out_dim, layers = _vit_sizes(vis, B)
        need = ctx.needs_input_grad[2:]
        gp = [torch.empty_like(p) if need[i] else None for i, p in enumerate(params)]
        blocks = _grad_structs(layers, gp[_VIT_OWN:])
        conv, cls, pos, lpw, lpb, low, lob, proj = gp[:_VIT_OWN]
        grads = _lib.VitGrads(_addr(proj), _addr(low), _addr(lob), _addr(lpw), _addr(lpb), _addr(pos), _addr(cls), _addr(conv), blocks)
        keep = []
        desc = _vit_exact_desc(vis, params, keep)
        gg = _upstream(g)
        nbytes = lib.xmh_vit_train_ws_bytes(B, L, width, conv_k, out_dim)
        ws = _workspace(nbytes, gg.device)
        check(lib.xmh_vit_backward(ctypes.byref(desc), ptr(image), B, ptr(buf), buf.numel() * 4, ptr(gg), ctypes.byref(grads), 0, ptr(ws), nbytes,
                                   current_stream()), "xmh_vit_backward")
        return (None, None, *gp)


_TEXT_OWN = 5      # token_embedding.weight, positional_embedding, ln_final w/b, text_projection; the blocks' parameters follow


def _text_train_params(clip):
    return [clip.token_embedding.weight, clip.positional_embedding, clip.ln_final.weight, clip.ln_final.bias, clip.text_projection] + \
        _block_params(clip.transformer)


def _text_exact_desc(clip, params, keep):
    _tower_params_ok(params, "encode_text_train")
    tok, pos, lfw, lfb, proj = (p.detach() for p in params[:_TEXT_OWN])
    tr = clip.transformer
    blocks = _exact_desc(tr, params[_TEXT_OWN:], keep)
    proj_t = proj.t().contiguous()
    keep.extend((proj_t, blocks))
    keep.extend(params[:_TEXT_OWN])
    width = tok.shape[1]
    heads = tr.resblocks[0].heads if len(tr.resblocks) else max(width // 64, 1)
    return _lib.TextWeights(tok.shape[0], pos.shape[0], width, heads, len(tr.resblocks), proj.shape[1], tok.data_ptr(), pos.data_ptr(),
                            lfw.data_ptr(), lfb.data_ptr(), _lib.Linear(proj_t.data_ptr(), None, None, None, proj.shape[1], width), blocks)


class _TextTrain(torch.autograd.Function):
    """forward = xmh_text_train_forward, backward = xmh_text_backward"""

    @staticmethod
    def forward(ctx, clip, ids, kpm, *params):
        B, L = ids.shape
        width, out_dim, layers = params[0].shape[1], params[4].shape[1], len(clip.transformer.resblocks)
        keep = []
        desc = _text_exact_desc(clip, params, keep)
        sbytes = lib.xmh_text_train_saved_bytes(B, L, width, layers)
        nbytes = lib.xmh_text_train_ws_bytes(B, L, width, out_dim)
        buf = torch.empty(max(sbytes // 4, 1), dtype=torch.float32, device=ids.device)
        ws = _workspace(nbytes, ids.device)
        out = torch.empty(B, out_dim, dtype=torch.float32, device=ids.device)
        eos = torch.empty(B, dtype=torch.int32, device=ids.device)
        check(lib.xmh_text_train_forward(ctypes.byref(desc), ptr(ids), ptr(kpm), B, L, ptr(out), ptr(eos), ptr(buf), sbytes, ptr(ws), nbytes,
                                         current_stream()), "xmh_text_train_forward")
        ctx.clip, ctx.kpm = clip, kpm
        ctx.save_for_backward(ids, eos, buf, *params)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        ids, eos, buf, *params = ctx.saved_tensors
        clip = ctx.clip
        B, L = ids.shape
        width, out_dim, layers = params[0].shape[1], params[4].shape[1], len(clip.transformer.resblocks)
        need = ctx.needs_input_grad[3:]
        gp = [torch.empty_like(p) if need[i] else None for i, p in enumerate(params)]
        blocks = _grad_structs(layers, gp[_TEXT_OWN:])
        tok, pos, lfw, lfb, proj = gp[:_TEXT_OWN]
        grads = _lib.TextGrads(_addr(proj), _addr(lfw), _addr(lfb), _addr(pos), _addr(tok), blocks)
        keep = []
        desc = _text_exact_desc(clip, params, keep)
        gg = _upstream(g)
        nbytes = lib.xmh_text_train_ws_bytes(B, L, width, out_dim)
        ws = _workspace(nbytes, gg.device)
        check(lib.xmh_text_backward(ctypes.byref(desc), ptr(ids), ptr(ctx.kpm), ptr(eos), B, L, ptr(buf), buf.numel() * 4, ptr(gg),
                                    ctypes.byref(grads), 0, ptr(ws), nbytes, current_stream()), "xmh_text_backward")
        return (None, None, None, *gp)


class VisionTransformer(nn.Module):
    def __init__(self, input_resolution, patch_size, width, layers, heads, output_dim, return_patches=False):
        super().__init__()
        self.input_resolution, self.patch_size, self.output_dim = input_resolution, patch_size, output_dim
        self.conv1 = nn.Conv2d(3, width, kernel_size=patch_size, stride=patch_size, bias=False)
        self.class_embedding = nn.Parameter(torch.zeros(width))
        self.positional_embedding = nn.Parameter(torch.zeros((input_resolution // patch_size) ** 2 + 1, width))
        self.ln_pre = nn.LayerNorm(width)
        self.transformer = Transformer(width, layers, heads)
        self.ln_post = nn.LayerNorm(width)
        self.proj = nn.Parameter(torch.zeros(width, output_dim))
        self.return_patches = return_patches

    def _desc(self, precision: int, keep: list):
        width = self.conv1.weight.shape[0]
        blocks = _blocks_desc(list(self.transformer.resblocks), precision, keep)
        small = [ops._f32c(t.detach()).contiguous() for t in (self.class_embedding, self.positional_embedding, self.ln_pre.weight,
                                                              self.ln_pre.bias, self.ln_post.weight, self.ln_post.bias)]
        keep.extend(small)
        keep.append(blocks)
        heads = self.transformer.resblocks[0].heads if len(self.transformer.resblocks) else 1
        return _lib.VitWeights(self.input_resolution, self.patch_size, width, heads, len(self.transformer.resblocks), self.proj.shape[1],
                               _linear_desc(self.conv1.weight.reshape(width, -1), None, precision, keep),
                               *[_addr(t) for t in small],
                               _linear_desc(_transposed(self, "proj"), None, precision, keep), blocks)

    def run(self, image: torch.Tensor):
        if NATIVE_FORWARD:
            image = ops._f32c(image).contiguous()
            B, out_dim = image.shape[0], self.proj.shape[1]
            if image.shape[1:] != (3, self.input_resolution, self.input_resolution):
                raise ValueError("image batch is %s, the tower takes [B, 3, %d, %d]" % (tuple(image.shape), self.input_resolution, self.input_resolution))
            L = self.positional_embedding.shape[0]
            desc, precision = _cached_desc(self, self._desc)
            nbytes = lib.xmh_clip_workspace_bytes(B, L, desc.width, 3 * self.patch_size ** 2, out_dim if self.return_patches else 0, precision)
            ws = _workspace(nbytes, image.device)
            if not self.return_patches:
                out = torch.empty(B, out_dim, dtype=torch.float32, device=image.device)
                check(lib.xmh_vit_b32_forward(ctypes.byref(desc), ptr(image), B, precision, ptr(out), None, ptr(ws), nbytes, current_stream()),
                      "xmh_vit_b32_forward")
                return out
            y = torch.empty(B, L, out_dim, dtype=torch.float32, device=image.device)
            check(lib.xmh_vit_b32_forward(ctypes.byref(desc), ptr(image), B, precision, None, ptr(y), ptr(ws), nbytes, current_stream()),
                  "xmh_vit_b32_forward")
            return y[:, 0, :], y[:, 1:, :].permute(1, 0, 2), None                                # cls, tokens (LND), attn
        B = image.shape[0]
        width = self.conv1.weight.shape[0]
        n_patches = self.positional_embedding.shape[0] - 1
        cols = ops.im2col_patch(image, self.patch_size)
        patches = ops.gemm_nt(cols, self.conv1.weight.reshape(width, -1))
        x = ops.vit_assemble(patches, self.class_embedding, self.positional_embedding, self.ln_pre.weight, self.ln_pre.bias, B, n_patches)
        x = self.transformer.run(x)
        proj_t = _transposed(self, "proj")
        L = n_patches + 1
        if not self.return_patches:
            cls = ops.gather_rows(x, group=L, offset=0)
            cls = ops.layernorm(cls, self.ln_post.weight, self.ln_post.bias)
            return ops.gemm_nt(cls, proj_t)
        y = ops.gemm_nt(ops.layernorm(x, self.ln_post.weight, self.ln_post.bias), proj_t)      # [B, L, out]
        return y[:, 0, :], y[:, 1:, :].permute(1, 0, 2), None                                    # cls, tokens (LND), attn


class CLIP(nn.Module):
    def __init__(self, embed_dim, image_resolution, vision_layers, vision_width, vision_patch_size, context_length,
                 vocab_size, transformer_width, transformer_heads, transformer_layers, return_patches=False):
        super().__init__()
        self.context_length, self.vocab_size, self.return_patches = context_length, vocab_size, return_patches
        self.visual = VisionTransformer(image_resolution, vision_patch_size, vision_width, vision_layers, vision_width // 64,
                                        embed_dim, return_patches=return_patches)
        self.transformer = Transformer(transformer_width, transformer_layers, transformer_heads)
        self.token_embedding = nn.Embedding(vocab_size, transformer_width)
        self.positional_embedding = nn.Parameter(torch.zeros(context_length, transformer_width))
        self.ln_final = nn.LayerNorm(transformer_width)
        self.text_projection = nn.Parameter(torch.zeros(transformer_width, embed_dim))
        self.logit_scale = nn.Parameter(torch.ones([]))

    @property
    def dtype(self):
        return self.visual.conv1.weight.dtype

    @torch.no_grad()
    def encode_image(self, image):
        return self.visual.run(image)

    def encode_image_train(self, image):
        """encode_image in exact fp32 behind torch.autograd: the result carries a graph whose backward is ONE call of
        xmh_vit_backward.  Gradients go to exactly the parameters of the image tower with requires_grad (none to the image).  Under
        no_grad, or with nothing to differentiate, this is the plain exact-mode forward and no record is kept."""
        vis = self.visual
        if self.return_patches or vis.return_patches:
            raise NotImplementedError("encode_image_train returns the cls feature only: the patch tokens (return_patches=True) feed MITH's "
                                      "head, whose backward is not built")
        image = ops._f32c(image).contiguous()
        if image.dim() != 4 or image.shape[1:] != (3, vis.input_resolution, vis.input_resolution):
            raise ValueError("image batch is %s, the tower takes [B, 3, %d, %d]" % (tuple(image.shape), vis.input_resolution, vis.input_resolution))
        params = _vit_params(vis)
        if torch.is_grad_enabled() and any(p.requires_grad for p in params):
            return _VitTrain.apply(vis, image, *params)
        B, (L, width), out_dim = image.shape[0], vis.positional_embedding.shape, vis.proj.shape[1]
        keep = []
        desc = _vit_exact_desc(vis, params, keep)
        nbytes = lib.xmh_clip_workspace_bytes(B, L, width, 3 * vis.patch_size ** 2, 0, ops.PREC_F32X)
        ws = _workspace(nbytes, image.device)
        out = torch.empty(B, out_dim, dtype=torch.float32, device=image.device)
        check(lib.xmh_vit_b32_forward(ctypes.byref(desc), ptr(image), B, ops.PREC_F32X, ptr(out), None, ptr(ws), nbytes, current_stream()),
              "xmh_vit_b32_forward")
        return out

    def encode_text_train(self, text, key_padding_mask=None):
        """encode_text in exact fp32 behind torch.autograd, on the padded rows: gradients go to exactly the parameters of the text
        tower with requires_grad (logit_scale is no input: its .grad stays None, as in the reference, where nothing reads it).  Under
        no_grad, or with nothing to differentiate, this is the plain exact-mode forward and no record is kept."""
        if self.return_patches:
            raise NotImplementedError("encode_text_train returns the EOS feature only: the token outputs (return_patches=True) feed MITH's "
                                      "head, whose backward is not built")
        if not text.is_cuda:
            raise RuntimeError("xmh ops need CUDA/HIP tensors (got %s); there is no CPU fallback" % text.device)
        ids = text.to(torch.int64).contiguous()
        if ids.dim() != 2 or ids.shape[1] > self.context_length:
            raise ValueError("token batch is %s, the tower takes [B, L] with L <= %d" % (tuple(ids.shape), self.context_length))
        kpm = None if key_padding_mask is None else key_padding_mask.to(device=ids.device, dtype=torch.uint8).contiguous()
        params = _text_train_params(self)
        if torch.is_grad_enabled() and any(p.requires_grad for p in params):
            return _TextTrain.apply(self, ids, kpm, *params)
        B, L = ids.shape
        width, out_dim = params[0].shape[1], params[4].shape[1]
        keep = []
        desc = _text_exact_desc(self, params, keep)
        nbytes = lib.xmh_clip_workspace_bytes(B, L, width, 0, 0, ops.PREC_F32X)
        ws = _workspace(nbytes, ids.device)
        out = torch.empty(B, out_dim, dtype=torch.float32, device=ids.device)
        check(lib.xmh_text_forward(ctypes.byref(desc), ptr(ids), ptr(kpm), B, L, ops.PREC_F32X, ptr(out), None, None, ptr(ws), nbytes,
                                   current_stream()), "xmh_text_forward")
        return out

    def _text_desc(self, precision: int, keep: list):
        blocks = _blocks_desc(list(self.transformer.resblocks), precision, keep)
        small = [ops._f32c(t.detach()).contiguous() for t in (self.token_embedding.weight, self.positional_embedding,
                                                              self.ln_final.weight, self.ln_final.bias)]
        keep.extend(small)
        keep.append(blocks)
        width = self.token_embedding.weight.shape[1]
        heads = self.transformer.resblocks[0].heads if len(self.transformer.resblocks) else 1
        return _lib.TextWeights(self.token_embedding.weight.shape[0], self.positional_embedding.shape[0], width, heads,
                                len(self.transformer.resblocks), self.text_projection.shape[1], *[_addr(t) for t in small],
                                _linear_desc(_transposed(self, "text_projection"), None, precision, keep), blocks)

    def _text_params(self):
        yield from self.transformer.parameters()
        yield from (self.token_embedding.weight, self.positional_embedding, self.ln_final.weight, self.ln_final.bias, self.text_projection)

    def _encode_text_native(self, text, key_padding_mask, masked_rows="exact"):
        if not text.is_cuda:
            raise RuntimeError("xmh ops need CUDA/HIP tensors; there is no CPU fallback")
        ids = text.to(torch.int64).contiguous()
        B, L = ids.shape
        desc, precision = _cached_desc(self, self._text_desc, params=self._text_params(), slot="text")
        out_dim = self.text_projection.shape[1]
        kpm = None if key_padding_mask is None else key_padding_mask.to(device=ids.device, dtype=torch.uint8).contiguous()
        nbytes = lib.xmh_clip_workspace_bytes(B, L, desc.width, 0, out_dim if self.return_patches else 0, precision)
        ws = _workspace(nbytes, ids.device)
        eos_tok = torch.empty(B, out_dim, dtype=torch.float32, device=ids.device)
        packable = L <= 64 and TEXT_PACKING and precision != 2 and out_dim <= desc.width
        if packable and not self.return_patches:
            # only the EOS embedding is wanted and the attention is causal: the tokens behind a caption's EOS cannot reach it, so the
            # tower runs on the rows up to EOS only (bit-identical output, sum(lengths) / (B L) of the work).  Round 5: the lengths are
            # counted on the device and every launch is sized by its upper bound (xmh_text_forward_packed_dev) -- round 4 read the row
            # count back with .item(), a host sync per caption batch that serialised the two towers' streams.
            check(lib.xmh_text_forward_packed_dev(ctypes.byref(desc), ptr(ids), ptr(kpm), B, L, precision, ptr(eos_tok), None, ptr(ws), nbytes,
                                                  current_stream()), "xmh_text_forward_packed_dev")
            return eos_tok
        if not self.return_patches and kpm is None and L <= 64 and TEXT_PACKING and precision == 2:
            # exact mode (fp32 MFMA; diagnostics): round 4's form of the same packing, the row count read back by the host
            offs = torch.zeros(B + 1, dtype=torch.int32, device=ids.device)
            offs[1:] = torch.cumsum(ids.argmax(dim=1) + 1, 0)
            total = int(offs[B].item())
            if total < 0.9 * B * L:
                check(lib.xmh_text_forward_packed(ctypes.byref(desc), ptr(ids), ptr(offs), total, B, L, precision, ptr(eos_tok), ptr(ws), nbytes,
                                                  current_stream()), "xmh_text_forward_packed")
                return eos_tok
        if not self.return_patches:
            check(lib.xmh_text_forward(ctypes.byref(desc), ptr(ids), ptr(kpm), B, L, precision, ptr(eos_tok), None, None, ptr(ws), nbytes,
                                       current_stream()), "xmh_text_forward")
            return eos_tok
        y = torch.empty(B, L, out_dim, dtype=torch.float32, device=ids.device)
        new_mask = None if kpm is None else (kpm.bool() | (ids == self.vocab_size - 1))
        if packable and masked_rows == "zero" and kpm is not None:
            # the caller reads no row the mask hides (MITH: every consumer of the tokens applies new_mask, models/MITH/hash/hash.py:142-148):
            # the rows behind the last visible position are not computed and come back as zeros; every other row is the padded call's
            check(lib.xmh_text_forward_packed_dev(ctypes.byref(desc), ptr(ids), ptr(kpm), B, L, precision, ptr(eos_tok), ptr(y), ptr(ws), nbytes,
                                                  current_stream()), "xmh_text_forward_packed_dev")
            return eos_tok, y.permute(1, 0, 2), None, new_mask
        check(lib.xmh_text_forward(ctypes.byref(desc), ptr(ids), ptr(kpm), B, L, precision, ptr(eos_tok), ptr(y), None, ptr(ws), nbytes,
                                   current_stream()), "xmh_text_forward")
        return eos_tok, y.permute(1, 0, 2), None, new_mask

    @torch.no_grad()
    def encode_text(self, text, key_padding_mask=None, masked_rows="exact"):
        """reference models/CLIP/model.py:373-396.  ``masked_rows`` (this package's callers only): "exact" returns every token row as the
        reference computes it; "zero" lets the rows that ``key_padding_mask`` hides behind the last visible position come back as zeros
        (not computed) -- for callers that apply the returned mask to everything they read, like the MITH head."""
        if NATIVE_FORWARD:
            return self._encode_text_native(text, key_padding_mask, masked_rows)
        x, eos = ops.text_embed(text, self.token_embedding.weight, self.positional_embedding)
        B, L, _ = x.shape
        kpm = None if key_padding_mask is None else key_padding_mask.to(x.device)
        x = self.transformer.run(x, causal=True, key_padding_mask=kpm)
        proj_t = _transposed(self, "text_projection")
        if not self.return_patches:
            e = ops.gather_rows(x, group=L, idx=eos)
            return ops.gemm_nt(ops.layernorm(e, self.ln_final.weight, self.ln_final.bias), proj_t)
        y = ops.gemm_nt(ops.layernorm(x, self.ln_final.weight, self.ln_final.bias), proj_t)        # [B, L, out]
        eos_tok = ops.gather_rows(y, group=L, idx=eos)
        new_mask = None if kpm is None else (kpm.bool() | (text.to(x.device) == self.vocab_size - 1))
        return eos_tok, y.permute(1, 0, 2), None, new_mask


def round_like_convert_weights(model: CLIP) -> None:
    """The reference casts Conv/Linear/MultiheadAttention/proj tensors to fp16 before loading the checkpoint
    (convert_weights, models/CLIP/model.py:415-436) and the runner later calls .float(): those tensors end up as
    fp16-rounded fp32.  Same rounding here, applied after load."""
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                m.weight.copy_(m.weight.half().float())
                if m.bias is not None:
                    m.bias.copy_(m.bias.half().float())
            if isinstance(m, nn.MultiheadAttention):
                m.in_proj_weight.copy_(m.in_proj_weight.half().float())
                m.in_proj_bias.copy_(m.in_proj_bias.half().float())
        for p in (model.visual.proj, model.text_projection):
            p.copy_(p.half().float())


def build_model(state_dict: dict, return_patches: bool = False) -> CLIP:
    """Infer the architecture from tensor shapes like the reference's build_model (models/CLIP/model.py:438-489);
    ViT checkpoints only (the ResNet branch is unused by every config)."""
    if "visual.proj" not in state_dict:
        raise NotImplementedError("only ViT CLIP checkpoints are supported (no config of the reference uses RN50)")
    vw = state_dict["visual.conv1.weight"].shape[0]
    v_layers = len([k for k in state_dict if k.startswith("visual.") and k.endswith(".attn.in_proj_weight")])
    patch = state_dict["visual.conv1.weight"].shape[-1]
    grid = round((state_dict["visual.positional_embedding"].shape[0] - 1) ** 0.5)
    tw = state_dict["ln_final.weight"].shape[0]
    t_layers = len(set(k.split(".")[2] for k in state_dict if k.startswith("transformer.resblocks")))
    model = CLIP(state_dict["text_projection"].shape[1], patch * grid, v_layers, vw, patch, state_dict["positional_embedding"].shape[0],
                 state_dict["token_embedding.weight"].shape[0], tw, tw // 64, t_layers, return_patches=return_patches)
    sd = {k: v for k, v in state_dict.items() if k not in ("input_resolution", "context_length", "vocab_size")}
    model.load_state_dict(sd)
    round_like_convert_weights(model)
    return model.float().eval()
