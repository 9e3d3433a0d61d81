"""The CLIP block stack and the two towers behind torch.autograd: exact fp32 over the parameters in place, one C call
for the forward that keeps the record and one for the whole backward.  ``Transformer.run_train``, ``CLIP.encode_image_train`` and
``CLIP.encode_text_train`` (models/clip.py) check their arguments and call ``run_blocks`` / ``encode_image`` / ``encode_text`` here;
``CLIP.encode_image_train_tokens`` / ``encode_text_train_tokens`` call ``encode_image_tokens`` / ``encode_text_tokens``.

Which parameter is which is stated once, in the three tables below: (field of the grads struct in include/xmh.h, attribute path on
the module), in the struct's field order.  The parameter list handed to ``Function.apply``, the weights descriptor, the gradient
buffers and the grads struct all follow the table; a tower's list is its own parameters, then the twelve of every block."""
from __future__ import annotations

import ctypes
import operator

import torch

from .. import _lib, ops
from .._lib import check, current_stream, lib, ptr
from .clip import _addr, _text_forward_eos, _vit_forward_cls, _workspace

BLOCK = (("ln1_w", "ln_1.weight"), ("ln1_b", "ln_1.bias"), ("qkv_w", "attn.in_proj_weight"), ("qkv_b", "attn.in_proj_bias"),
         ("out_w", "attn.out_proj.weight"), ("out_b", "attn.out_proj.bias"), ("ln2_w", "ln_2.weight"), ("ln2_b", "ln_2.bias"),
         ("fc_w", "mlp.c_fc.weight"), ("fc_b", "mlp.c_fc.bias"), ("proj_w", "mlp.c_proj.weight"), ("proj_b", "mlp.c_proj.bias"))      # of a _Block
VIT = (("proj", "proj"), ("ln_post_w", "ln_post.weight"), ("ln_post_b", "ln_post.bias"), ("ln_pre_w", "ln_pre.weight"), ("ln_pre_b", "ln_pre.bias"),
       ("pos", "positional_embedding"), ("cls", "class_embedding"), ("conv1", "conv1.weight"))                                       # of a VisionTransformer
TEXT = (("proj", "text_projection"), ("ln_final_w", "ln_final.weight"), ("ln_final_b", "ln_final.bias"), ("pos", "positional_embedding"),
        ("tok", "token_embedding.weight"))                                                                                            # of a CLIP


_get = {path: operator.attrgetter(path) for table in (BLOCK, VIT, TEXT) for _, path in table}      # a third of Module.get_parameter's time per step


def block_params(tr):
    return [_get[path](blk) for blk in tr.resblocks for _, path in BLOCK]


def tower_params(module, table):
    return [_get[path](module) for _, path in table] + block_params(module.transformer)


def _check_params(params, who):
    for p in params:
        if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
            raise RuntimeError("%s needs contiguous fp32 CUDA/HIP parameters (got %s %s); there is no CPU fallback" % (who, p.dtype, p.device))


def _exact_blocks(params):
    """xmh_clip_block array over the blocks' parameters IN PLACE (fp32 weights only: no operand planes, nothing cached across steps)"""
    n = len(BLOCK)
    arr = (_lib.ClipBlock * (len(params) // n))()
    lin = lambda w, b: _lib.Linear(w.data_ptr(), None, None, b.data_ptr(), w.shape[0], w.shape[1])      # noqa: E731
    for i in range(len(arr)):
        p = dict(zip((name for name, _ in BLOCK), params[n * i:n * i + n]))
        arr[i] = _lib.ClipBlock(p["ln1_w"].data_ptr(), p["ln1_b"].data_ptr(), p["ln2_w"].data_ptr(), p["ln2_b"].data_ptr(), lin(p["qkv_w"], p["qkv_b"]),
                                lin(p["out_w"], p["out_b"]), lin(p["fc_w"], p["fc_b"]), lin(p["proj_w"], p["proj_b"]))
    return arr


def _tower_parts(table, params, who, keep: list):
    """what both towers' descriptors are made of -> ({field: own parameter}, xmh_linear of proj, the block array).  Only `x @ proj`
    needs a copy: the descriptor holds proj transposed.  `keep` collects every tensor whose address goes into the descriptor."""
    _check_params(params, who)
    p = dict(zip((name for name, _ in table), params))
    blocks = _exact_blocks(params[len(table):])
    width, out_dim = p["proj"].shape
    proj_t = p["proj"].detach().t().contiguous()
    keep.extend((proj_t, blocks, *params))
    return p, _lib.Linear(proj_t.data_ptr(), None, None, None, out_dim, width), blocks


def vit_desc(vis, params, keep: list):
    """xmh_vit_weights over tower_params(vis, VIT)"""
    p, proj, blocks = _tower_parts(VIT, params, "encode_image_train", keep)
    conv, tr = p["conv1"], vis.transformer
    return _lib.VitWeights(vis.input_resolution, vis.patch_size, proj.k, tr.heads, len(tr.resblocks), proj.n,
                           _lib.Linear(conv.data_ptr(), None, None, None, conv.shape[0], conv[0].numel()), p["cls"].data_ptr(), p["pos"].data_ptr(),
                           p["ln_pre_w"].data_ptr(), p["ln_pre_b"].data_ptr(), p["ln_post_w"].data_ptr(), p["ln_post_b"].data_ptr(), proj, blocks)


def text_desc(clip, params, keep: list):
    """xmh_text_weights over tower_params(clip, TEXT)"""
    p, proj, blocks = _tower_parts(TEXT, params, "encode_text_train", keep)
    tr = clip.transformer
    return _lib.TextWeights(p["tok"].shape[0], p["pos"].shape[0], proj.k, tr.heads, len(tr.resblocks), proj.n, p["tok"].data_ptr(), p["pos"].data_ptr(),
                            p["ln_final_w"].data_ptr(), p["ln_final_b"].data_ptr(), proj, blocks)


def _grad_buffers(params, need):
    return [torch.empty_like(p) if n else None for p, n in zip(params, need)]


def block_grads(gp):
    """xmh_clip_block_grads array over the blocks' gradient buffers (None: not asked for), twelve per block in BLOCK's order"""
    n = len(BLOCK)
    grads = (_lib.ClipBlockGrads * max(len(gp) // n, 1))()
    for i in range(len(gp) // n):
        grads[i] = _lib.ClipBlockGrads(*[_addr(t) for t in gp[n * i:n * i + n]])
    return grads


def tower_grads(struct, table, gp):
    """xmh_vit_grads / xmh_text_grads over a tower's gradient buffers in the order of its parameter list"""
    return struct(*[_addr(t) for t in gp[:len(table)]], block_grads(gp[len(table):]))


def _upstream(g):
    g = g.detach().to(torch.float32)
    return g if g.is_contiguous() else g.contiguous()


# ---- the block stack -------------------------------------------------------------------------------------------------
def blocks_forward(tr, x, causal, kpm, params, keep_record=True):
    """exact-mode forward on a copy of x -> (y, record buffer or None, the descriptor, the tensors it points into)"""
    y = x.detach().to(torch.float32).contiguous()
    y = y.clone() if y.data_ptr() == x.data_ptr() else y
    B, L, D = y.shape
    _check_params(params, "run_train")
    blocks, keep = _exact_blocks(params), list(params)
    layers = len(blocks)
    nbytes = lib.xmh_clip_workspace_bytes(B, L, D, 0, 0, ops.PREC_F32X)
    ws = _workspace(nbytes, y.device)
    if not keep_record:
        check(lib.xmh_clip_blocks_forward(blocks, layers, D, tr.heads, ptr(y), B, L, int(causal), ptr(kpm), ops.PREC_F32X, ptr(ws), nbytes,
                                          current_stream()), "xmh_clip_blocks_forward")
        return y, None, blocks, keep
    sbytes = lib.xmh_clip_saved_bytes(B, L, D, layers)
    buf = torch.empty(max(sbytes // 4, 1), dtype=torch.float32, device=y.device)
    check(lib.xmh_clip_blocks_forward_saved(blocks, layers, D, tr.heads, ptr(y), B, L, int(causal), ptr(kpm), ops.PREC_F32X, ptr(ws), nbytes,
                                            ptr(buf), sbytes, current_stream()), "xmh_clip_blocks_forward_saved")
    return y, buf, blocks, keep


class _BlocksTrain(torch.autograd.Function):
    """forward = xmh_clip_blocks_forward_saved (exact mode), backward = xmh_clip_blocks_backward over the forward's descriptor"""

    @staticmethod
    def forward(ctx, tr, causal, kpm, x, *params):
        y, buf, ctx.blocks, ctx.keep = blocks_forward(tr, x, causal, kpm, params)
        ctx.heads, ctx.causal, ctx.kpm, ctx.meta = tr.heads, causal, kpm, (x.shape, x.dtype)
        ctx.save_for_backward(buf, *params)             # saved parameters: autograd notices an in-place change before backward
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable      # the gradient kernels are not themselves differentiable
    def backward(ctx, g):
        buf, *params = ctx.saved_tensors                # first: this is where that in-place change raises
        B, L, D = ctx.meta[0]
        layers = len(ctx.blocks)
        need = ctx.needs_input_grad
        gp = _grad_buffers(params, need[4:])
        dy = g.detach().to(torch.float32).contiguous()
        dy = dy.clone() if dy.data_ptr() == g.data_ptr() else dy      # updated in place: never the caller's tensor
        nbytes = lib.xmh_clip_blocks_backward_ws_bytes(B, L, D)
        ws = _workspace(nbytes, dy.device)
        check(lib.xmh_clip_blocks_backward(ctx.blocks, layers, D, ctx.heads, B, L, int(ctx.causal), ptr(ctx.kpm), ptr(buf),
                                           buf.numel() * 4 if layers else 0, ptr(dy), int(need[3]), block_grads(gp), 0, ptr(ws), nbytes,
                                           current_stream()), "xmh_clip_blocks_backward")
        gx = dy.reshape(ctx.meta[0]).to(ctx.meta[1]) if need[3] else None
        return (None, None, None, gx, *gp)


def run_blocks(tr, x, causal, kpm):
    params = block_params(tr)
    if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params)):
        return _BlocksTrain.apply(tr, causal, kpm, x, *params)
    return blocks_forward(tr, x, causal, kpm, params, keep_record=False)[0]


# ---- the two towers ----------------------------------------------------------------------------------------------------
def _train_buffers(desc, sbytes, nbytes, B, device):
    """-> (record buffer, workspace, output [B, out_dim]) of a tower's train forward"""
    return (torch.empty(max(sbytes // 4, 1), dtype=torch.float32, device=device), _workspace(nbytes, device),
            torch.empty(B, desc.out_dim, dtype=torch.float32, device=device))


class _VitTrain(torch.autograd.Function):
    """forward = xmh_vit_train_forward, backward = xmh_vit_backward over the forward's descriptor"""

    @staticmethod
    def forward(ctx, vis, image, *params):
        B, L = image.shape[0], vis.positional_embedding.shape[0]
        ctx.keep = []
        ctx.desc = d = vit_desc(vis, params, ctx.keep)
        sbytes = lib.xmh_vit_train_saved_bytes(B, L, d.width, d.layers)
        ctx.nbytes = lib.xmh_vit_train_ws_bytes(B, L, d.width, d.conv1.k, d.out_dim)
        buf, ws, out = _train_buffers(d, sbytes, ctx.nbytes, B, image.device)
        check(lib.xmh_vit_train_forward(ctypes.byref(d), ptr(image), B, ptr(out), ptr(buf), sbytes, ptr(ws), ctx.nbytes, current_stream()),
              "xmh_vit_train_forward")
        ctx.save_for_backward(image, buf, *params)      # saved parameters: autograd notices an in-place change before backward
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        image, buf, *params = ctx.saved_tensors         # first: this is where that in-place change raises
        gp = _grad_buffers(params, ctx.needs_input_grad[2:])
        grads = tower_grads(_lib.VitGrads, VIT, gp)
        gg = _upstream(g)
        ws = _workspace(ctx.nbytes, gg.device)
        check(lib.xmh_vit_backward(ctypes.byref(ctx.desc), ptr(image), image.shape[0], ptr(buf), buf.numel() * 4, ptr(gg), ctypes.byref(grads), 0,
                                   ptr(ws), ctx.nbytes, current_stream()), "xmh_vit_backward")
        return (None, None, *gp)


class _TextTrain(torch.autograd.Function):
    """forward = xmh_text_train_forward, backward = xmh_text_backward over the forward's descriptor"""

    @staticmethod
    def forward(ctx, clip, ids, kpm, *params):
        B, L = ids.shape
        ctx.keep = []
        ctx.desc = d = text_desc(clip, params, ctx.keep)
        sbytes = lib.xmh_text_train_saved_bytes(B, L, d.width, d.layers)
        ctx.nbytes = lib.xmh_text_train_ws_bytes(B, L, d.width, d.out_dim)
        buf, ws, out = _train_buffers(d, sbytes, ctx.nbytes, B, ids.device)
        eos = torch.empty(B, dtype=torch.int32, device=ids.device)
        check(lib.xmh_text_train_forward(ctypes.byref(d), ptr(ids), ptr(kpm), B, L, ptr(out), ptr(eos), ptr(buf), sbytes, ptr(ws), ctx.nbytes,
                                         current_stream()), "xmh_text_train_forward")
        ctx.kpm = kpm
        ctx.save_for_backward(ids, eos, buf, *params)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        ids, eos, buf, *params = ctx.saved_tensors
        B, L = ids.shape
        gp = _grad_buffers(params, ctx.needs_input_grad[3:])
        grads = tower_grads(_lib.TextGrads, TEXT, gp)
        gg = _upstream(g)
        ws = _workspace(ctx.nbytes, gg.device)
        check(lib.xmh_text_backward(ctypes.byref(ctx.desc), ptr(ids), ptr(ctx.kpm), ptr(eos), B, L, ptr(buf), buf.numel() * 4, ptr(gg),
                                    ctypes.byref(grads), 0, ptr(ws), ctx.nbytes, current_stream()), "xmh_text_backward")
        return (None, None, None, *gp)


# ---- the two towers with their token outputs --------------------------------------------------------------------------
def _grad_or_none(g):
    return None if g is None else _upstream(g)


class _VitTokensTrain(torch.autograd.Function):
    """forward = xmh_vit_train_forward_tokens -> (cls [B, E], tokens [B, L - 1, E]), backward = xmh_vit_backward_tokens over the forward's
    descriptor; an output the loss does not use hands None to backward, which the C entry takes as zeros"""

    @staticmethod
    def forward(ctx, vis, image, *params):
        B, L = image.shape[0], vis.positional_embedding.shape[0]
        ctx.set_materialize_grads(False)
        ctx.keep = []
        ctx.desc = d = vit_desc(vis, params, ctx.keep)
        sbytes = lib.xmh_vit_train_tokens_saved_bytes(B, L, d.width, d.layers)
        ctx.nbytes = lib.xmh_vit_train_tokens_ws_bytes(B, L, d.width, d.conv1.k, d.out_dim)
        buf, ws, cls = _train_buffers(d, sbytes, ctx.nbytes, B, image.device)
        tokens = torch.empty(B, L - 1, d.out_dim, dtype=torch.float32, device=image.device)
        check(lib.xmh_vit_train_forward_tokens(ctypes.byref(d), ptr(image), B, ptr(cls), ptr(tokens), ptr(buf), sbytes, ptr(ws), ctx.nbytes,
                                               current_stream()), "xmh_vit_train_forward_tokens")
        ctx.save_for_backward(image, buf, *params)      # saved parameters: autograd notices an in-place change before backward
        return cls, tokens

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_cls, g_tokens):
        image, buf, *params = ctx.saved_tensors         # first: this is where that in-place change raises
        if g_cls is None and g_tokens is None:
            return (None, None, *(None for _ in params))
        gp = _grad_buffers(params, ctx.needs_input_grad[2:])
        grads = tower_grads(_lib.VitGrads, VIT, gp)
        gc, gt = _grad_or_none(g_cls), _grad_or_none(g_tokens)
        ws = _workspace(ctx.nbytes, image.device)
        check(lib.xmh_vit_backward_tokens(ctypes.byref(ctx.desc), ptr(image), image.shape[0], ptr(buf), buf.numel() * 4, ptr(gc), ptr(gt),
                                          ctypes.byref(grads), 0, ptr(ws), ctx.nbytes, current_stream()), "xmh_vit_backward_tokens")
        return (None, None, *gp)


class _TextTokensTrain(torch.autograd.Function):
    """forward = xmh_text_train_forward_tokens -> (eos [B, E], tokens [B, L, E]), backward = xmh_text_backward_tokens"""

    @staticmethod
    def forward(ctx, clip, ids, kpm, *params):
        B, L = ids.shape
        ctx.set_materialize_grads(False)
        ctx.keep = []
        ctx.desc = d = text_desc(clip, params, ctx.keep)
        sbytes = lib.xmh_text_train_tokens_saved_bytes(B, L, d.width, d.layers)
        ctx.nbytes = lib.xmh_text_train_tokens_ws_bytes(B, L, d.width, d.out_dim)
        buf, ws, out = _train_buffers(d, sbytes, ctx.nbytes, B, ids.device)
        tokens = torch.empty(B, L, d.out_dim, dtype=torch.float32, device=ids.device)
        eos = torch.empty(B, dtype=torch.int32, device=ids.device)
        check(lib.xmh_text_train_forward_tokens(ctypes.byref(d), ptr(ids), ptr(kpm), B, L, ptr(out), ptr(tokens), ptr(eos), ptr(buf), sbytes, ptr(ws),
                                                ctx.nbytes, current_stream()), "xmh_text_train_forward_tokens")
        ctx.kpm = kpm
        ctx.save_for_backward(ids, eos, buf, *params)
        return out, tokens

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_eos, g_tokens):
        ids, eos, buf, *params = ctx.saved_tensors
        if g_eos is None and g_tokens is None:
            return (None, None, None, *(None for _ in params))
        B, L = ids.shape
        gp = _grad_buffers(params, ctx.needs_input_grad[3:])
        grads = tower_grads(_lib.TextGrads, TEXT, gp)
        ge, gt = _grad_or_none(g_eos), _grad_or_none(g_tokens)
        ws = _workspace(ctx.nbytes, ids.device)
        check(lib.xmh_text_backward_tokens(ctypes.byref(ctx.desc), ptr(ids), ptr(ctx.kpm), ptr(eos), B, L, ptr(buf), buf.numel() * 4, ptr(ge), ptr(gt),
                                           ctypes.byref(grads), 0, ptr(ws), ctx.nbytes, current_stream()), "xmh_text_backward_tokens")
        return (None, None, None, *gp)


def encode_image_tokens(vis, image):
    """-> (cls [B, E], tokens [B, L - 1, E]), dense"""
    params = tower_params(vis, VIT)
    if torch.is_grad_enabled() and any(p.requires_grad for p in params):
        return _VitTokensTrain.apply(vis, image, *params)
    keep = []
    d = vit_desc(vis, params, keep)
    B, L = image.shape[0], vis.positional_embedding.shape[0]
    nbytes = lib.xmh_clip_workspace_bytes(B, L, d.width, d.conv1.k, d.out_dim, ops.PREC_F32X)
    ws = _workspace(nbytes, image.device)
    y = torch.empty(B, L, d.out_dim, dtype=torch.float32, device=image.device)
    check(lib.xmh_vit_b32_forward(ctypes.byref(d), ptr(image), B, ops.PREC_F32X, None, ptr(y), ptr(ws), nbytes, current_stream()),
          "xmh_vit_b32_forward")
    return y[:, 0, :], y[:, 1:, :]


def encode_text_tokens(clip, ids, kpm):
    """-> (eos [B, E], tokens [B, L, E]); every row is computed"""
    params = tower_params(clip, TEXT)
    if torch.is_grad_enabled() and any(p.requires_grad for p in params):
        return _TextTokensTrain.apply(clip, ids, kpm, *params)
    keep = []
    d = text_desc(clip, params, keep)
    B, L = ids.shape
    nbytes = lib.xmh_clip_workspace_bytes(B, L, d.width, 0, d.out_dim, ops.PREC_F32X)
    ws = _workspace(nbytes, ids.device)
    eos = torch.empty(B, d.out_dim, dtype=torch.float32, device=ids.device)
    y = torch.empty(B, L, d.out_dim, dtype=torch.float32, device=ids.device)
    check(lib.xmh_text_forward(ctypes.byref(d), ptr(ids), ptr(kpm), B, L, ops.PREC_F32X, ptr(eos), ptr(y), None, ptr(ws), nbytes, current_stream()),
          "xmh_text_forward")
    return eos, y


def encode_image(vis, image):
    params = tower_params(vis, VIT)
    if torch.is_grad_enabled() and any(p.requires_grad for p in params):
        return _VitTrain.apply(vis, image, *params)
    keep = []
    return _vit_forward_cls(vit_desc(vis, params, keep), ops.PREC_F32X, image)


def encode_text(clip, ids, kpm):
    params = tower_params(clip, TEXT)
    if torch.is_grad_enabled() and any(p.requires_grad for p in params):
        return _TextTrain.apply(clip, ids, kpm, *params)
    keep = []
    return _text_forward_eos(text_desc(clip, params, keep), ops.PREC_F32X, ids, kpm)
