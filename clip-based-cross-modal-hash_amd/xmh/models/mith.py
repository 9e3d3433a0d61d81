"""MITH: CLIP in return_patches mode + the concept/token hash head (reference models/MITH/MITH.py:11-76,
models/MITH/hash/hash.py:9-254), registered as "MITH".  Parameters sit under the reference's key names
(``hash.gcl_i.mlp.mlps.0.0.weight`` ..., ``gcl_t`` aliasing ``gcl_i`` like in the reference, :218); the eval-path
dataflow is SURVEY 2.4.  ``res_*_cls`` / ``trans_tokens_*`` only feed the training losses; the eval path returns them as None.

Training: ``MITHHashLayer.encode_img_train`` / ``encode_txt_train`` run one modality of the head behind one
torch.autograd.Function whose forward and backward are one C call each (xmh_mith_grad.hip), exact fp32 over the parameters in place.
Which parameter is which is stated once, in the table ``MLP`` and in ``head_params`` below, in the style of clip_train.py.
``MITH.forward_train_heads`` puts them behind the frozen towers.

The training objective (reference :116-232) runs through xmh_mith_loss.hip behind ``_MITHLoss`` (a torch.autograd.Function).
Its rolling code buffer is one [train_num, K] tensor bound to the reference's four names (img_buffer_cls, txt_buffer_cls,
img_buffer_tokens, txt_buffer_tokens): that is what the reference's device branch (:169-173) leaves behind on every GPU run, because
``.to()`` of a tensor already on the device returns the tensor itself.  After a step's four row writes the batch rows therefore hold
tokens_hash_t, and all four likelihoods read the one buffer.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch
import torch.nn as nn

from .. import _lib, ops, towers
from .._lib import check, current_stream, lib, ptr
from ..common.register import registry
from . import clip as _clip
from . import clip_train as _ct
from .base import BaseModel
from .clip import Transformer
from .objective import need_cuda


class ResidualMLPs(nn.Module):
    def __init__(self, org_dim, dropout=0.0, num_layers=2, activation="gelu"):
        super().__init__()
        if activation != "gelu":
            raise NotImplementedError("MITH ships with activation: gelu")
        self.num_layers = num_layers
        self.mlps = nn.ModuleList(nn.Sequential(nn.Linear(org_dim, 4 * org_dim), nn.GELU(), nn.Dropout(p=dropout),
                                                nn.Linear(4 * org_dim, org_dim)) for _ in range(num_layers))
        self.lns = nn.ModuleList(nn.LayerNorm(org_dim) for _ in range(num_layers))

    def run(self, x):
        x = x.clone()
        for mlp, ln in zip(self.mlps, self.lns):
            h = ops.layernorm(x, ln.weight, ln.bias, ln.eps)
            f = ops.gemm_nt(h, mlp[0].weight, mlp[0].bias, act=ops.ACT_GELU_ERF)
            x = ops.gemm_nt(f, mlp[3].weight, mlp[3].bias, residual=x, out=x)
        return x


class GlobalConceptLearning(nn.Module):
    def __init__(self, k_concept, org_dim, dropout=0.0, activation="gelu", res_mlp_layers=2):
        super().__init__()
        self.mlp = ResidualMLPs(org_dim, dropout, res_mlp_layers, activation) if res_mlp_layers else nn.Identity()
        self.common_concept_embedding = nn.Linear(org_dim, k_concept, bias=False)

    def run(self, x):
        y = self.mlp.run(x) if isinstance(self.mlp, ResidualMLPs) else x
        return y, ops.gemm_nt(y, self.common_concept_embedding.weight, act=ops.ACT_TANH)


class PositionalEncoding(nn.Module):
    def __init__(self, d_model, dropout=0.0, max_len=128):
        super().__init__()
        pe = torch.zeros(max_len, d_model)
        position = torch.arange(0, max_len, dtype=torch.float).unsqueeze(1)
        div_term = torch.exp(torch.arange(0, d_model, 2).float() * (-math.log(10000.0) / d_model))
        pe[:, 0::2] = torch.sin(position * div_term)
        pe[:, 1::2] = torch.cos(position * div_term)
        self.register_buffer("pe", pe.unsqueeze(0).transpose(0, 1) / (d_model ** 0.5))       # [max_len, 1, d_model]


class BitwiseHashing(nn.Module):
    def __init__(self, org_dim, k_bits=32):
        super().__init__()
        self.k = k_bits
        self.fc_list = nn.ModuleList(nn.Linear(org_dim, 1) for _ in range(k_bits))

    def stacked(self):
        return torch.cat([fc.weight for fc in self.fc_list], 0), torch.cat([fc.bias for fc in self.fc_list], 0)


class LocalizedTokenAggregation(nn.Module):
    def __init__(self, top_k):
        super().__init__()
        self.top_k = top_k


class LocalConceptTransforming(nn.Module):
    def __init__(self, clip_embed_dim, k_bits, transformer_layers, dropout, top_k):
        super().__init__()
        self.lta = LocalizedTokenAggregation(top_k=top_k)
        self.position = PositionalEncoding(clip_embed_dim, dropout=dropout, max_len=k_bits)
        self.transformer = Transformer(width=clip_embed_dim, layers=transformer_layers, heads=clip_embed_dim // 64)
        self.hashing = BitwiseHashing(org_dim=clip_embed_dim, k_bits=k_bits)

    def run(self, tokens, scores, token_mask, addend=None):
        """tokens [B,L,D] raw CLIP tokens, scores [B,L,K] -> tokens_hash [B,K] (+ addend)."""
        m = ops.lta_aggregate(scores, tokens, token_mask, self.position.pe, self.lta.top_k)     # [B,K,D], pos-enc added
        z = self.transformer.run(m)
        w, b = self.hashing.stacked()
        return ops.bitwise_hash(z, w, b, addend)


class MITHHashLayer(nn.Module):
    def __init__(self, clip_embed_dim=512, k_bits=16, dropout=0.0, transformer_layers=2, activation="gelu", top_k_label=8,
                 res_mlp_layers=2):
        super().__init__()
        self.k_bits = k_bits
        self.dropout = float(dropout)
        self.gcl_i = self.gcl_t = GlobalConceptLearning(k_bits, clip_embed_dim, dropout, activation, res_mlp_layers)
        self.lct_i = LocalConceptTransforming(clip_embed_dim, k_bits, transformer_layers, dropout, top_k_label)
        self.lct_t = LocalConceptTransforming(clip_embed_dim, k_bits, transformer_layers, dropout, top_k_label)
        self.img_concept_proj = nn.Linear(clip_embed_dim, clip_embed_dim)
        self.txt_concept_proj = nn.Linear(clip_embed_dim, clip_embed_dim)

    def _desc(self, gcl, lct, precision: int, keep: list):
        """xmh_mith_head of one modality (its GlobalConceptLearning + LocalConceptTransforming)."""
        D = lct.hashing.fc_list[0].weight.shape[1]
        layers = list(gcl.mlp.mlps) if isinstance(gcl.mlp, ResidualMLPs) else []
        mlps = (_lib.MithMlp * max(len(layers), 1))()
        for i, (mlp, ln) in enumerate(zip(layers, gcl.mlp.lns if layers else [])):
            lw, lb = ops._f32c(ln.weight.detach()), ops._f32c(ln.bias.detach())
            keep.extend((lw, lb))
            mlps[i] = _lib.MithMlp(lw.data_ptr(), lb.data_ptr(), float(ln.eps), _clip._linear_desc(mlp[0].weight, mlp[0].bias, precision, keep),
                                   _clip._linear_desc(mlp[3].weight, mlp[3].bias, precision, keep))
        blocks = _clip._blocks_desc(list(lct.transformer.resblocks), precision, keep)
        w, b = lct.hashing.stacked()
        w, b, pe = ops._f32c(w.detach()).contiguous(), ops._f32c(b.detach()).contiguous(), ops._f32c(lct.position.pe.detach()).contiguous()
        keep.extend((mlps, blocks, w, b, pe))
        return _lib.MithHead(D, self.k_bits, lct.lta.top_k, len(layers), len(lct.transformer.resblocks), lct.transformer.heads, mlps,
                             _clip._linear_desc(gcl.common_concept_embedding.weight, None, precision, keep), pe.data_ptr(), blocks,
                             w.data_ptr(), b.data_ptr())

    def _encode_native(self, gcl, lct, cls, tokens, mask):
        """xmh_head_mith: the whole eval dataflow of one modality from one C call."""
        cls, tokens = ops._f32c(cls).contiguous(), ops._f32c(tokens).contiguous()
        B, L, D = tokens.shape
        params = list(gcl.parameters()) + list(lct.parameters()) + list(lct.buffers())
        desc, precision = _clip._cached_desc(lct, lambda prec, keep: self._desc(gcl, lct, prec, keep), params=params, slot="mith")
        m = _clip._kpm_u8(mask, tokens.device)
        nbytes = lib.xmh_head_mith_workspace_bytes(B, L, D, self.k_bits, precision)
        ws = _clip._workspace(nbytes, tokens.device)
        cls_hash = torch.empty(B, self.k_bits, dtype=torch.float32, device=tokens.device)
        tokens_hash = torch.empty_like(cls_hash)
        check(lib.xmh_head_mith(ctypes.byref(desc), ptr(cls), ptr(tokens), ptr(m), B, L, precision, ptr(cls_hash), ptr(tokens_hash), ptr(ws),
                                nbytes, current_stream()), "xmh_head_mith")
        return None, cls_hash, tokens_hash, None

    @torch.no_grad()
    def _encode(self, gcl, lct, cls, tokens_lnd, mask):
        tokens = tokens_lnd.permute(1, 0, 2)                       # LND view of a [B,L,D] buffer -> back to [B,L,D]
        if _clip.NATIVE_FORWARD and cls.dim() == 2 and tokens.dim() == 3:
            return self._encode_native(gcl, lct, cls, tokens, mask)
        _, cls_hash = gcl.run(cls)
        _, scores = gcl.run(tokens)                                # concept scores of every token, [B,L,K]
        tokens_hash = lct.run(tokens, scores, mask)
        return None, cls_hash, tokens_hash, None

    def encode_img(self, img_cls, img_tokens):
        return self._encode(self.gcl_i, self.lct_i, img_cls, img_tokens, None)

    def _encode_train(self, gcl, lct, proj, cls, tokens_lnd, mask, who):
        if self.dropout > 0:
            raise NotImplementedError("%s: dropout = %g; the training head is built for dropout 0 (configs/MITH/config.yaml), there is "
                                      "no mask replay" % (who, self.dropout))
        if not (cls.is_cuda and tokens_lnd.is_cuda):
            raise RuntimeError("%s needs CUDA/HIP tensors (got %s, %s); there is no CPU fallback" % (who, cls.device, tokens_lnd.device))
        if cls.dim() != 2 or tokens_lnd.dim() != 3 or tokens_lnd.shape[1:] != cls.shape:
            raise ValueError("%s: cls %s and tokens %s (LND) do not fit" % (who, tuple(cls.shape), tuple(tokens_lnd.shape)))
        tokens = tokens_lnd.permute(1, 0, 2)                       # LND view of a [B,L,D] buffer -> back to [B,L,D]
        params = head_params(gcl, lct, proj)
        m = _clip._kpm_u8(mask, tokens.device)
        if torch.is_grad_enabled() and (cls.requires_grad or tokens.requires_grad or any(p.requires_grad for p in params)):
            return _MITHHeadTrain.apply(gcl, lct, m, cls, tokens, *params)
        return _head_forward(gcl, lct, m, cls, tokens, params, keep_record=False)[0]

    def encode_img_train(self, img_cls, img_tokens):
        """encode_img of the reference in training mode (models/MITH/hash/hash.py:231-238) behind torch.autograd: img_cls [B, D],
        img_tokens [L, B, D] (the LND view the towers return) -> (res_img_cls [B, D], img_cls_hash [B, K], tokens_hash_i [B, K],
        trans_tokens_i [K, B, D]), fp32 CUDA tensors with a graph.  Gradients go to exactly the parameters with requires_grad (gcl_i
        is gcl_t: its .grad is autograd's sum over both modalities) and to the two inputs if they require grad.  Under no_grad, or
        with nothing to differentiate, it is the same forward and no record is kept.  B == 1 returns [1, K]: the reference's
        torch.squeeze (:84) collapses that shape to [K], which is not imitated."""
        return self._encode_train(self.gcl_i, self.lct_i, self.img_concept_proj, img_cls, img_tokens, None, "encode_img_train")

    def encode_txt_train(self, txt_eos, txt_tokens, key_padding_mask):
        """encode_txt in training mode (:240-247), as encode_img_train; key_padding_mask [B, L] (True = the token is ignored) or None"""
        return self._encode_train(self.gcl_t, self.lct_t, self.txt_concept_proj, txt_eos, txt_tokens, key_padding_mask, "encode_txt_train")

    def encode_txt(self, txt_eos, txt_tokens, key_padding_mask):
        return self._encode(self.gcl_t, self.lct_t, txt_eos, txt_tokens, key_padding_mask)


# ---- the head behind torch.autograd ------------------------------------------------------------------------------------
# (field of xmh_mith_mlp_grads in include/xmh.h, attribute path on a ResidualMLPs with the layer index), in the struct's field order
MLP = (("ln_w", "lns.%d.weight"), ("ln_b", "lns.%d.bias"), ("fc1_w", "mlps.%d.0.weight"), ("fc1_b", "mlps.%d.0.bias"),
       ("fc2_w", "mlps.%d.3.weight"), ("fc2_b", "mlps.%d.3.bias"))


def head_params(gcl, lct, proj):
    """parameter list of one modality: six per residual MLP (MLP's order), the concept embedding, twelve per transformer block
    (clip_train.BLOCK), the K hash weights [1, D], the K hash biases [1], the concept projection's weight and bias"""
    layers = gcl.mlp.num_layers if isinstance(gcl.mlp, ResidualMLPs) else 0
    mlps = [gcl.mlp.get_parameter(path % i) for i in range(layers) for _, path in MLP]
    fcs = list(lct.hashing.fc_list)
    return mlps + [gcl.common_concept_embedding.weight] + _ct.block_params(lct.transformer) + [fc.weight for fc in fcs] + [fc.bias for fc in fcs] + \
        [proj.weight, proj.bias]


def _split(params, R, layers, K):
    """head_params' list -> (mlps, concept, blocks, hash weights, hash biases, proj weight, proj bias)"""
    a, b = len(MLP) * R, len(MLP) * R + 1 + len(_ct.BLOCK) * layers
    return params[:a], params[a], params[a + 1:b], params[b:b + K], params[b + K:b + 2 * K], params[b + 2 * K], params[b + 2 * K + 1]


def _head_forward(gcl, lct, mask, cls, tokens, params, keep_record=True):
    """xmh_mith_train_forward on fp32 copies of cls [B, D] and tokens [B, L, D] -> ((res_cls, cls_hash, tokens_hash, trans_tokens),
    what backward needs or None)"""
    cls_c, tok = ops._f32c(cls.detach()).contiguous(), ops._f32c(tokens.detach()).contiguous()
    B, L, D = tok.shape
    K, tr = lct.hashing.k, lct.transformer
    R, layers = (gcl.mlp.num_layers if isinstance(gcl.mlp, ResidualMLPs) else 0), len(tr.resblocks)
    _ct._check_params(params, "MITH's training head")
    pm, concept, pb, hw, hb, proj_w, proj_b = _split(params, R, layers, K)
    lin = lambda w, b: _lib.Linear(w.data_ptr(), None, None, _clip._addr(b), w.shape[0], w.shape[1])      # noqa: E731
    mlps = (_lib.MithMlp * max(R, 1))()
    for i in range(R):
        p = dict(zip((name for name, _ in MLP), pm[len(MLP) * i:len(MLP) * (i + 1)]))
        mlps[i] = _lib.MithMlp(p["ln_w"].data_ptr(), p["ln_b"].data_ptr(), float(gcl.mlp.lns[i].eps), lin(p["fc1_w"], p["fc1_b"]), lin(p["fc2_w"], p["fc2_b"]))
    blocks = _ct._exact_blocks(pb)
    w, b = torch.cat([t.detach() for t in hw], 0), torch.cat([t.detach() for t in hb], 0)      # the K one-row layers stacked
    pe = ops._f32c(lct.position.pe.detach()).reshape(-1, D)[:K].contiguous()
    desc = _lib.MithTrain(_lib.MithHead(D, K, lct.lta.top_k, R, layers, tr.heads, mlps, lin(concept, None), pe.data_ptr(), blocks, w.data_ptr(),
                                        b.data_ptr()), lin(proj_w, proj_b))
    dev = tok.device
    nbytes = lib.xmh_mith_train_ws_bytes(B, L, D, K, R)
    sbytes = lib.xmh_mith_train_saved_bytes(B, L, D, K, R, layers) if keep_record else 0
    ws = _clip._workspace(nbytes, dev)
    buf = torch.empty(max(sbytes // 4, 1), dtype=torch.float32, device=dev) if keep_record else None
    outs = (torch.empty(B, D, dtype=torch.float32, device=dev), torch.empty(B, K, dtype=torch.float32, device=dev),
            torch.empty(B, K, dtype=torch.float32, device=dev), torch.empty(K, B, D, dtype=torch.float32, device=dev))
    check(lib.xmh_mith_train_forward(ctypes.byref(desc), ptr(cls_c), ptr(tok), ptr(mask), B, L, *(ptr(t) for t in outs), ptr(buf), sbytes, ptr(ws),
                                     nbytes, current_stream()), "xmh_mith_train_forward")
    if not keep_record:
        return outs, None
    return outs, (desc, [mlps, blocks, w, b, pe], cls_c, buf, (B, L, D, K, R, layers), nbytes)


def saved_attention(buf, geom):
    """the LTA attention A [B, K, L] inside the record xmh_mith_train_forward keeps, for tests and diagnostics.  C++ states the layout
    (kept_layout, csrc/xmh_mith_grad.hip; Python cannot include it): the block record, per residual MLP x | ln | fc_pre | fc_act,
    cls_hash, tokens_hash, A, z, p -- every piece rounded up to 256 bytes."""
    B, L, D, K, R, layers = geom
    al = lambda n: (4 * n + 255) // 256 * 256      # noqa: E731
    off = al(layers * 16 * B * K * D) + R * (2 * al(B * D) + 2 * al(4 * B * D)) + 2 * al(B * K)
    return buf[off // 4:off // 4 + B * K * L].view(B, K, L)


class _MITHHeadTrain(torch.autograd.Function):
    """forward = xmh_mith_train_forward, backward = xmh_mith_train_backward over the forward's descriptor: one modality of the head"""

    @staticmethod
    def forward(ctx, gcl, lct, mask, cls, tokens, *params):
        outs, (ctx.desc, ctx.keep, cls_c, buf, ctx.geom, ctx.nbytes) = _head_forward(gcl, lct, mask, cls, tokens, params)
        ctx.meta = ((cls.shape, cls.dtype), (tokens.shape, tokens.dtype))
        ctx.set_materialize_grads(False)                # an output the loss does not use hands backward None, not a tensor of zeros
        ctx.save_for_backward(cls_c, buf, *params)      # saved parameters: autograd notices an in-place change before backward
        return outs

    @staticmethod
    @torch.autograd.function.once_differentiable      # the gradient kernels are not themselves differentiable
    def backward(ctx, *ups):
        cls_c, buf, *params = ctx.saved_tensors         # first: this is where that in-place change raises
        B, L, D, K, R, layers = ctx.geom
        need = ctx.needs_input_grad
        pneed = need[5:]
        pm, _, pb, hw, hb, _, _ = _split(list(range(len(params))), R, layers, K)      # index ranges of the groups
        stacked = set(hw) | set(hb)
        gp = [torch.empty_like(p) if n and i not in stacked else None for i, (p, n) in enumerate(zip(params, pneed))]
        dev = cls_c.device
        d_hw = torch.empty(K, D, dtype=torch.float32, device=dev) if any(pneed[i] for i in hw) else None
        d_hb = torch.empty(K, dtype=torch.float32, device=dev) if any(pneed[i] for i in hb) else None
        d_cls = torch.empty(B, D, dtype=torch.float32, device=dev) if need[3] else None
        d_tok = torch.empty(B, L, D, dtype=torch.float32, device=dev) if need[4] else None
        mg = (_lib.MithMlpGrads * max(R, 1))()
        for i in range(R):
            mg[i] = _lib.MithMlpGrads(*[_clip._addr(gp[j]) for j in pm[len(MLP) * i:len(MLP) * (i + 1)]])
        bg = _ct.block_grads([gp[j] for j in pb])
        grads = _lib.MithGrads(mg, _clip._addr(gp[len(pm)]), bg, _clip._addr(d_hw), _clip._addr(d_hb), _clip._addr(gp[-2]), _clip._addr(gp[-1]),
                               _clip._addr(d_cls), _clip._addr(d_tok))
        gg = [None if g is None else _ct._upstream(g) for g in ups]
        ws = _clip._workspace(ctx.nbytes, dev)
        check(lib.xmh_mith_train_backward(ctypes.byref(ctx.desc), ptr(cls_c), B, L, *(ptr(g) for g in gg), ptr(buf), buf.numel() * 4,
                                          ctypes.byref(grads), 0, ptr(ws), ctx.nbytes, current_stream()), "xmh_mith_train_backward")
        for k, (i, j) in enumerate(zip(hw, hb)):          # the stacked rows back to the K one-row layers
            gp[i] = d_hw[k:k + 1] if pneed[i] else None
            gp[j] = d_hb[k:k + 1] if pneed[j] else None
        (cs, cd), (ts, td) = ctx.meta
        return (None, None, None, None if d_cls is None else d_cls.to(cd).reshape(cs), None if d_tok is None else d_tok.to(td).reshape(ts), *gp)


class _MITHLoss(torch.autograd.Function):
    """forward = xmh_mith_loss -> the ten terms as fp32 [10] (element 0 the loss), backward = xmh_mith_loss_grad (all eight inputs
    in one call).  The buffer Y is saved as it is, so an in-place write to it before backward() fails autograd's version check."""

    TEMPERATURE = 0.07                                    # info_nce_loss / info_nce_loss_bmm default (:116, :133)

    @staticmethod
    def _args(model, Y, S, xs):
        B, K = xs[2].shape
        D = xs[0].shape[1]
        N = Y.shape[0]
        a = _lib.MithLossArgs(N, B, K, D, *(t.data_ptr() for t in xs), Y.data_ptr(), S.data_ptr(),
                              *(getattr(model, n) for n, _ in MITH.HYPER), _MITHLoss.TEMPERATURE)
        ws = _clip._workspace(lib.xmh_mith_loss_ws_bytes(N, B, K, D), Y.device)
        return a, ws

    @staticmethod
    def forward(ctx, model, Y, S, *inputs):
        xs = tuple(t.detach().float().contiguous() for t in inputs)
        a, ws = _MITHLoss._args(model, Y, S, xs)
        out = torch.empty(10, dtype=torch.float64, device=Y.device)
        check(lib.xmh_mith_loss(ctypes.byref(a), ptr(ws), ws.numel(), ptr(out), current_stream()), "xmh_mith_loss")
        ctx.model = model
        ctx.meta = tuple((t.shape, t.dtype) for t in inputs)
        ctx.save_for_backward(Y, S, *xs)
        return out.float()

    @staticmethod
    @torch.autograd.function.once_differentiable      # the gradient kernel is not itself differentiable: fail loudly on double backward
    def backward(ctx, g):
        Y, S, *xs = ctx.saved_tensors
        need = ctx.needs_input_grad[3:]
        a, ws = _MITHLoss._args(ctx.model, Y, S, xs)
        up = g.detach().float().contiguous()          # only element 0 (the loss) carries a gradient
        grads = [torch.empty_like(t) if n else None for t, n in zip(xs, need)]
        gp = (ctypes.c_void_p * 8)(*(None if t is None else t.data_ptr() for t in grads))
        check(lib.xmh_mith_loss_grad(ctypes.byref(a), ptr(up), gp, 0, ptr(ws), ws.numel(), current_stream()), "xmh_mith_loss_grad")
        return (None, None, None, *(None if t is None else t.to(d).reshape(s) for t, (s, d) in zip(grads, ctx.meta)))


@registry.register_model("MITH")
class MITH(BaseModel):
    # the loss weights and their defaults (models/MITH/MITH.py:16-25); cfg values override them through from_config
    HYPER = (("hyper_tokens_intra", 1.0), ("hyper_distill", 1.0), ("hyper_info_nce", 50.0), ("hyper_cls_inter", 10.0),
             ("hyper_quan", 8.0), ("hyper_alpha", 0.01), ("hyper_lambda", 0.99))
    BUFFER_SEED = 1814

    def __init__(self, cfg, outputDim=16, clipPath="./ViT-B-32.pt", train_num=10000, hash_func="tanh", dropout=0,
                 transformer_layers=2, activation="gelu", top_k_label=8, res_mlp_layers=2, **hyper):
        super().__init__(cfg)
        embed_dim, _, self.backbone = self.load_backbone(clipPath=clipPath, return_patches=True)
        self.hash = MITHHashLayer(embed_dim, outputDim, dropout, transformer_layers, activation, top_k_label, res_mlp_layers)
        self.output_dim, self.hash_func = outputDim, hash_func
        self.hyper = hyper
        for name, default in self.HYPER:
            setattr(self, name, float(hyper.get(name, default)))
        # The rolling code buffer (:47-51): randn [train_num, K] on the host, a plain attribute, so not in state_dict.  It is drawn from
        # a private generator, as HyPProxies draws its proxies, so that constructing a model leaves the caller's random stream alone
        # (its values therefore differ from the reference's draw from the global generator).  One tensor under the four names.
        g = torch.Generator().manual_seed(self.BUFFER_SEED)
        self._bind_buffer(torch.randn(train_num, outputDim, generator=g))

    def _bind_buffer(self, t):
        self.img_buffer_cls = self.txt_buffer_cls = self.img_buffer_tokens = self.txt_buffer_tokens = t

    def encode_image(self, image):
        cls_token, seq_tokens, _ = self.backbone.encode_image(image)
        return self.hash.encode_img(img_cls=cls_token, img_tokens=seq_tokens)

    def encode_text(self, text, key_padding_mask=None):
        if key_padding_mask is not None and key_padding_mask.device != text.device:
            key_padding_mask = key_padding_mask.to(text.device)
        # every consumer of the tokens below applies new_mask (LocalizedTokenAggregation, models/MITH/hash/hash.py:142-148), so the rows
        # the mask hides need not be computed (xmh_text_forward_packed_dev; XMH_TEXT_PACKING=0 runs them)
        txt_eos, txt_tokens, _, new_mask = self.backbone.encode_text(text, key_padding_mask=key_padding_mask, masked_rows="zero")
        return self.hash.encode_txt(txt_eos, txt_tokens, new_mask)

    def forward_train(self, image, text):
        raise NotImplementedError("MITH.forward_train(image, text) has no key padding mask, which MITH's text path needs for the token "
                                  "outputs its head reads: forward_train_towers(image, text, key_padding_mask) trains MITH end to end, "
                                  "forward_train_heads its head over a frozen backbone")

    def forward_train_towers(self, image, text, key_padding_mask=None):
        """The eight tensors of ``forward``, in its order, with a graph through the hash head AND both towers: the towers
        run through encode_image_train_tokens / encode_text_train_tokens -- exact fp32, every row, one stream -- and the head through
        encode_img_train / encode_txt_train with the text tower's new_mask.  With MITHTrainer.compute_loss and build_optimizer this is
        the reference's training step (runners/MITH/runner.py:98-123)."""
        if key_padding_mask is not None and key_padding_mask.device != text.device:
            key_padding_mask = key_padding_mask.to(text.device)
        cls_token, seq_tokens = self.backbone.encode_image_train_tokens(image)
        txt_eos, txt_tokens, new_mask = self.backbone.encode_text_train_tokens(text, key_padding_mask=key_padding_mask)
        return (*self.hash.encode_img_train(cls_token, seq_tokens), *self.hash.encode_txt_train(txt_eos, txt_tokens, new_mask))

    def forward_train_heads(self, image, text, key_padding_mask=None):
        """The eight tensors of ``forward``, in its order, with a graph through the hash head only: the towers run as in
        encode_image / encode_text under no_grad (a frozen backbone), the head through encode_img_train / encode_txt_train.  With
        MITHTrainer.compute_loss and build_optimizer this trains MITH's heads."""
        if key_padding_mask is not None and key_padding_mask.device != text.device:
            key_padding_mask = key_padding_mask.to(text.device)
        with torch.no_grad():
            cls_token, seq_tokens, _ = self.backbone.encode_image(image)
            txt_eos, txt_tokens, _, new_mask = self.backbone.encode_text(text, key_padding_mask=key_padding_mask, masked_rows="zero")
        return (*self.hash.encode_img_train(cls_token, seq_tokens), *self.hash.encode_txt_train(txt_eos, txt_tokens, new_mask))

    def forward(self, image, text, key_padding_mask=None, labels=None, indexs=None, return_loss=False):
        img, txt = towers.run_both(lambda: self.encode_image(image), lambda: self.encode_text(text, key_padding_mask=key_padding_mask))
        if return_loss:                                   # reference :71-74: no label_sim is passed, so its assertion fires
            return self.object_function(*img, *txt, labels=labels, indexs=indexs)
        return (*img, *txt)

    def compute_loss(self, res_img_cls, img_cls_hash, tokens_hash_i, trans_tokens_i, res_txt_cls, txt_cls_hash, tokens_hash_t,
                     trans_tokens_t, labels=None, indexs=None, label_sim=None, **kwags):
        """reference :162-231 -- (loss, loss_dict).  `loss` is a 0-dim fp32 device tensor, differentiable with respect to the eight
        inputs; loss_dict has the reference's nested keys, its values detached 0-dim slices of the kernel's output."""
        assert label_sim is not None, "MITH must provide the label similarity"
        xs = (res_img_cls, res_txt_cls, img_cls_hash, txt_cls_hash, tokens_hash_i, tokens_hash_t, trans_tokens_i, trans_tokens_t)
        N, K = self.img_buffer_cls.shape
        B, D = img_cls_hash.shape[0], res_img_cls.shape[-1]
        if any(tuple(t.shape) != (B, D) for t in xs[:2]) or any(tuple(t.shape) != (B, K) for t in xs[2:6]) \
                or any(tuple(t.shape) != (K, B, D) for t in xs[6:]) or tuple(label_sim.shape) != (N, B):
            raise RuntimeError("MITH loss: inputs %s and label_sim %s do not fit a [%d, %d] buffer"
                               % ([tuple(t.shape) for t in xs], tuple(label_sim.shape), N, K))
        rows = self._rows(indexs, N, B)                   # host indices are checked before anything is launched
        need_cuda(*xs)
        dev = img_cls_hash.device
        if self.img_buffer_cls.device != dev:             # :170-173 -- all four names end up on the one device tensor
            self._bind_buffer(self.img_buffer_cls.to(dev, non_blocking=True))
        if label_sim.device != dev:
            label_sim = label_sim.to(dev)
        Y = self.img_buffer_cls
        Y.index_copy_(0, rows.to(dev), tokens_hash_t.detach().to(Y.dtype))   # :174-177: of the four writes, tokens_hash_t's stays
        out = _MITHLoss.apply(self, Y, label_sim.float().contiguous(), *xs)
        v = out.detach()
        loss_dict = {"All loss": v[0],
                     "LikeHood": {"intra_tokens": {"image": v[1], "text": v[2]}, "cls_inter": {"image": v[3], "text": v[4]}},
                     "Quantization": {"image": v[5], "text": v[6]},
                     "InfoNCE": {"cls": v[7], "tokens": v[8]},
                     "Distillation": v[9]}
        return out[0], loss_dict

    @staticmethod
    def _rows(indexs, N, B):
        """the batch's buffer rows as an int64 tensor (on the host unless they came on the device).  numpy arrays, lists and host
        tensors are range-checked here (IndexError, as the reference's indexing raises); rows below 0 count from the end, as in torch
        indexing.  Rows on the device are taken as they are: checking them would synchronise."""
        if indexs is None:
            raise RuntimeError("MITH loss needs `indexs`, the batch's rows in the training set")
        if isinstance(indexs, torch.Tensor) and indexs.is_cuda:
            idx = indexs.to(torch.int64).reshape(-1)
            idx = torch.where(idx < 0, idx + N, idx)
        else:
            host = np.asarray(indexs.cpu() if isinstance(indexs, torch.Tensor) else indexs).astype(np.int64).reshape(-1)
            bad = host[(host < -N) | (host >= N)]
            if bad.size:
                raise IndexError("MITH loss: index %d is out of bounds for the buffer of %d rows" % (int(bad[0]), N))
            idx = torch.from_numpy(np.where(host < 0, host + N, host))
        if idx.numel() != B:
            raise RuntimeError("MITH loss: %d indices for a batch of %d" % (idx.numel(), B))
        return idx

    def object_function(self, res_img_cls, img_cls_hash, tokens_hash_i, trans_tokens_i, res_txt_cls, txt_cls_hash, tokens_hash_t,
                        trans_tokens_t, labels=None, indexs=None, label_sim=None, **kwags):
        """reference :234-241: compute_loss with the same keywords"""
        return self.compute_loss(res_img_cls=res_img_cls, img_cls_hash=img_cls_hash, tokens_hash_i=tokens_hash_i,
                                 trans_tokens_i=trans_tokens_i, res_txt_cls=res_txt_cls, txt_cls_hash=txt_cls_hash,
                                 tokens_hash_t=tokens_hash_t, trans_tokens_t=trans_tokens_t, labels=labels, indexs=indexs,
                                 label_sim=label_sim, **kwags)

    @classmethod
    def from_config(cls, cfg, output_dim=16, train_num=10000):
        keys = ("hyper_tokens_intra", "hyper_distill", "hyper_info_nce", "hyper_cls_inter", "hyper_quan", "hyper_alpha", "hyper_lambda")
        return cls(cfg=cfg, outputDim=output_dim, clipPath=cfg.get("clip_path", "./ViT-B-32.pt"), train_num=train_num,
                   hash_func=cfg.get("hash_func", "tanh"), dropout=cfg.get("dropout", 0), transformer_layers=cfg.get("transformer_layers", 2),
                   activation=cfg.get("activation", "gelu"), top_k_label=cfg.get("top_k_label", 8), res_mlp_layers=cfg.get("res_mlp_layers", 2),
                   **{k: cfg.get(k) for k in keys if cfg.get(k) is not None})
