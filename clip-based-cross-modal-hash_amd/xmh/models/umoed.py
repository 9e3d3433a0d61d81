"""UMoED (reference models/UMoED): a transformer decoder over the towers' token rows as the hash head, its second feed-forward
product a Soft-MoE, and the pairwise set objective -- through xmh_umoed.hip.

``UMoEDTokenHash`` / ``UMoEDHashLayer`` carry the reference's state-dict names (hash/hash_moe.py TokenHash, HashLayer), so a reference
checkpoint loads strictly; one C call per modality and batch (xmh_head_umoed) runs the head in inference.  ``forward`` / ``encode_img`` /
``encode_txt`` stay inference only and raise in train mode or with a graph asked for; the train-mode head with its six dropout sites per
layer and its backward (xmh_head_umoed_train_forward / xmh_head_umoed_backward) is ``forward_train`` / ``encode_img_train`` /
``encode_txt_train``, one autograd.Function.  ``UMoEDObjective`` is the reference's ``similarity_loss`` in the one
family its configuration uses (``distance.mode: pairwise``, ``distance_mode: cosine``, ``triplet: True``): one forward and one backward
call (xmh_umoed_loss / xmh_umoed_loss_grad) behind one autograd.Function.  ``UMoED`` (registered as "UMoED") puts both behind the CLIP
towers' token outputs.

Departures from the reference: tokens are always taken as [B, T, E] (it decides whether to permute by comparing a dimension with the
token count and goes wrong at B = 50 and B = 32); ``MoE: True`` with ``hidden_dim != embed_dim`` is refused (it builds the decoder
at the embedding width and the learned rows at ``hidden_dim``, and fails in its first forward)."""
import ctypes as C
import math

import torch
import torch.nn as nn

from .. import _lib, ops, towers
from .. import retrieval as R
from .._lib import check, current_stream, lib, ptr, workspace
from ..common.register import registry
from .base import BaseModel
from .heads import _DRAW, _param
from .objective import Objective, Spec, need_cuda

HASH_FUNCS = ("linear_subspace", "tanh", "softmax")          # XMH_UMOED_LINEAR_SUBSPACE, XMH_UMOED_TANH, XMH_UMOED_SOFTMAX
MERGE_FUNCS = ("concatenate", "mean")                        # XMH_UMOED_CONCATENATE, XMH_UMOED_MEAN
ROUTES = (("linear_subspace", "concatenate"), ("tanh", "mean"), ("softmax", "mean"))
TERMS = ("loss", "T_i2t", "T_t2i", "U_img", "U_txt")


# ---- the objective (reference UMoED.py similarity_loss) ---------------------------------------------------------------------------------
def _pack(consts, aux, ts):
    e1, e2 = ts
    B, M, V = e1.shape
    cst, C_ = consts
    return (B, M, V, C_), (ptr(e1), ptr(e2), B, M, V, C_, ptr(aux[0]), C.byref(cst))


# forward = xmh_umoed_loss -> fp32 [5], backward = xmh_umoed_loss_grad (both gradients, one call; only element 0 carries one)
_UMOED = Spec(lib.xmh_umoed_loss, lib.xmh_umoed_loss_grad, _pack, lib.xmh_umoed_loss_ws_bytes,
              "UMoED objective: B=%d M=%d V=%d C=%d outside B <= 512, M <= 128, V <= 256, C <= 127", out_len=8, terms=5)


class UMoEDObjective(nn.Module):
    """the constants of the reference's UMoED.__init__ (``distance``, ``chamfer`` and ``hash_pars`` blocks, its defaults) and its
    similarity_loss.  No parameters.  Only the pairwise / cosine / triplet family is built; anything else raises, naming the key."""

    def __init__(self, mode="chamfer", distance_mode="cosine", triplet=True, extreme=False, extreme_T=0.01, token_triplet_margin=0.2,
                 triplet_alpha=1.0, unif_alpha=0.01):
        super().__init__()
        if "pairwise" not in str(mode):
            raise NotImplementedError("UMoED objective: distance.mode %r (only 'pairwise' is built)" % (mode,))
        if distance_mode != "cosine":
            raise NotImplementedError("UMoED objective: distance_mode %r (only 'cosine' is built)" % (distance_mode,))
        if not triplet:
            raise NotImplementedError("UMoED objective: triplet %r (only the triplet form is built, not the bayesian one)" % (triplet,))
        self.mode, self.distance_mode, self.triplet = mode, distance_mode, True
        self.consts = _lib.UmoedConsts(int(bool(extreme)), float(extreme_T), float(token_triplet_margin), float(triplet_alpha), float(unif_alpha))

    @classmethod
    def from_config(cls, cfg, extreme=None, extreme_T=None, triplet=None, distance_mode=None):
        """the model block of a configuration (a mapping with ``get``): nested blocks and defaults as the reference reads them
        (its from_config's ``extreme: True``, ``extreme_T: 0.01``); the keyword arguments override, as its constructor's do"""
        d, c, h = (cfg.get(k, None) or {} for k in ("distance", "chamfer", "hash_pars"))
        return cls(mode=d.get("mode", "chamfer"),
                   distance_mode=cfg.get("distance_mode", "cosine") if distance_mode is None else distance_mode,
                   triplet=cfg.get("triplet", True) if triplet is None else triplet,
                   extreme=cfg.get("extreme", True) if extreme is None else extreme,
                   extreme_T=cfg.get("extreme_T", 0.01) if extreme_T is None else extreme_T,
                   token_triplet_margin=c.get("token_triplet_margin", 0.2), triplet_alpha=h.get("triplet_alpha", 1),
                   unif_alpha=c.get("unif_alpha", 0.01))

    def terms(self, img_embeds, txt_embeds, labels):
        """-> fp32 [5] on the device (TERMS); element 0 carries the gradient"""
        need_cuda(img_embeds, txt_embeds)
        labels = torch.as_tensor(labels)
        B = img_embeds.shape[0]
        if img_embeds.dim() != 3 or txt_embeds.shape != img_embeds.shape or labels.dim() != 2 or labels.shape[0] != B:
            raise RuntimeError("UMoED objective: embeddings %s / %s, labels %s do not fit together"
                               % (tuple(img_embeds.shape), tuple(txt_embeds.shape), tuple(labels.shape)))
        lab = R.pack_labels((labels == 1).to(torch.uint8).to(img_embeds.device))
        return Objective.apply(_UMOED, (self.consts, labels.shape[1]), (lab,), img_embeds, txt_embeds)

    def forward(self, img_embeds, txt_embeds, labels=None):
        """-> (loss, loss_dict) with the reference's nested names; without labels every sample is its own class (object_function)"""
        if labels is None:
            labels = torch.ones([img_embeds.shape[0]], dtype=torch.int).diag()
        out = self.terms(img_embeds, txt_embeds, labels)
        v = out.detach()
        ta, ua = self.consts.triplet_alpha, self.consts.unif_alpha
        return out[0], {"All loss": v[0],
                        "Tokens": {"Similarity": {"i2t": v[1], "t2i": v[2], "it2i": 0, "it2t": 0, "All": (v[1] + v[2]) / 4 * ta},
                                   "Diversity": {"i": v[3], "t": v[4], "it": 0, "All": (v[3] + v[4]) / 3 * ua}}}


# ---- the head (reference hash/hash_moe.py, hash/block/) --------------------------------------------------------------------------------
class _Experts(nn.Module):
    """MultiExpertLayer: weight [n, F, d] ("in, out"), bias [n, d]"""

    def __init__(self, in_features, out_features, num_experts):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(num_experts, in_features, out_features))
        self.bias = nn.Parameter(torch.empty(num_experts, out_features))


class _SoftMoE(nn.Module):
    """SoftMoE: phi [F, n, p] and the experts"""

    def __init__(self, in_features, out_features, num_experts, slots_per_expert):
        super().__init__()
        self.phi = nn.Parameter(torch.empty(in_features, num_experts, slots_per_expert))
        self.experts = _Experts(in_features, out_features, num_experts)


class _SoftMoEDecoderLayer(nn.Module):
    """SoftMoEDecoderLayer's parameters under its names, in its order; the torch modules only hold them"""

    def __init__(self, d_model, nhead, num_experts, slots_per_expert, dim_feedforward, dropout):
        super().__init__()
        self.dropout = nn.Dropout(dropout)
        self.norm1 = nn.LayerNorm(d_model)
        self.self_attn = nn.MultiheadAttention(d_model, nhead, dropout=dropout, batch_first=True)
        self.norm2 = nn.LayerNorm(d_model)
        self.multihead_attn = nn.MultiheadAttention(d_model, nhead, dropout=dropout, batch_first=True)
        self.norm3 = nn.LayerNorm(d_model)
        self.linear = nn.Linear(d_model, dim_feedforward)
        self.moe = _SoftMoE(dim_feedforward, d_model, num_experts, slots_per_expert)


class _Decoder(nn.Module):
    def __init__(self, layers):
        super().__init__()
        self.layers = nn.ModuleList(layers)


def _uniform(t, bound, g):
    with torch.no_grad():
        t.uniform_(-bound, bound, generator=g)


def _init_linear(fc, g):
    """nn.Linear.reset_parameters: kaiming_uniform(a = sqrt 5), i.e. U(+-1 / sqrt fan_in), for the weight and the bias"""
    bound = 1.0 / math.sqrt(fc.weight.shape[1])
    _uniform(fc.weight, bound, g)
    _uniform(fc.bias, bound, g)


def _init_mha(m, g):
    """nn.MultiheadAttention._reset_parameters: xavier_uniform in_proj, zero biases; out_proj.weight keeps nn.Linear's law"""
    nn.init.xavier_uniform_(m.in_proj_weight, generator=g)
    nn.init.constant_(m.in_proj_bias, 0.0)
    _uniform(m.out_proj.weight, 1.0 / math.sqrt(m.out_proj.weight.shape[1]), g)
    nn.init.constant_(m.out_proj.bias, 0.0)


class _UMoEDHeadTrain(torch.autograd.Function):
    """forward = xmh_head_umoed_train_forward, backward = xmh_head_umoed_backward: one modality; only ``embeds`` carries a gradient"""

    @staticmethod
    def forward(ctx, mod, tokens, keep, *params):
        embeds, code, x, saved = mod._run_train(tokens, keep)
        ctx.mod, ctx.p, ctx.meta = mod, float(mod.dropout_p), (tokens.shape, tokens.dtype)
        ctx.mark_non_differentiable(code)
        ctx.save_for_backward(x, saved, keep, *params)   # saved parameters: autograd notices an in-place change before backward
        return embeds, code

    @staticmethod
    @torch.autograd.function.once_differentiable      # the gradient kernels are not themselves differentiable
    def backward(ctx, g_embeds, g_code):
        x, saved, keep, *params = ctx.saved_tensors
        mod, need = ctx.mod, ctx.needs_input_grad
        B, T = x.shape[0], x.shape[1]
        gx = torch.empty_like(x) if need[1] else None
        gp = [torch.empty_like(_param(q)) if n else None for q, n in zip(params, need[3:])]
        at = lambda t: None if t is None else t.data_ptr()                                   # noqa: E731
        head, alive = mod._desc()
        n = len(_lib.UmoedLayerGrads.NAMES)
        layers = (_lib.UmoedLayerGrads * head.n_layers)(*[_lib.UmoedLayerGrads(*[at(t) for t in gp[1 + n * i:1 + n * (i + 1)]])
                                                         for i in range(head.n_layers)])
        grads = _lib.UmoedHeadGrads(layers, at(gp[0]), at(gp[-2]), at(gp[-1]), at(gx))
        up = g_embeds.detach().float().contiguous()
        wsb = C.c_size_t(0)
        lib.xmh_head_umoed_train_bytes(B, T, C.byref(head), C.byref(wsb))
        ws = workspace(wsb.value, x.device)
        check(lib.xmh_head_umoed_backward(C.byref(head), ptr(x), ptr(keep), ctx.p, ptr(up), B, T, ptr(saved), saved.numel(),
                                          C.byref(grads), 0, ptr(ws), ws.numel(), current_stream()), "xmh_head_umoed_backward")
        del alive
        if gx is not None:
            gx = gx.reshape(ctx.meta[0]).to(ctx.meta[1])
        return (None, gx, None, *gp)


class UMoEDTokenHash(nn.Module):
    """reference TokenHash: ``decoder_learned_parameters`` [M, d], ``decoder.layers.{i}`` (a Soft-MoE decoder at the embedding width
    with ``MoE``, else nn.TransformerDecoder's layers at ``hidden_dim`` behind ``first_layer``), ``classifier`` Linear(d, V).
    Initial weights follow the reference's init laws from a private generator seeded with ``seed``; as there (deepcopy of one layer)
    every layer starts from the same values."""

    def __init__(self, outputDim=2, embedDim=512, setDim=64, dropout=0.3, decoder_heads=8, decoder_layers=6, hash_func="linear_subspace",
                 merge_func="concatenate", num_experts=8, slots_per_expert=8, MoE=False, hidden_dim=512, dim_feedforward=2048, seed=0):
        super().__init__()
        if (hash_func, merge_func) not in ROUTES:
            raise NotImplementedError("UMoED head: hash_func %r with merge_func %r (built: %s)"
                                      % (hash_func, merge_func, ", ".join("%s + %s" % r for r in ROUTES)))
        if hidden_dim is None or isinstance(hidden_dim, str):
            hidden_dim = embedDim
        if MoE and hidden_dim != embedDim:
            raise NotImplementedError("UMoED head: MoE: True with hidden_dim %d != embed_dim %d: the reference builds the Soft-MoE decoder at "
                                      "the embedding width and the learned rows at hidden_dim, and fails in its first forward" % (hidden_dim, embedDim))
        self.hash_func, self.merge_func, self.MoE = hash_func, merge_func, bool(MoE)
        self.dropout_p = float(dropout)
        self.generator = None                 # torch.Generator of the module's device for the dropout masks; None: the global one
        self.heads, self.num_experts, self.slots_per_expert = decoder_heads, num_experts, slots_per_expert
        if MoE:
            self.decoder = _Decoder([_SoftMoEDecoderLayer(embedDim, decoder_heads, num_experts, slots_per_expert, dim_feedforward, dropout)
                                     for _ in range(decoder_layers)])
        else:
            self.decoder = _Decoder([nn.TransformerDecoderLayer(d_model=hidden_dim, nhead=decoder_heads, dim_feedforward=dim_feedforward,
                                                                dropout=dropout, batch_first=True) for _ in range(decoder_layers)])
        self.first_layer = nn.Linear(embedDim, hidden_dim) if hidden_dim != embedDim else None
        self.decoder_learned_parameters = nn.Parameter(torch.randn(setDim, hidden_dim))
        self.classifier = nn.Linear(hidden_dim, outputDim)
        g = torch.Generator().manual_seed(int(seed))
        first = self.decoder.layers[0]
        for m in (first.self_attn, first.multihead_attn):
            _init_mha(m, g)
        if MoE:
            _init_linear(first.linear, g)
            _uniform(first.moe.phi, 1.0 / math.sqrt(num_experts * slots_per_expert), g)      # kaiming_uniform(a = sqrt 5) over dim 1 x the rest
            bound = 1.0 / math.sqrt(dim_feedforward * embedDim)
            _uniform(first.moe.experts.weight, bound, g)
            _uniform(first.moe.experts.bias, bound, g)
        else:
            _init_linear(first.linear1, g)
            _init_linear(first.linear2, g)
        for layer in self.decoder.layers[1:]:
            layer.load_state_dict(first.state_dict())
        if self.first_layer is not None:
            _init_linear(self.first_layer, g)
        with torch.no_grad():
            self.decoder_learned_parameters.normal_(generator=g)
        _init_linear(self.classifier, g)

    @property
    def code_width(self):
        M, V = self.decoder_learned_parameters.shape[0], self.classifier.weight.shape[0]
        return M * int(math.log2(V)) if self.hash_func == "linear_subspace" else V

    def _desc(self):
        """-> (xmh_umoed_head, what must stay alive while it is used)"""
        layers = (_lib.UmoedLayer * len(self.decoder.layers))()
        for dst, y in zip(layers, self.decoder.layers):
            t = {"ln1_g": y.norm1.weight, "ln1_b": y.norm1.bias, "sa_in_w": y.self_attn.in_proj_weight, "sa_in_b": y.self_attn.in_proj_bias,
                 "sa_out_w": y.self_attn.out_proj.weight, "sa_out_b": y.self_attn.out_proj.bias, "ln2_g": y.norm2.weight, "ln2_b": y.norm2.bias,
                 "ca_in_w": y.multihead_attn.in_proj_weight, "ca_in_b": y.multihead_attn.in_proj_bias,
                 "ca_out_w": y.multihead_attn.out_proj.weight, "ca_out_b": y.multihead_attn.out_proj.bias, "ln3_g": y.norm3.weight,
                 "ln3_b": y.norm3.bias}
            if self.MoE:
                t.update(lin_w=y.linear.weight, lin_b=y.linear.bias, phi=y.moe.phi, exp_w=y.moe.experts.weight, exp_b=y.moe.experts.bias)
            else:
                t.update(lin_w=y.linear1.weight, lin_b=y.linear1.bias, lin2_w=y.linear2.weight, lin2_b=y.linear2.bias)
            for k, p in t.items():
                setattr(dst, k, _param(p).data_ptr())
        first = self.first_layer
        y0 = self.decoder.layers[0]
        M, d = self.decoder_learned_parameters.shape
        V = self.classifier.weight.shape[0]
        F = (y0.linear if self.MoE else y0.linear1).weight.shape[0]
        E = first.weight.shape[1] if first is not None else d
        head = _lib.UmoedHead(layers, len(self.decoder.layers),
                              _param(first.weight).data_ptr() if first is not None else None, _param(first.bias).data_ptr() if first is not None else None,
                              _param(self.decoder_learned_parameters).data_ptr(), _param(self.classifier.weight).data_ptr(),
                              _param(self.classifier.bias).data_ptr(), E, d, self.heads, F, M, V,
                              self.num_experts if self.MoE else 0, self.slots_per_expert if self.MoE else 0, int(self.MoE),
                              HASH_FUNCS.index(self.hash_func), MERGE_FUNCS.index(self.merge_func), float(y0.norm1.eps))
        return head, layers

    def forward(self, tokens):
        """tokens [B, T, E] -> (embeds [B, M, V], code [B, M log2 V] or [B, V]); inference only"""
        if self.training or (torch.is_grad_enabled() and (tokens.requires_grad or any(p.requires_grad for p in self.parameters()))):
            raise NotImplementedError("UMoED head: the backward of the decoder head is not built behind forward(); run it in eval mode under "
                                      "torch.no_grad(), or train through forward_train (encode_img_train / encode_txt_train)")
        head, keep = self._desc()
        if tokens.dim() != 3 or tokens.shape[2] != head.E:
            raise ValueError("a UMoED head takes [B, T, %d] tokens, got %s" % (head.E, tuple(tokens.shape)))
        x = ops._f32c(tokens.detach()).contiguous()
        B, T = x.shape[0], x.shape[1]
        nbytes = lib.xmh_head_umoed_bytes(B, T, C.byref(head))
        ws = workspace(nbytes, x.device)              # 0 outside the bounds: the call below then says which one
        embeds = torch.empty(B, head.M, head.V, dtype=torch.float32, device=x.device)
        code = torch.empty(B, self.code_width, dtype=torch.float32, device=x.device)
        check(lib.xmh_head_umoed(C.byref(head), ptr(x), B, T, ptr(embeds), ptr(code), ptr(ws), nbytes, current_stream()), "xmh_head_umoed")
        del keep
        return embeds, code

    # ---- train mode ------------------------------------------------------------------------------------------------------
    def head_params(self):
        """the parameters in the order of xmh_umoed_head_grads: the learned rows, each layer's nineteen (UmoedLayerGrads.NAMES), the
        classifier's weight and bias"""
        out = [self.decoder_learned_parameters]
        for y in self.decoder.layers:
            out += [y.norm1.weight, y.norm1.bias, y.self_attn.in_proj_weight, y.self_attn.in_proj_bias, y.self_attn.out_proj.weight,
                    y.self_attn.out_proj.bias, y.norm2.weight, y.norm2.bias, y.multihead_attn.in_proj_weight, y.multihead_attn.in_proj_bias,
                    y.multihead_attn.out_proj.weight, y.multihead_attn.out_proj.bias, y.norm3.weight, y.norm3.bias, y.linear.weight,
                    y.linear.bias, y.moe.phi, y.moe.experts.weight, y.moe.experts.bias]
        return out + [self.classifier.weight, self.classifier.bias]

    def _check_trainable(self):
        if not self.MoE:
            raise NotImplementedError("UMoED head: MoE: False (the plain decoder) has no train mode; only the Soft-MoE decoder does")
        if self.first_layer is not None:
            raise NotImplementedError("UMoED head: a first_layer (hidden_dim != embed_dim) has no train mode")

    def keep_sections(self, B: int, T: int):
        """the element counts of the six keep-mask sections of one layer, in the library's order (drop1 .. drop6)"""
        M, d = self.decoder_learned_parameters.shape
        F = self.decoder.layers[0].linear.weight.shape[0]
        return [B * self.heads * M * M, B * M * d, B * self.heads * M * T, B * M * d, B * M * F, B * M * d]

    def draw_keep_mask(self, B: int, T: int, device):
        """the keep bytes of one train-mode forward, uint8 [layers x sum(keep_sections)] on the device, or None when p == 0.  Drawn by
        torch from ``self.generator`` as a byte Bernoulli(1 - p): the library draws no random numbers"""
        self._check_trainable()
        p = self.dropout_p
        if p <= 0.0:
            return None
        if p >= 1.0:
            raise ValueError("dropout p = %g: nothing would be kept" % p)
        n = sum(self.keep_sections(B, T)) * len(self.decoder.layers)
        return torch.empty(n, dtype=torch.uint8, device=device).bernoulli_(1.0 - p, generator=self.generator)

    def _run_train(self, tokens, keep):
        """one train-mode forward call -> (embeds, code, the tokens as the kernels read them, the record the call filled)"""
        self._check_trainable()
        head, alive = self._desc()
        if tokens.dim() != 3 or tokens.shape[2] != head.E:
            raise ValueError("a UMoED head takes [B, T, %d] tokens, got %s" % (head.E, tuple(tokens.shape)))
        if not tokens.is_cuda:
            raise RuntimeError("UMoED head in train mode needs CUDA/HIP tensors (got %s); there is no CPU fallback" % (tokens.device,))
        x = ops._f32c(tokens.detach()).contiguous()
        B, T = x.shape[0], x.shape[1]
        want = lib.xmh_umoed_keep_bytes(B, T, C.byref(head))          # 0 outside the bounds: the call below then says which one
        if keep is not None and want and (keep.dtype != torch.uint8 or keep.numel() != want):
            raise ValueError("UMoED head: a keep mask of %d %s where B=%d T=%d take %d bytes (six sections per layer, keep_sections)"
                             % (keep.numel(), keep.dtype, B, T, want))
        wsb = C.c_size_t(0)
        nbytes = lib.xmh_head_umoed_train_bytes(B, T, C.byref(head), C.byref(wsb))
        saved, ws = workspace(nbytes, x.device), workspace(wsb.value, x.device)     # 0 outside the bounds: the call below then says which one
        embeds = torch.empty(B, head.M, head.V, dtype=torch.float32, device=x.device)
        code = torch.empty(B, self.code_width, dtype=torch.float32, device=x.device)
        check(lib.xmh_head_umoed_train_forward(C.byref(head), ptr(x), ptr(keep), self.dropout_p, B, T, ptr(embeds), ptr(code), ptr(saved), nbytes,
                                               ptr(ws), wsb.value, current_stream()), "xmh_head_umoed_train_forward")
        del alive
        return embeds, code, x, saved

    def forward_train(self, tokens, keep=_DRAW):
        """tokens [B, T, E] -> (embeds [B, M, V], code), the train-mode head whatever ``self.training`` says, behind torch.autograd when
        anything requires grad.  `keep` overrides the drawn mask (uint8, draw_keep_mask's layout, or None for no dropout) -- tests replay
        stored masks.  The code carries no gradient."""
        if keep is _DRAW:
            keep = self.draw_keep_mask(tokens.shape[0], tokens.shape[1], tokens.device)
        elif keep is not None:
            keep = keep.to(device=tokens.device, dtype=torch.uint8).contiguous().reshape(-1)
        params = self.head_params()
        if torch.is_grad_enabled() and (tokens.requires_grad or any(q.requires_grad for q in params)):
            self._check_trainable()
            return _UMoEDHeadTrain.apply(self, tokens, keep, *params)
        return self._run_train(tokens, keep)[:2]


class UMoEDHashLayer(nn.Module):
    """reference HashLayer under its attribute names: ``hash_module`` with ``fusion``, else ``img_token_hash`` / ``txt_token_hash``"""

    def __init__(self, visual_tokens=48, txt_tokens=32, img_feature_size=512, txt_feature_size=512, outputDim=64, setDim=64, dropout=0.3,
                 decoder_heads=8, decoder_layers=6, num_experts=8, expert_layers=3, slots_per_expert=8, MoE=False, fusion=True, hidden_dim=512,
                 hash_func_="tanh", merge_func_="mean", dim_feedforward=2048, seed=0):
        super().__init__()
        if hash_func_ not in HASH_FUNCS:
            raise ValueError(f"Unsupported hash func for {hash_func_}")
        if merge_func_ not in MERGE_FUNCS:
            raise ValueError(f"Unsupported merge func for {merge_func_}")
        self.hash_func_, self.fusion = hash_func_, bool(fusion)
        kw = dict(outputDim=outputDim, embedDim=img_feature_size, setDim=setDim, dropout=dropout, decoder_heads=decoder_heads,
                  decoder_layers=decoder_layers, hash_func=hash_func_, merge_func=merge_func_, num_experts=num_experts,
                  slots_per_expert=slots_per_expert, MoE=MoE, hidden_dim=hidden_dim, dim_feedforward=dim_feedforward)
        if self.fusion:
            self.hash_module = UMoEDTokenHash(seed=seed, **kw)
        else:
            self.img_token_hash = UMoEDTokenHash(seed=seed, **kw)
            self.txt_token_hash = UMoEDTokenHash(seed=seed + 1, **kw)

    def encode_img(self, token_embeds):
        return (self.hash_module if self.fusion else self.img_token_hash)(token_embeds)

    def encode_txt(self, token_embeds):
        # without fusion the reference's encode_txt still runs img_token_hash (hash_moe.py:130-138; txt_token_hash is never used): kept
        return (self.hash_module if self.fusion else self.img_token_hash)(token_embeds)

    def encode_img_train(self, token_embeds, keep=_DRAW):
        """the train-mode head (dropout, a graph when anything requires grad); `keep` replays a stored mask"""
        return (self.hash_module if self.fusion else self.img_token_hash).forward_train(token_embeds, keep)

    def encode_txt_train(self, token_embeds, keep=_DRAW):
        # img_token_hash without fusion, as encode_txt: txt_token_hash never receives a gradient (reference hash_moe.py:130-138)
        return (self.hash_module if self.fusion else self.img_token_hash).forward_train(token_embeds, keep)

    def encode_imgAndtxt(self, img_embeds, txt_embeds):
        """the tokens of both modalities stacked along T through ``hash_module`` (only there with fusion, as in the reference)"""
        return self.hash_module(torch.cat([img_embeds, txt_embeds], dim=1))

    def quantization(self, code):
        if self.hash_func_ == "tanh":
            return torch.tanh(code)
        if self.hash_func_ == "softmax":
            return torch.softmax(code.reshape(code.shape[0], -1, 2), dim=-1).reshape(code.shape[0], -1)
        return linear_subspace_code(code)

    def forward(self, img_inp_embeds, txt_inp_embeds):
        return (*self.encode_img(img_inp_embeds), *self.encode_txt(txt_inp_embeds), None, None)


def linear_subspace_code(logits):
    """[B, M, V] -> [B, M log2 V]: the argmax of each row as log2 V bits, most significant first, 1 -> +1 and 0 -> -1 (torch ops: the
    quantization helper outside the hot path; the head's kernel writes the same code)"""
    B, M, V = logits.shape
    bits = int(math.log2(V))
    idx = torch.argmax(logits, dim=-1)
    shifts = torch.arange(bits - 1, -1, -1, device=logits.device)
    return (((idx.unsqueeze(-1) >> shifts) & 1).to(torch.float32) * 2 - 1).reshape(B, M * bits)


@registry.register_model("UMoED")
class UMoED(BaseModel):
    """reference models/UMoED/UMoED.py: CLIP in return_patches mode, the decoder head over every token row of a tower (the image side
    with the cls row first), and the pairwise objective over the two [B, M, V] logit tensors."""

    def __init__(self, cfg, outputDim=16, clipPath="./ViT-B-32.pt", triplet_margin=0.1, train_num=10000, txt_token_size=32, setDim=64,
                 dropout=0.3, hash_func="softmax", merge_func="mean", cls_alpha=0.7, decoder_heads=8, decoder_layers=6, extreme=False,
                 extreme_T=0.01, triplet=True, distance_mode="cosine", num_experts=8, expert_layers=3, slots_per_expert=8, MoE=False, fusion=True,
                 hidden_dim=512, dim_feedforward=2048, seed=0, **kwags):
        super().__init__(cfg)
        self.hash_func = hash_func
        embed_dim, visual_token_size, self.backbone = self.load_backbone(clipPath=clipPath, return_patches=True)
        self.visual_token_size, self.txt_token_size, self.cls_alpha = visual_token_size, txt_token_size, cls_alpha
        assert outputDim % setDim == 0, f"'outputDim={outputDim}' must be the integer times of 'setDim={setDim}'"
        vocab_size = 2 ** (outputDim // setDim)
        self.hash = UMoEDHashLayer(visual_tokens=visual_token_size, txt_tokens=txt_token_size, outputDim=vocab_size, img_feature_size=embed_dim,
                                   txt_feature_size=embed_dim, setDim=setDim, dropout=dropout, decoder_heads=decoder_heads,
                                   decoder_layers=decoder_layers, hash_func_=hash_func, merge_func_=merge_func, num_experts=num_experts,
                                   expert_layers=expert_layers, slots_per_expert=slots_per_expert, MoE=MoE, hidden_dim=hidden_dim, fusion=fusion,
                                   dim_feedforward=dim_feedforward, seed=seed)
        self.output_dim = outputDim
        self.extreme, self.extreme_T, self.distance_mode = extreme, extreme_T, distance_mode
        # a checkpoint of any objective family still loads, encodes and evaluates: what is not built is said when the objective is asked for
        try:
            self.objective, self._objective_error = UMoEDObjective.from_config(cfg if cfg is not None else {}, extreme=extreme, extreme_T=extreme_T,
                                                                               triplet=triplet, distance_mode=distance_mode), None
        except NotImplementedError as e:
            self.objective, self._objective_error = None, e

    @staticmethod
    def _image_tokens(cls_token, seq_tokens):
        """cls [B, E] and the patch rows [L - 1, B, E] (the towers' LND view) -> [B, L, E], the cls row on top of the patch rows"""
        return torch.cat([cls_token.unsqueeze(1), seq_tokens.permute(1, 0, 2)], dim=1)

    def get_features(self, image, text):
        """-> (image tokens [B, L, E], text tokens [B, T, E]); every text row is used, padded ones too (masked_rows="exact")"""
        def img():
            cls_token, seq_tokens, _ = self.backbone.encode_image(image)
            return self._image_tokens(cls_token, seq_tokens)

        def txt():
            _, tokens, _, _ = self.backbone.encode_text(text, masked_rows="exact")
            return tokens.permute(1, 0, 2)
        return towers.run_both(img, txt)

    def encode_image(self, image):
        cls_token, seq_tokens, _ = self.backbone.encode_image(image)
        return self.hash.encode_img(self._image_tokens(cls_token, seq_tokens))

    def encode_text(self, text):
        _, tokens, _, _ = self.backbone.encode_text(text, masked_rows="exact")
        return self.hash.encode_txt(tokens.permute(1, 0, 2))

    def encoder_fusion(self, image, text):
        img_tokens, txt_tokens = self.get_features(image, text)
        return self.hash.encode_imgAndtxt(img_embeds=img_tokens, txt_embeds=txt_tokens)

    def forward(self, image, text, labels=None, indexs=None, return_loss=False):
        """-> (img_embeds, img_hash, txt_embeds, txt_hash, None, None): the reference leaves the fusion pair out of its forward"""
        img_tokens, txt_tokens = self.get_features(image, text)
        img_embeds, img_hash = self.hash.encode_img(img_tokens)
        txt_embeds, txt_hash = self.hash.encode_txt(txt_tokens)
        if return_loss:
            return self.object_function(img_embeds=img_embeds, img_hash=img_hash, txt_embeds=txt_embeds, txt_hash=txt_hash, fusion_embeds=None,
                                        fusion_hash=None, labels=labels, indexs=indexs)
        return img_embeds, img_hash, txt_embeds, txt_hash, None, None

    def forward_train(self, image, text):
        """the six outputs of ``forward`` with a graph through the head AND both towers (encode_*_train_tokens)"""
        cls_token, seq_tokens = self.backbone.encode_image_train_tokens(image)
        _, txt_tokens, _ = self.backbone.encode_text_train_tokens(text)
        return (*self.hash.encode_img_train(self._image_tokens(cls_token, seq_tokens)), *self.hash.encode_txt_train(txt_tokens.permute(1, 0, 2)),
                None, None)

    def forward_train_heads(self, image, text):
        """the same six with a graph through the head only: the towers run as in ``forward`` under no_grad (a frozen backbone)"""
        with torch.no_grad():
            img_tokens, txt_tokens = self.get_features(image, text)
        return (*self.hash.encode_img_train(img_tokens), *self.hash.encode_txt_train(txt_tokens), None, None)

    def similarity_loss(self, img_embeds, img_hash, txt_embeds, txt_hash, fusion_embeds=None, fusion_hash=None, labels=None, indexs=None, **kwags):
        """-> (loss, loss_dict) from one forward call of the library; the dictionary is detached"""
        if self.objective is None:
            raise self._objective_error
        return self.objective(img_embeds, txt_embeds, labels)

    def object_function(self, img_embeds, img_hash, txt_embeds, txt_hash, fusion_embeds=None, fusion_hash=None, labels=None, indexs=None, **kwags):
        return self.similarity_loss(img_embeds=img_embeds, img_hash=img_hash, txt_embeds=txt_embeds, txt_hash=txt_hash, fusion_embeds=fusion_embeds,
                                    fusion_hash=fusion_hash, labels=labels, indexs=indexs, **kwags)

    @classmethod
    def from_config(cls, cfg, output_dim=16, train_num=10000, txt_token_size=32):
        """the reference's keys and defaults: ``extreme`` is True here and False in the constructor, ``num_experts`` 3 and
        ``expert_layers`` 8 here, and ``output_dim`` doubles for the pair softmax"""
        hash_func = cfg.get("hash_func", "softmax")
        if "softmax" in hash_func:
            output_dim *= 2
        return cls(cfg=cfg, outputDim=output_dim, clipPath=cfg.get("clip_path", "./ViT-B-32.pt"), loss_type=cfg.get("loss_type", "l1"),
                   triplet_margin=cfg.get("triplet_margin", 0.1), train_num=train_num, txt_token_size=txt_token_size, setDim=cfg.get("setDim", 64),
                   dropout=cfg.get("dropout", 0.3), hash_func=hash_func, merge_func=cfg.get("merge_func", "mean"), cls_alpha=cfg.get("cls_alpha", 0.7),
                   decoder_heads=cfg.get("decoder_heads", 8), decoder_layers=cfg.get("decoder_layers", 6), extreme=cfg.get("extreme", True),
                   extreme_T=cfg.get("extreme_T", 0.01), triplet=cfg.get("triplet", True), distance_mode=cfg.get("distance_mode", "cosine"),
                   num_experts=cfg.get("num_experts", 3), expert_layers=cfg.get("expert_layers", 8), slots_per_expert=cfg.get("slots_per_expert", 8),
                   MoE=cfg.get("MoE", False), hidden_dim=cfg.get("hidden_dim", 512), fusion=cfg.get("fusion", True),
                   dim_feedforward=cfg.get("dim_feedforward", 2048), seed=cfg.get("seed", 0))
