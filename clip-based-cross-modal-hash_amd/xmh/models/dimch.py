"""DIMCH's training objective (reference models/DIMCH/DIMCH.py:152-234 chamfer_similarity_loss with distance/distance.py and
loss/triplet_loss.py) through xmh_dimch.hip: ``DIMCHObjective`` holds the reference's constants and maps the token
embeddings ``[B, M, K]`` and codes ``[B, K]`` of both modalities and the labels to ``(loss, loss_dict)``.

The whole objective is ONE forward call (xmh_dimch_loss) and ONE backward call (xmh_dimch_loss_grad) of the library; nothing of
size N x N (N = B M) is ever stored, where the reference builds [N, N] matrices several times a step and an [N, N, N] tensor for its
diversity term.  The loss dictionary has the reference's nested names; its values are detached views of the one output array.

``DIMCHHashLayer`` is the reference's token-set head (models/DIMCH/hash/hash.py) under its state-dict names, one C call per
modality in inference (xmh_head_dimch) and, in train mode, one forward and one backward call behind ``_DIMCHHeadTrain``
(xmh_head_dimch_train_forward / xmh_head_dimch_backward).  ``DIMCH`` (registered as "DIMCH") puts both behind the CLIP towers' token
outputs.  Two departures from the reference: the code is always [B, K] (its ``.squeeze()`` drops the batch axis at B = 1), and tokens
are always taken as [B, T, E] (it decides whether to permute by comparing a dimension with T and goes wrong at B = 50 and B = 32)."""
import ctypes as C

import torch
import torch.nn as nn

from .. import _lib, ops, towers
from .. import retrieval as R
from .._lib import check, current_stream, lib, ptr, workspace
from ..common.register import registry
from .base import BaseModel
from .heads import _DRAW, _param
from .objective import Objective, Spec, need_cuda

MODES = ("smooth_chamfer", "chamfer", "max", "avg")          # XMH_DIMCH_SMOOTH_CHAMFER .. XMH_DIMCH_AVG
HASH_FUNCS = ("tanh", "softmax")                             # XMH_DIMCH_TANH, XMH_DIMCH_SOFTMAX
TERMS = ("loss", "T_i2t", "T_t2i", "mmd", "unif", "Th_i2t", "Th_t2i", "Q_img", "Q_txt")


class DimchConsts(C.Structure):
    """xmh_dimch_consts of include/xmh.h"""
    _fields_ = [("mode", C.c_int), ("hash_func", C.c_int)] + [(k, C.c_float) for k in (
        "denominator", "temperature", "temperature_txt_scale", "token_triplet_margin", "triplet_margin", "mmd_gamma", "triplet_alpha",
        "mmd_alpha", "unif_alpha", "hash_triplet_alpha", "quan_alpha")]


def mode_index(mode):
    """the reference's SetwiseDistance.compute picks by substring, in this order (distance.py:116-123)"""
    for i, key in enumerate(("smooth", "chamfer", "max", "avg")):
        if key in mode:
            return i
    raise ValueError("DIMCH distance mode %r is none of %s" % (mode, ", ".join(MODES)))


def _pack(consts, aux, ts):
    e1, e2, h1, h2 = ts
    B, M, K = e1.shape
    Kh = h1.shape[1]
    cst, C_ = consts
    return (B, M, K, Kh, C_), (ptr(e1), ptr(e2), ptr(h1), ptr(h2), B, M, K, Kh, C_, ptr(aux[0]), C.byref(cst))


# forward = xmh_dimch_loss -> fp32 [9], backward = xmh_dimch_loss_grad (all four gradients, one call; only element 0 carries one).
# The codes' width does not enter the workspace; its bound is the embeddings'.
_DIMCH = Spec(lib.xmh_dimch_loss, lib.xmh_dimch_loss_grad, _pack,
              lambda B, M, K, Kh, C_: 0 if Kh > 256 else lib.xmh_dimch_loss_ws_bytes(B, M, K, C_),
              "DIMCH objective: B=%d M=%d K=%d Kh=%d C=%d outside B <= 512, M <= 64, K, Kh <= 256, C <= 127", out_len=12, terms=9)


class DIMCHObjective(nn.Module):
    """the constants of the reference's DIMCH.__init__ (:44-64: ``distance``, ``chamfer`` and ``hash_pars`` blocks, its defaults) and
    its chamfer_similarity_loss.  No parameters."""

    def __init__(self, mode="chamfer", denominator=2.0, temperature=16.0, temperature_txt_scale=1.0, token_triplet_margin=0.2,
                 triplet_margin=0.3, mmd_gamma=0.5, triplet_alpha=1.0, mmd_alpha=0.01, unif_alpha=0.01, hash_triplet_alpha=0.5,
                 quan_alpha=0.001, hash_func="softmax"):
        super().__init__()
        if hash_func not in HASH_FUNCS:
            raise ValueError("DIMCH hash_func %r is none of %s" % (hash_func, ", ".join(HASH_FUNCS)))
        self.mode, self.hash_func = mode, hash_func
        self.consts = DimchConsts(mode_index(mode), HASH_FUNCS.index(hash_func), denominator, temperature, temperature_txt_scale,
                                  token_triplet_margin, triplet_margin, mmd_gamma, triplet_alpha, mmd_alpha, unif_alpha, hash_triplet_alpha,
                                  quan_alpha)

    @classmethod
    def from_config(cls, cfg):
        """the model block of a configuration (a mapping with ``get``), nested blocks and defaults as the reference reads them"""
        d, c, h = (cfg.get(k, None) or {} for k in ("distance", "chamfer", "hash_pars"))
        return cls(mode=d.get("mode", "chamfer"), denominator=d.get("denominator", 2.0), temperature=d.get("temperature", 16.0),
                   temperature_txt_scale=d.get("temperature_txt_scale", 1.0), token_triplet_margin=c.get("token_triplet_margin", 0.2),
                   triplet_margin=h.get("triplet_margin", 0.3), mmd_gamma=c.get("mmd_gamma", 0.5), triplet_alpha=h.get("triplet_alpha", 1),
                   mmd_alpha=c.get("mmd_alpha", 0.01), unif_alpha=c.get("unif_alpha", 0.01),
                   hash_triplet_alpha=h.get("hash_triplet_alpha", 0.5), quan_alpha=h.get("quan_alpha", 0.001),
                   hash_func=cfg.get("hash_func", "softmax"))

    def terms(self, img_embeds, img_hash, txt_embeds, txt_hash, labels):
        """-> fp32 [9] on the device (TERMS); element 0 carries the gradient"""
        need_cuda(img_embeds, img_hash, txt_embeds, txt_hash)
        labels = torch.as_tensor(labels)
        B = img_embeds.shape[0]
        if img_embeds.dim() != 3 or txt_embeds.shape != img_embeds.shape or img_hash.dim() != 2 or txt_hash.shape != img_hash.shape \
                or img_hash.shape[0] != B or labels.dim() != 2 or labels.shape[0] != B:
            raise RuntimeError("DIMCH objective: embeddings %s / %s, codes %s / %s, labels %s do not fit together"
                               % (tuple(img_embeds.shape), tuple(txt_embeds.shape), tuple(img_hash.shape), tuple(txt_hash.shape),
                                  tuple(labels.shape)))
        lab = R.pack_labels((labels == 1).to(torch.uint8).to(img_embeds.device))
        return Objective.apply(_DIMCH, (self.consts, labels.shape[1]), (lab,), img_embeds, txt_embeds, img_hash, txt_hash)

    def forward(self, img_embeds, img_hash, txt_embeds, txt_hash, labels=None):
        """reference :152-242 -- (loss, loss_dict); without labels every sample is its own class (object_function, :237-242)"""
        if labels is None:
            labels = torch.ones([img_embeds.shape[0]], dtype=torch.int).diag()
        out = self.terms(img_embeds, img_hash, txt_embeds, txt_hash, labels)
        v = out.detach()
        return out[0], {"All loss": v[0],
                        "Tokens": {"Similarity": {"i2t": v[1], "t2i": v[2]}, "Maximum Mean Discrepancy": v[3], "Diversity": v[4]},
                        "Hash": {"Triplet": {"i2t": v[5], "t2i": v[6]}, "Quantization": {"image": v[7], "text": v[8]}}}


# ---- the token-set head (reference models/DIMCH/hash/hash.py:18-100) -------------------------------------------------------------------
class _DIMCHHeadTrain(torch.autograd.Function):
    """forward = xmh_head_dimch_train_forward, backward = xmh_head_dimch_backward: one modality, gradients enter through either output"""

    @staticmethod
    def forward(ctx, mod, tokens, keep, *params):
        embeds, code, x, buf = mod._run(tokens, keep, train=True)
        ctx.mod, ctx.has_keep, ctx.meta = mod, keep is not None, (tokens.shape, tokens.dtype)
        ctx.set_materialize_grads(False)                # an output the loss does not use hands backward None, not a tensor of zeros
        ctx.save_for_backward(x, buf, *params)          # saved parameters: autograd notices an in-place change before backward
        return embeds, code

    @staticmethod
    @torch.autograd.function.once_differentiable      # the gradient kernels are not themselves differentiable
    def backward(ctx, g_embeds, g_code):
        x, buf, *params = ctx.saved_tensors
        mod, need = ctx.mod, ctx.needs_input_grad
        B = x.shape[0]
        gx = torch.empty_like(x) if need[1] else None
        gp = [torch.empty_like(_param(p)) if n else None for p, n in zip(params, need[3:])]
        ups = [None if g is None else g.detach().float().contiguous() for g in (g_embeds, g_code)]
        desc = mod._desc(params)
        grads = _lib.DimchHeadGrads(*[None if t is None else t.data_ptr() for t in (*gp, gx)])
        wsb = C.c_size_t(0)
        lib.xmh_head_dimch_bytes(B, desc.T, desc.E, desc.H, desc.M, desc.K, C.byref(wsb))
        ws = workspace(wsb.value, x.device)
        check(lib.xmh_head_dimch_backward(C.byref(desc), ptr(x), int(ctx.has_keep), float(mod.dropout_p), ptr(ups[0]), ptr(ups[1]), B, ptr(buf),
                                          buf.numel(), C.byref(grads), 0, ptr(ws), ws.numel(), current_stream()), "xmh_head_dimch_backward")
        if gx is not None:
            gx = gx.reshape(ctx.meta[0]).to(ctx.meta[1])
        return (None, gx, None, *gp)


class DIMCHTokenHash(nn.Module):
    """reference TokenHash (:18-52) without ``add_global``: ``token_layer`` Conv1d(T -> M, 3, padding 1) along the embedding axis,
    ``hash_layer`` Linear(E, E / 2), ReLU, Dropout, Linear(E / 2, K); mean over the M set members; tanh or the pair softmax.
    Initial weights follow weights_init_kaiming (models/common/hash.py:5-14) from a private generator seeded with ``seed``: the same
    seed gives the same head whatever the global stream holds.  ``self.training`` alone picks the path, as in heads.py."""

    def __init__(self, inputDim=32, outputDim=64, embedDim=512, setDim=64, dropout=0.3, hash_func="tanh", seed=0):
        super().__init__()
        if hash_func not in HASH_FUNCS:
            raise ValueError("DIMCH hash_func %r is none of %s" % (hash_func, ", ".join(HASH_FUNCS)))
        self.token_layer = nn.Conv1d(inputDim, setDim, kernel_size=3, stride=1, padding=1)
        self.hash_layer = nn.Sequential(nn.Linear(embedDim, embedDim // 2), nn.ReLU(), nn.Dropout(p=dropout), nn.Linear(embedDim // 2, outputDim))
        self.hash_func = hash_func
        self.generator = None                 # torch.Generator of the module's device for the dropout masks; None: the global one
        g = torch.Generator().manual_seed(int(seed))
        nn.init.kaiming_normal_(self.token_layer.weight, a=0, mode="fan_in", generator=g)
        nn.init.constant_(self.token_layer.bias, 0.0)
        for fc in (self.hash_layer[0], self.hash_layer[3]):
            nn.init.kaiming_uniform_(fc.weight, mode="fan_out", generator=g)
            nn.init.constant_(fc.bias, 0.0)

    @property
    def dropout_p(self):
        return float(self.hash_layer[2].p)

    def head_params(self):
        """the six parameters in the order of xmh_dimch_head"""
        return [self.token_layer.weight, self.token_layer.bias, self.hash_layer[0].weight, self.hash_layer[0].bias, self.hash_layer[3].weight,
                self.hash_layer[3].bias]

    def _desc(self, params):
        cw, cb, w1, b1, w2, b2 = (_param(p) for p in params)
        M, T, _ = cw.shape
        return _lib.DimchHead(*(t.data_ptr() for t in (cw, cb, w1, b1, w2, b2)), T, w1.shape[1], w1.shape[0], M, w2.shape[0],
                              HASH_FUNCS.index(self.hash_func))

    def draw_keep_mask(self, B: int, device):
        """the dropout keep mask of one train-mode forward, uint8 [B M, E / 2] on the device, or None when p == 0; drawn here with
        ``torch.rand(..., generator=self.generator) >= p`` as DSPHLinearHash does: the library draws no random numbers"""
        p = self.dropout_p
        if p <= 0.0:
            return None
        if p >= 1.0:
            raise ValueError("dropout p = %g: nothing would be kept" % p)
        M, H = self.token_layer.weight.shape[0], self.hash_layer[0].weight.shape[0]
        return (torch.rand(B * M, H, device=device, generator=self.generator) >= p).view(torch.uint8)

    def _run(self, tokens, keep, train):
        """one forward call -> (embeds [B, M, K], code [B, K], the tokens as the kernels read them, the buffer the call filled)"""
        T, E = self.token_layer.weight.shape[1], self.hash_layer[0].weight.shape[1]
        if tokens.dim() != 3 or tuple(tokens.shape[1:]) != (T, E):
            raise ValueError("a DIMCH head takes [B, %d, %d] tokens, got %s" % (T, E, tuple(tokens.shape)))
        x = ops._f32c(tokens.detach()).contiguous()
        B = x.shape[0]
        desc = self._desc(self.head_params())
        nbytes = lib.xmh_head_dimch_bytes(B, desc.T, desc.E, desc.H, desc.M, desc.K, None)
        if nbytes == 0:
            raise RuntimeError("DIMCH head: B=%d T=%d E=%d M=%d K=%d outside B M <= 32768, T <= 256, E <= 2048, K <= 256"
                               % (B, desc.T, desc.E, desc.M, desc.K))
        buf = workspace(nbytes, x.device)
        embeds = torch.empty(B, desc.M, desc.K, dtype=torch.float32, device=x.device)
        code = torch.empty(B, desc.K, dtype=torch.float32, device=x.device)
        if train:
            check(lib.xmh_head_dimch_train_forward(C.byref(desc), ptr(x), ptr(keep), self.dropout_p, B, ptr(embeds), ptr(code), ptr(buf), nbytes,
                                                   current_stream()), "xmh_head_dimch_train_forward")
        else:
            check(lib.xmh_head_dimch(C.byref(desc), ptr(x), B, ptr(embeds), ptr(code), ptr(buf), nbytes, current_stream()), "xmh_head_dimch")
        return embeds, code, x, buf

    def _train(self, tokens, keep=_DRAW):
        """train-mode forward; `keep` overrides the drawn mask (uint8 [B M, E / 2], or None for no dropout) -- tests replay stored masks"""
        if keep is _DRAW:
            keep = self.draw_keep_mask(tokens.shape[0], tokens.device)
        elif keep is not None:
            keep = keep.to(device=tokens.device, dtype=torch.uint8).contiguous()
        params = self.head_params()
        if torch.is_grad_enabled() and (tokens.requires_grad or any(p.requires_grad for p in params)):
            return _DIMCHHeadTrain.apply(self, tokens, keep, *params)
        return self._run(tokens, keep, train=True)[:2]

    @torch.no_grad()
    def _infer(self, tokens):
        return self._run(tokens, None, train=False)[:2]

    def forward(self, tokens, keep=_DRAW):
        """tokens [B, T, E] -> (embeds [B, M, K], code [B, K])"""
        return self._train(tokens, keep) if self.training else self._infer(tokens)


class DIMCHHashLayer(nn.Module):
    """reference HashLayer (:55-100) under its attribute names, so that a reference checkpoint loads strictly: twelve entries,
    ``{img,txt}_token_hash.token_layer.{weight [M, T, 3], bias [M]}``, ``.hash_layer.0.{weight [E / 2, E], bias}`` and
    ``.hash_layer.3.{weight [K, E / 2], bias}``.  ``add_global`` is never set by DIMCH and is not built."""

    def __init__(self, visual_tokens=48, txt_tokens=32, feature_size=512, outputDim=64, setDim=64, dropout=0.3, add_global=False,
                 hash_func_="tanh", merge_func="mean", seed=0):
        super().__init__()
        if add_global:
            raise NotImplementedError("DIMCH never sets add_global; the head is built without it")
        if merge_func != "mean":
            raise NotImplementedError("DIMCH's head merges the set by its mean (merge_func %r)" % (merge_func,))
        self.hash_func_ = hash_func_
        self.img_token_hash = DIMCHTokenHash(visual_tokens, outputDim, feature_size, setDim, dropout, hash_func_, seed=seed)
        self.txt_token_hash = DIMCHTokenHash(txt_tokens, outputDim, feature_size, setDim, dropout, hash_func_, seed=seed + 1)

    def encode_img(self, token_embeds, keep=_DRAW):
        """-> (token_embeds [B, M, K], token_hash [B, K]); `keep` replays a stored dropout mask in train mode"""
        return self.img_token_hash(token_embeds, keep)

    def encode_txt(self, token_embeds, keep=_DRAW):
        return self.txt_token_hash(token_embeds, keep)

    def encode_img_train(self, token_embeds, keep=_DRAW):
        """the train-mode path whatever ``self.training`` says (behind torch.autograd when anything requires grad)"""
        return self.img_token_hash._train(token_embeds, keep)

    def encode_txt_train(self, token_embeds, keep=_DRAW):
        return self.txt_token_hash._train(token_embeds, keep)

    def quantization(self, code):
        """reference :87-88"""
        if self.hash_func_ == "tanh":
            return torch.tanh(code)
        return torch.softmax(code.reshape(code.shape[0], -1, 2), dim=-1).reshape(code.shape[0], -1)

    def forward(self, img_token_embeds, txt_token_embeds):
        return (*self.encode_img(img_token_embeds), *self.encode_txt(txt_token_embeds))


@registry.register_model("DIMCH")
class DIMCH(BaseModel):
    """reference models/DIMCH/DIMCH.py:13-243: CLIP in return_patches mode, the token-set head over every token row of both towers
    (the image side with the cls row first), and the set-distance objective."""

    def __init__(self, cfg, outputDim=16, clipPath="./ViT-B-32.pt", triplet_margin=0.1, train_num=10000, txt_token_size=32, setDim=64,
                 dropout=0.3, hash_func="softmax", merge_func="mean", cls_alpha=0.7, seed=0, **kwags):
        super().__init__(cfg)
        self.hash_func = hash_func
        embed_dim, visual_token_size, self.backbone = self.load_backbone(clipPath=clipPath, return_patches=True)
        self.visual_token_size, self.txt_token_size, self.cls_alpha = visual_token_size, txt_token_size, cls_alpha
        self.hash = DIMCHHashLayer(visual_tokens=visual_token_size, txt_tokens=txt_token_size, feature_size=embed_dim, outputDim=outputDim,
                                   setDim=setDim, dropout=dropout, hash_func_=hash_func, merge_func=merge_func, seed=seed)
        self.output_dim = outputDim
        self.objective = DIMCHObjective.from_config(cfg if cfg is not None else {})
        self.objective.hash_func = hash_func                  # the constructor's argument decides (reference :34, :142-147)
        self.objective.consts.hash_func = HASH_FUNCS.index(hash_func)
        self.triplet_margin = self.objective.consts.triplet_margin

    @staticmethod
    def _image_tokens(cls_token, seq_tokens):
        """cls [B, E] and the patch rows [L - 1, B, E] (the towers' LND view) -> [B, L, E], the cls row first (reference :68-74)"""
        return torch.cat([cls_token.unsqueeze(1), seq_tokens.permute(1, 0, 2)], dim=1)

    def encode_image(self, image):
        cls_token, seq_tokens, _ = self.backbone.encode_image(image)
        return self.hash.encode_img(self._image_tokens(cls_token, seq_tokens))

    def encode_text(self, text):
        # the head reads every token row and there is no key padding mask (reference :80-85): masked_rows="exact"
        _, tokens, _, _ = self.backbone.encode_text(text, masked_rows="exact")
        return self.hash.encode_txt(tokens.permute(1, 0, 2))

    def forward(self, image, text, labels=None, indexs=None, return_loss=False):
        """reference :116-123 -- (img_embeds, img_hash, txt_embeds, txt_hash), or the objective of them"""
        (img_embeds, img_hash), (txt_embeds, txt_hash) = towers.run_both(lambda: self.encode_image(image), lambda: self.encode_text(text))
        if return_loss:
            return self.object_function(img_embeds, img_hash, txt_embeds, txt_hash, labels=labels, indexs=indexs)
        return img_embeds, img_hash, txt_embeds, txt_hash

    def forward_train(self, image, text):
        """the four tensors of ``forward`` with a graph through the head AND both towers (encode_*_train_tokens)"""
        cls_token, seq_tokens = self.backbone.encode_image_train_tokens(image)
        _, txt_tokens, _ = self.backbone.encode_text_train_tokens(text)
        return (*self.hash.encode_img_train(self._image_tokens(cls_token, seq_tokens)), *self.hash.encode_txt_train(txt_tokens.permute(1, 0, 2)))

    def forward_train_heads(self, image, text):
        """the same four tensors with a graph through the head only: the towers run as in ``forward`` under no_grad (a frozen backbone)"""
        with torch.no_grad():
            cls_token, seq_tokens, _ = self.backbone.encode_image(image)
            _, txt_tokens, _, _ = self.backbone.encode_text(text, masked_rows="exact")
        return (*self.hash.encode_img_train(self._image_tokens(cls_token, seq_tokens)), *self.hash.encode_txt_train(txt_tokens.permute(1, 0, 2)))

    def chamfer_similarity_loss(self, img_embeds, img_hash, txt_embeds, txt_hash, labels=None, indexs=None, **kwags):
        """reference :152-234 -- (loss, loss_dict) from one forward call of the library; the dictionary is detached"""
        return self.objective(img_embeds, img_hash, txt_embeds, txt_hash, labels)

    def object_function(self, img_embeds, img_hash, txt_embeds, txt_hash, labels=None, indexs=None, **kwags):
        """reference :237-242: without labels every sample is its own class"""
        return self.chamfer_similarity_loss(img_embeds=img_embeds, img_hash=img_hash, txt_embeds=txt_embeds, txt_hash=txt_hash, labels=labels,
                                            indexs=indexs, **kwags)

    @classmethod
    def from_config(cls, cfg, output_dim=16, train_num=10000, txt_token_size=32):
        """reference :87-114, the doubling of ``output_dim`` for the pair softmax included"""
        hash_func = cfg.get("hash_func", "softmax")
        if "softmax" in hash_func:
            output_dim *= 2
        return cls(cfg=cfg, outputDim=output_dim, clipPath=cfg.get("clip_path", "./ViT-B-32.pt"), triplet_margin=cfg.get("triplet_margin", 0.1),
                   train_num=train_num, txt_token_size=txt_token_size, setDim=cfg.get("setDim", 64), dropout=cfg.get("dropout", 0.3),
                   hash_func=hash_func, merge_func=cfg.get("merge_func", "mean"), cls_alpha=cfg.get("cls_alpha", "0.7"),
                   seed=cfg.get("seed", 0))
