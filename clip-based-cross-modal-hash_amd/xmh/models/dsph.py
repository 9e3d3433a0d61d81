"""DSPH model wrapper (reference models/DSPH/DSPH.py:13-82): backbone + Linear/tanh head, registered as "DSPH", and its HyP loss
(models/DSPH/loss/HyP.py) through xmh_hyp.hip.  A reference DSPH checkpoint carries ``hyp.proxies`` [numclass, K]
(models/DSPH/loss/HyP.py:15-16) beside ``backbone.*`` and ``hash.*`` -- pinned by tests/golden/runner.npz (DSPH_state_keys, from the
reference's own class) -- so the module tree here has it too and ``load_state_dict`` of such a checkpoint succeeds strictly.

The reference reads the HyP threshold out of ``loss/codetable.xlsx`` at construction (:33-35).  Here it is, in this order: an
explicit ``threshold`` (constructor argument or ``cfg.threshold``); the cell of ``cfg.codetable`` (a path to the user's copy of
that workbook, read by codetable.hyp_threshold); otherwise unset -- the model constructs and encodes as usual and the first loss
call raises ValueError.

In `.train()` mode the two heads (heads.py::DSPHLinearHash) run dropout with a keep mask drawn on the device and carry the loss
gradient on to `fc.weight`, `fc.bias` and the embeddings (xmh_head_grad.hip); `forward_train` (base.py) hands it on to both CLIP
towers (xmh_tower_grad.hip)."""
import torch
import torch.nn as nn

from .. import retrieval as R
from .._lib import lib, ptr
from ..common.register import registry
from .base import BaseModel
from .codetable import hyp_threshold
from .heads import DSPHHashLayer
from .objective import Objective, Spec, need_cuda


class HyPProxies(nn.Module):
    """the reference's HyP loss (models/DSPH/loss/HyP.py:7-70): ``proxies`` [numclass, output_dim], randn then
    kaiming_normal_(fan_out).  The reference seeds the GLOBAL generator with ``hypseed`` to draw them; a private generator is used
    here so that constructing a model has no side effect on the caller's random stream (values of a freshly constructed model
    therefore differ from the reference's; a loaded checkpoint overwrites them either way)."""

    def __init__(self, numclass=80, output_dim=16, hypseed=0, alpha=0.8, threshold=None):
        super().__init__()
        self.alpha, self.threshold = alpha, threshold
        g = torch.Generator().manual_seed(int(hypseed))
        std = (2.0 / max(1, numclass)) ** 0.5                          # kaiming_normal_, mode="fan_out" of a [numclass, output_dim] matrix
        self.proxies = nn.Parameter(torch.randn(numclass, output_dim, generator=g) * std)

    def forward(self, x=None, y=None, label=None):
        """reference HyP.forward (:18-70): the loss as a 0-dim fp32 device tensor, differentiable with respect to x, y and the
        proxies.  `label` is the [B, numclass] 0/1 matrix; on another device it is moved, as the reference does."""
        if self.threshold is None:
            raise ValueError("DSPH's HyP loss has no threshold: set `threshold` in the model config, or `codetable` to the path of "
                             "the reference's codetable.xlsx")
        need_cuda(x, y, self.proxies)
        if x.dim() != 2 or y.shape != x.shape or label.dim() != 2 or label.shape[0] != x.shape[0] \
                or label.shape[1] != self.proxies.shape[0] or x.shape[1] != self.proxies.shape[1]:
            raise RuntimeError("HyP loss: x %s, y %s, label %s, proxies %s do not fit together"
                               % (tuple(x.shape), tuple(y.shape), tuple(label.shape), tuple(self.proxies.shape)))
        if label.device != x.device:
            label = label.to(x.device)
        return Objective.apply(_HYP, (float(self.threshold), float(self.alpha)), (R.pack_labels(label),), x, y, self.proxies)


def _pack(consts, aux, ts):
    x, y, P = ts
    B, K = x.shape
    C = P.shape[0]
    return (B, K, C), (ptr(x), ptr(y), ptr(P), B, K, C, ptr(aux[0]), *consts)


# forward = xmh_hyp_loss -> the loss as a 0-dim tensor, backward = xmh_hyp_loss_grad (with respect to x, y and the proxies, one call)
_HYP = Spec(lib.xmh_hyp_loss, lib.xmh_hyp_loss_grad, _pack, lib.xmh_hyp_loss_ws_bytes,
            "HyP loss: B=%d K=%d C=%d outside B <= 4096, K <= 4096, C <= 1024", out_len=8, terms=0, null_grads=False)


@registry.register_model("DSPH")
class DSPH(BaseModel):
    def __init__(self, cfg, outputDim=16, clipPath="./ViT-B-32.pt", train_num=10000, numclass=80, hypseed=1, alpha=0, threshold=None,
                 codetable=None):
        super().__init__(cfg)
        embed_dim, self.backbone = self.load_backbone(clipPath=clipPath, return_patches=False)
        self.hash = DSPHHashLayer(inputDim=embed_dim, outputDim=outputDim)
        self.output_dim, self.numclass, self.hypseed, self.alpha = outputDim, numclass, hypseed, alpha
        threshold = self.resolve_threshold(cfg, outputDim, numclass, threshold, codetable)
        self.hyp = HyPProxies(numclass=numclass, output_dim=outputDim, hypseed=hypseed, alpha=alpha, threshold=threshold)

    @staticmethod
    def resolve_threshold(cfg, output_dim, numclass, threshold=None, codetable=None):
        """explicit threshold (argument, then cfg.threshold), else the cell of the codetable (argument, then cfg.codetable), else None"""
        get = cfg.get if hasattr(cfg, "get") else (lambda k, d=None: d)
        if threshold is None:
            threshold = get("threshold", None)
        if threshold is not None:
            return float(threshold)
        if codetable is None:
            codetable = get("codetable", None)
        return None if codetable is None else hyp_threshold(codetable, output_dim, numclass)

    def encode_image(self, image):
        return self.hash.encode_img(self.backbone.encode_image(image))

    def encode_text(self, text):
        return self.hash.encode_txt(self.backbone.encode_text(text))

    def loss(self, image, text, labels=None, indexs=None, **kwags):
        """reference :68-76 -- (loss, {"All loss": detached loss})"""
        loss = self.hyp(image, text, labels)
        return loss, {"All loss": loss.detach()}

    def object_function(self, img_hash, txt_hash, labels=None, indexs=None, **kwags):
        """reference :78-82 -- without labels every sample is its own class, which fits the proxies only when numclass == B"""
        if labels is None:
            if img_hash.shape[0] != self.hyp.proxies.shape[0]:
                raise RuntimeError("object_function without labels needs numclass == batch size (numclass %d, batch %d): the "
                                   "identity labels are [B, B]" % (self.hyp.proxies.shape[0], img_hash.shape[0]))
            labels = torch.ones([img_hash.shape[0]], dtype=torch.int).diag()
        return self.loss(img_hash, txt_hash, labels, indexs, **kwags)

    @classmethod
    def from_config(cls, cfg, output_dim=16, train_num=10000):
        return cls(cfg=cfg, outputDim=output_dim, clipPath=cfg.get("clip_path", "./ViT-B-32.pt"), train_num=train_num,
                   numclass=cfg.get("numclass", 80), hypseed=cfg.get("hypseed", 0), alpha=cfg.get("alpha", 0.8))
