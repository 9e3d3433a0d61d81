"""DNPH model wrapper (reference models/DNPH/DNPH.py:10-105): CLIP backbone + a head with two outputs per modality (the tanh code
and 80 class logits, heads.py::DNPHHashLayer), registered as "DNPH", and its objective through xmh_dnph.hip:

  loss1  reference loss/loss.py:12-33 -- softmax over the squared distances of the L2-normalised codes to the L2-normalised class
         ``proxies`` with an additive margin on the codes' own classes, plus the cross-entropy of both class-prediction outputs
         against the argmax of the label row
  noise  reference DNPH.py:77-89 and loss/b_reg.py -- random +-1 vectors, assigned to the batch's codes so that the total L2 distance
         is minimal (xmh_assign_min_cost on the host, what the reference asks of scipy), pull each code towards a corner of the cube

A reference checkpoint carries ``loss.proxies`` [numclass, K] beside ``backbone.*`` and ``hash.*``; the module tree here has the
same names and shapes (tests/golden/dnph.npz pins the head's) and loads it strictly.

The whole objective, noise term included, is ONE forward call (xmh_dnph_loss) and ONE backward call (xmh_dnph_loss_grad) of the
library.  The assignment needs the codes on the host: ``gene_noise`` copies the detached B x K floats back, once per step for both
modalities -- the reference's own synchronisation (``img_hash.cpu()``), kept because the solver is sequential and B x B."""
import numpy as np
import torch
import torch.nn as nn

from .. import retrieval as R
from .._lib import check, lib, ptr
from ..common.register import registry
from .base import BaseModel
from .heads import DNPHHashLayer
from .objective import Objective, Spec, need_cuda


def assign_min_cost(cost):
    """the square linear sum assignment of a [n, n] cost matrix (float64, host) -> col_of_row int32 [n], total cost minimal:
    xmh_assign_min_cost (shortest augmenting paths), the package's stand-in for scipy.optimize.linear_sum_assignment"""
    cost = np.ascontiguousarray(cost, dtype=np.float64)
    if cost.ndim != 2 or cost.shape[0] != cost.shape[1]:
        raise ValueError("assign_min_cost: a square cost matrix is needed, got %s" % (cost.shape,))
    cols = np.empty(cost.shape[0], dtype=np.int32)
    check(lib.xmh_assign_min_cost(cost.ctypes.data, cost.shape[0], cols.ctypes.data), "xmh_assign_min_cost")
    return cols


def gene_noise(embeddings, noises):
    """reference loss/b_reg.py:19-41: row i of the result is the noise vector assigned to code i, the assignment minimising the sum
    of ``||h_i - s_j||_2``.  embeddings [B, K] float32 (host), noises [B, K] integer +-1 -> float64 [B, K], as the reference"""
    h = np.asarray(embeddings)
    s = np.asarray(noises)
    if h.ndim != 2 or s.shape != h.shape:
        raise ValueError("gene_noise: codes %s and noises %s do not fit together" % (h.shape, s.shape))
    # np.linalg.norm(fts - noises, axis=1) of the reference: float32 codes minus integers is a float64 difference
    diff = h.astype(np.float64)[:, None, :] - s.astype(np.float64)[None, :, :]
    cost = np.sqrt((diff * diff).sum(-1))
    return s[assign_min_cost(cost)].astype(np.float64)


class DNPHLoss(nn.Module):
    """the reference's Loss (loss/loss.py:5-33): ``proxies`` [numclass, output_dim] = randn / 8, and ``mrg``.  The reference draws
    them from the GLOBAL generator; a private one, seeded with ``seed``, is used here so that constructing a model has no side effect
    on the caller's random stream (values of a freshly constructed model therefore differ from the reference's; a loaded checkpoint
    overwrites them either way)."""

    def __init__(self, num_classes=80, output_dim=16, mrg=1.0, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(int(seed))
        self.proxies = nn.Parameter(torch.randn(num_classes, output_dim, generator=g) / 8)
        self.mrg = mrg

    def forward(self, feature_1, feature_2, predict_1, predict_2, label_1, label_2=None):
        """reference Loss.forward (:12-33): p_loss + d_loss as a 0-dim fp32 device tensor, differentiable with respect to the four
        inputs and the proxies.  The reference passes the same labels twice; ``label_2`` is accepted and must be them."""
        return self.terms(feature_1, feature_2, predict_1, predict_2, label_1, label_2)[0]

    def terms(self, feature_1, feature_2, predict_1, predict_2, label_1, label_2=None, noise_1=None, noise_2=None, noise_alpha=0.0):
        """-> fp32 [6] on the device: loss, p_loss, d_loss of the image and of the text prediction, and the two noise means (0
        without noises); element 0 carries the gradient.  With ``noise_1`` / ``noise_2`` ([B, K] +-1) element 0 is the whole
        objective of DNPH.compute_loss, ``loss1 - noise_alpha (noise_img + noise_txt)``, from the same two library calls."""
        need_cuda(feature_1, feature_2, predict_1, predict_2, self.proxies)
        label_1 = torch.as_tensor(label_1)
        if label_2 is not None and label_2 is not label_1 and not torch.equal(torch.as_tensor(label_2).to(label_1.device), label_1):
            raise ValueError("DNPH loss: the two label matrices differ; both modalities of a pair carry the same labels")
        B, K = feature_1.shape if feature_1.dim() == 2 else (-1, -1)
        C = self.proxies.shape[0]
        if B < 0 or feature_2.shape != feature_1.shape or predict_1.dim() != 2 or predict_2.shape != predict_1.shape \
                or predict_1.shape[0] != B or tuple(label_1.shape) != (B, C) or K != self.proxies.shape[1]:
            raise RuntimeError("DNPH loss: codes %s / %s, predictions %s / %s, labels %s, proxies %s do not fit together"
                               % (tuple(feature_1.shape), tuple(feature_2.shape), tuple(predict_1.shape), tuple(predict_2.shape),
                                  tuple(label_1.shape), tuple(self.proxies.shape)))
        if predict_1.shape[1] < C:
            raise RuntimeError("DNPH loss: %d class logits for %d classes" % (predict_1.shape[1], C))
        noises = [None if n is None else torch.as_tensor(n).to(device=feature_1.device, dtype=torch.float32).contiguous()
                  for n in (noise_1, noise_2)]
        for n in noises:
            if n is not None and n.shape != feature_1.shape:
                raise RuntimeError("DNPH loss: noises %s for codes %s" % (tuple(n.shape), tuple(feature_1.shape)))
        lab = R.pack_labels((label_1 == 1).to(torch.uint8).to(feature_1.device))          # the reference tests `label == 1` (:24)
        return Objective.apply(_DNPH, (float(self.mrg), float(noise_alpha)), (lab, *noises), feature_1, feature_2, predict_1, predict_2,
                               self.proxies)


def _pack(consts, aux, ts):
    f1, f2, p1, p2, P = ts
    B, K = f1.shape
    C, Cp = P.shape[0], p1.shape[1]
    lab, n1, n2 = aux
    return (B, K, C, Cp), (ptr(f1), ptr(f2), ptr(p1), ptr(p2), ptr(P), B, K, C, Cp, ptr(lab), *consts, ptr(n1), ptr(n2))


# forward = xmh_dnph_loss -> fp32 [6], backward = xmh_dnph_loss_grad (all five gradients, one call; only element 0 carries one)
_DNPH = Spec(lib.xmh_dnph_loss, lib.xmh_dnph_loss_grad, _pack, lib.xmh_dnph_loss_ws_bytes,
             "DNPH loss: B=%d K=%d C=%d Cp=%d outside B <= 4096, K <= 4096, Cp >= C, C, Cp <= 1024", out_len=8, terms=6)


@registry.register_model("DNPH")
class DNPH(BaseModel):
    def __init__(self, cfg, outputDim=16, clipPath="./ViT-B-32.pt", train_num=10000, numclass=80, mrg=1.0, noise_alpha=0.1, seed=0):
        super().__init__(cfg)
        embed_dim, self.backbone = self.load_backbone(clipPath=clipPath, return_patches=False)
        self.hash = DNPHHashLayer(inputDim=embed_dim, outputDim=outputDim)        # the reference hands no numclass on: 80 logits
        self.output_dim = outputDim
        self.loss = DNPHLoss(num_classes=numclass, mrg=mrg, output_dim=outputDim, seed=seed)
        self.noise_alpha = noise_alpha
        # the +-1 noise vectors of compute_loss come from this generator, the model's own and seeded from the config (``seed``), not
        # from numpy's global one as the reference's rand_unit_rect: a seeded run repeats, and drawing has no side effect on the caller
        self.noise_generator = np.random.default_rng(int(seed))

    def encode_image(self, image):
        return self.hash.encode_img(self.backbone.encode_image(image))

    def encode_text(self, text):
        return self.hash.encode_txt(self.backbone.encode_text(text))

    def encode_image_train(self, image):
        return self.hash.encode_img(self.backbone.encode_image_train(image))

    def encode_text_train(self, text):
        return self.hash.encode_txt(self.backbone.encode_text_train(text))

    def forward(self, image, text, labels=None, indexs=None, return_loss=False):
        """reference :45-52 -- (img_hash, txt_hash, img_pre, txt_pre), or the objective of them"""
        img_hash, img_pre = self.encode_image(image)
        txt_hash, txt_pre = self.encode_text(text)
        if return_loss:
            return self.object_function(img_hash=img_hash, txt_hash=txt_hash, img_pre=img_pre, txt_pre=txt_pre, labels=labels, indexs=indexs)
        return img_hash, txt_hash, img_pre, txt_pre

    def forward_train(self, image, text):
        """the four outputs a training step differentiates (what the reference's ``model(image, text)`` is in train mode): gradients
        reach every parameter of the head and of both towers that has requires_grad"""
        img_hash, img_pre = self.encode_image_train(image)
        txt_hash, txt_pre = self.encode_text_train(text)
        return img_hash, txt_hash, img_pre, txt_pre

    def rand_unit_rect(self, npoints, ndim):
        """reference loss/b_reg.py:5-16: [npoints, ndim] integers, +1 or -1 with equal probability -- from ``self.noise_generator``
        (see the constructor), not from numpy's global generator"""
        return self.noise_generator.integers(0, 2, size=(npoints, ndim), dtype=np.int64) * 2 - 1

    def compute_loss(self, img_hash, txt_hash, img_pre, txt_pre, labels=None, indexs=None, noises=None, **kwags):
        """reference :72-99 -- (loss, {"All loss", "Noise": {"image", "text"}}), the dictionary detached.  ``noises`` ([B, K] +-1)
        overrides the draw of the vectors that are assigned to the codes (tests replay stored ones); the two assignments are
        gene_noise's.  One host round trip: the detached codes of both modalities, B x K floats each."""
        B, K = img_hash.shape
        s_vector = self.rand_unit_rect(B, K) if noises is None else np.asarray(torch.as_tensor(noises).cpu())
        codes = torch.stack([img_hash.detach().float(), txt_hash.detach().float()]).cpu().numpy()      # the step's one synchronisation
        i_noises = torch.from_numpy(gene_noise(codes[0], s_vector)).float()
        t_noises = torch.from_numpy(gene_noise(codes[1], s_vector)).float()
        out = self.loss.terms(img_hash, txt_hash, img_pre, txt_pre, labels, labels, noise_1=i_noises, noise_2=t_noises, noise_alpha=self.noise_alpha)
        v = out.detach()
        return out[0], {"All loss": v[0], "Noise": {"image": v[4], "text": v[5]}}

    def object_function(self, img_hash, txt_hash, img_pre, txt_pre, labels=None, indexs=None, **kwags):
        """reference :101-105 -- without labels every sample is its own class, which fits the proxies only when numclass == B"""
        if labels is None:
            if img_hash.shape[0] != self.loss.proxies.shape[0]:
                raise RuntimeError("object_function without labels needs numclass == batch size (numclass %d, batch %d): the "
                                   "identity labels are [B, B]" % (self.loss.proxies.shape[0], img_hash.shape[0]))
            labels = torch.ones([img_hash.shape[0]], dtype=torch.int).diag()
        return self.compute_loss(img_hash, txt_hash, img_pre, txt_pre, labels, indexs, **kwags)

    @classmethod
    def from_config(cls, cfg, output_dim=16, train_num=10000):
        """reference :54-70, its quirk included: ``noise_alpha`` defaults to 1.0 here and to 0.1 in the constructor"""
        return cls(cfg=cfg, outputDim=output_dim, clipPath=cfg.get("clip_path", "./ViT-B-32.pt"), train_num=train_num,
                   numclass=cfg.get("numclass", 80), mrg=cfg.get("mrg", 1.0), noise_alpha=cfg.get("noise_alpha", 1.0),
                   seed=cfg.get("seed", 0))
