"""TwDH model wrapper (reference models/TwDH/TwDH.py:10-230): CLIP backbone + the DCMHT hash layer at ``long_dim`` bits, and
for every configured short length a fixed ``[2*long, 2*short]`` transform followed by the pair softmax
(``quantization(long_hash.matmul(trans))``, :66-85).  Registered as "TwDH".

The reference torch.load()s the centre / transform tensors from ``<long_center>/<long>.pkl``,
``<short_center>/<short>.pkl`` and ``<trans_matrix>/<long>/<short>.pkl``; the same layout is read here.  Without such files
(benchmarks, tests) ``trans_matrix: synthetic`` + ``short_dims: [..]`` builds seeded transforms instead, and ``long_center:
synthetic`` / ``short_center: synthetic`` seeded +-1 centres for ``num_classes`` classes.  The centres only enter the training
loss: they are loaded when their path exists, and a model without them encodes as before.

Training: ``forward_train_codes`` runs both towers and ``self.hash`` in train mode behind torch.autograd and the
short codes through ``_ShortCodes`` (xmh_twdh_short_forward / _backward: all transforms as one exact-fp32 product).  The
objective (:125-190: hash-centre BCE + quantisation term over the long code and every short code) is ``_Objective`` over
xmh_twdh_targets / xmh_twdh_loss / xmh_twdh_loss_grad."""
import ctypes
import os

import torch

from .. import _lib, ops
from .. import retrieval as R
from .._lib import check, current_stream, lib, ptr
from ..common.register import registry
from .base import BaseModel
from .heads import DCMHTHashLayer
from .objective import need_cuda
from .weights import _gen


def _load_center(path, key):
    """one centre file -> fp32 [C, K] with every entry +1 or -1 (the kernels sum them as integers)"""
    c = torch.load(path, map_location="cpu").float()
    return _check_center(c, "%s (%s)" % (key, path))


def _check_center(c, what):
    if c.dim() != 2 or not bool(((c == 1) | (c == -1)).all()):
        raise ValueError("TwDH %s: a hash centre is a [classes, bits] matrix of +1 / -1, got shape %s with other entries or ranks"
                         % (what, tuple(c.shape)))
    return c


@registry.register_model("TwDH")
class TwDH(BaseModel):
    def __init__(self, cfg, long_dim=512, short_dim=16, clipPath="./ViT-B-32.pt", train_num=10000, hash_func="softmax",
                 trans="./data/transformer/TwDH/center/trans", short_dims=None, quan_alpha=0.5, low_rate=0, long_center=None,
                 short_center=None, num_classes=80):
        super().__init__(cfg)
        embed_dim, self.backbone = self.load_backbone(clipPath=clipPath, return_patches=False)
        self.hash = DCMHTHashLayer(feature_size=embed_dim, outputDim=long_dim, num_heads=8, batch_first=True, hash_func_=hash_func)
        self.output_dim = self.long_dim = long_dim
        self.quan_alpha, self.low_rate = quan_alpha, low_rate
        self.trans = {}                                         # key (short length as str) -> [2*long, 2*short] fp32
        if trans == "synthetic":
            for sd in (short_dims or [short_dim]):
                g = _gen(1814, "twdh_trans/%d/%d" % (long_dim, sd))
                self.trans[str(sd)] = torch.randn(2 * long_dim, 2 * sd, generator=g) * (2 * long_dim) ** -0.5
        elif os.path.isfile(trans):
            self.trans[os.path.basename(trans).strip().split(".")[0]] = torch.load(trans, map_location="cpu").float()
        else:
            for item in sorted(os.listdir(trans)):
                self.trans[item.strip().split(".")[0]] = torch.load(os.path.join(trans, item), map_location="cpu").float()
        self.short_dims = [int(k) for k in self.trans]
        self._trans_t = {}                                      # device copies, transposed to the nn.Linear layout gemm_nt takes
        # the hash centres (reference :35-44): long_center fp32 [C, long_dim] or None, short_center {key: fp32 [C, short]}
        self.long_center, self.short_center = None, {}
        if long_center == "synthetic":
            self.long_center = self._synthetic_center(num_classes, long_dim, "long")
        elif long_center is not None and os.path.isfile(long_center):
            self.long_center = _load_center(long_center, "long_center")
        if short_center == "synthetic":
            self.short_center = {k: self._synthetic_center(num_classes, int(k), "short") for k in self.trans}
        elif short_center is not None and os.path.isfile(short_center):
            self.short_center = {os.path.basename(short_center).strip().split(".")[0]: _load_center(short_center, "short_center")}
        elif short_center is not None and os.path.isdir(short_center):
            self.short_center = {item.strip().split(".")[0]: _load_center(os.path.join(short_center, item), "short_center")
                                 for item in sorted(os.listdir(short_center))}
        self._train_cache = None                                # device constants of the training path (_constants)

    @staticmethod
    def _synthetic_center(num_classes, bits, which):
        g = _gen(1814, "twdh_center/%s/%d/%d" % (which, num_classes, bits))
        return (torch.randint(0, 2, (num_classes, bits), generator=g) * 2 - 1).float()

    def get_short_dims(self):
        return self.short_dims

    def _short(self, long_hash):
        out = {}
        for k, v in self.trans.items():
            w = self._trans_t.get(k)
            if w is None or w.device != long_hash.device:
                w = v.to(long_hash.device).t().contiguous()
                self._trans_t[k] = w
            out[k] = ops.pair_softmax(ops.gemm_nt(long_hash, w))  # quantization(long_hash.matmul(v)), TwDH.py:73,83
        return out

    # ---- training ---------------------------------------------------------------------------------------------------
    def _constants(self, device):
        """what the training path keeps on the device: T_cat [2L, 2S] (the transforms side by side, in self.trans' order), its
        transpose, and -- with centres -- the int8 centres of all streams side by side [C, K_tot] and the stream table"""
        src = list(self.trans.values()) + [self.long_center] + list(self.short_center.values())
        c = self._train_cache
        # rebuilt when a matrix is replaced or the model moves (the cache holds the very tensors it was built from)
        if c is not None and c["device"] == device and len(c["src"]) == len(src) and all(a is b for a, b in zip(c["src"], src)):
            return c
        c = {"device": device, "src": src}
        for k, v in self.trans.items():
            if tuple(v.shape) != (2 * self.long_dim, 2 * int(k)):
                raise ValueError("TwDH trans_matrix: transform %r is %s, not [2 * long_dim, 2 * %s]" % (k, tuple(v.shape), k))
        if self.trans:
            cat = torch.cat(list(self.trans.values()), 1).float().to(device)
            c["trans"], c["trans_t"] = cat.contiguous(), cat.t().contiguous()
        if self.long_center is not None and set(self.short_center) == set(self.trans):
            lens = [self.long_dim] + [int(k) for k in self.trans]
            if len(lens) > _lib.TwdhStreams.MAX:
                raise ValueError("TwDH: %d code lengths (at most %d)" % (len(lens), _lib.TwdhStreams.MAX))
            centres = [_check_center(self.long_center, "long_center")] + [_check_center(self.short_center[k], "short_center") for k in self.trans]
            for cen, n in zip(centres, lens):
                if cen.shape != (centres[0].shape[0], n):
                    raise ValueError("TwDH long_center / short_center: a centre of shape %s where [%d, %d] is expected"
                                     % (tuple(cen.shape), centres[0].shape[0], n))
            c["centres"] = torch.cat(centres, 1).to(torch.int8).to(device).contiguous()
            st = _lib.TwdhStreams()
            st.n = len(lens)
            at = 0
            for i, n in enumerate(lens):
                st.bit[i], st.K[i] = at, n
                at += n
            c["streams"], c["ktot"] = st, at
        self._train_cache = c
        return c

    def _short_train(self, long_hash):
        """the short codes of one modality with a graph: {key: view [B, 2*short] of one [B, 2S] matrix}"""
        if not self.trans:
            return {}
        if not long_hash.is_cuda:
            raise RuntimeError("TwDH's training path needs CUDA/HIP tensors (got %s); there is no CPU fallback" % long_hash.device)
        c = self._constants(long_hash.device)
        if torch.is_grad_enabled() and long_hash.requires_grad:
            p = _ShortCodes.apply(long_hash, c["trans"], c["trans_t"])
        else:
            p = _short_forward(long_hash, c["trans_t"])[0]
        out, at = {}, 0
        for k in self.trans:
            out[k] = p[:, at:at + 2 * int(k)]
            at += 2 * int(k)
        return out

    def forward_train(self, image, text):
        raise NotImplementedError("TwDH.forward_train(image, text) returns a pair of codes, and TwDH's step needs four (the long code and "
                                  "its short codes, per modality): forward_train_codes(image, text) is the differentiable forward")

    def forward_train_codes(self, image, text):
        """(img_long, img_short, txt_long, txt_short) of the reference's ``model(image, text)`` in train mode (:116-123), with a graph
        through the short-code transforms, the hash layer (``self.hash`` in .train() mode) and both towers (encode_image_train /
        encode_text_train): gradients reach every parameter with requires_grad.  The transforms and centres are constants."""
        img_long = self.hash.encode_img(self.backbone.encode_image_train(image))
        txt_long = self.hash.encode_txt(self.backbone.encode_text_train(text))
        return img_long, self._short_train(img_long), txt_long, self._short_train(txt_long)

    def encode_image(self, image):
        long_hash = self.hash.encode_img(self.backbone.encode_image(image))
        return long_hash, self._short(long_hash)

    def encode_text(self, text):
        long_hash = self.hash.encode_txt(self.backbone.encode_text(text))
        return long_hash, self._short(long_hash)

    def soft_argmax_hash_loss(self, code):
        """reference :125-130 -- 1 - mean((2 code - 1)^2), a 0-dim fp32 device tensor, differentiable with respect to `code` as the
        reference's is (xmh_quant_loss / xmh_quant_loss_grad)"""
        need_cuda(code)
        return _Quant.apply(code)

    def draw_ties(self):
        """the reference's random_center of one compute_loss (:196), by its own call and in its order -- the long centre, then the
        short centres in key order -- so that a seeded run consumes the CPU generator as the reference does: {key: +-1 fp32}"""
        ties = {"long": torch.randint_like(self.long_center[0], 2)}
        for k, v in self.short_center.items():
            ties[k] = torch.randint_like(v[0], 2)
        return {k: t * 2 - 1 for k, t in ties.items()}

    def hash_targets(self, labels, device, ties=None):
        """the target bits of all streams, packed [B, ceil(K_tot / 32)] int32 on the device (xmh_twdh_targets); `ties` overrides
        the draw (tests replay stored ones).  A label is set where it equals 1, as in the reference (:198)."""
        self._require_centres()
        c = self._constants(device)
        labels = torch.as_tensor(labels)
        if labels.dim() != 2 or labels.shape[1] > c["centres"].shape[0]:
            raise ValueError("TwDH loss: labels %s for hash centres of %d classes" % (tuple(labels.shape), c["centres"].shape[0]))
        ties = self.draw_ties() if ties is None else ties
        tie = torch.cat([ties["long"].reshape(-1)] + [ties[k].reshape(-1) for k in self.trans]).to(torch.int8)
        if tie.numel() != c["ktot"]:
            raise ValueError("TwDH loss: %d tie entries for %d target bits" % (tie.numel(), c["ktot"]))
        # pinned staging: the copy is queued on the stream and the host goes on (from pageable memory it would wait for it)
        tie = (tie if tie.is_cuda else tie.pin_memory()).to(device, non_blocking=True)
        lab = R.pack_labels((labels == 1).to(torch.uint8).to(device))             # the reference tests `label == 1` (:198)
        B = labels.shape[0]
        targets = torch.empty(B, (c["ktot"] + 31) // 32, dtype=torch.int32, device=device)
        check(lib.xmh_twdh_targets(ptr(lab), labels.shape[1], ptr(c["centres"]), ptr(tie), B, c["ktot"], ptr(targets), current_stream()),
              "xmh_twdh_targets")
        return targets

    def _require_centres(self):
        if self.long_center is None or not self.short_center and self.trans:
            raise ValueError("TwDH loss: no hash centres -- the config keys long_center (a directory with <long_dim>.pkl) and short_center "
                             "(a file or a directory of <short>.pkl) must name existing files, or be 'synthetic'")
        if set(self.short_center) != set(self.trans):
            raise ValueError("TwDH loss: short_center has the code lengths %s and trans_matrix %s; the two config keys must name the same lengths"
                             % (sorted(self.short_center), sorted(self.trans)))

    def transform_fidelity(self):
        """{key: (n_wrong, wrong [C, short] bool)} of every loaded transform against the loaded centres: the class / bit pairs at
        which the transform does not turn the long centre into the short one (twdh_transform.transform_fidelity; a lossless
        transform has n_wrong == 0).  A query: nothing is checked at load time."""
        from .twdh_transform import transform_fidelity
        self._require_centres()
        return {k: transform_fidelity(self.long_center, self.short_center[k], v) for k, v in self.trans.items()}

    def compute_loss(self, long_img_hash, long_txt_hash, short_img_hash, short_txt_hash, labels, indexs, ties=None, **kwags):
        """reference :132-184 -- (loss, loss_dict).  `loss` is a 0-dim fp32 device tensor, differentiable with respect to the two
        long codes and every short code; loss_dict has the reference's nested keys, its values detached 0-dim slices of the kernel's
        output."""
        self._require_centres()
        keys = list(self.trans)
        if set(short_img_hash) != set(keys) or set(short_txt_hash) != set(keys):
            raise ValueError("TwDH loss: short codes %s / %s for the lengths %s" % (sorted(short_img_hash), sorted(short_txt_hash), sorted(keys)))
        B = long_img_hash.shape[0]
        xs = [long_img_hash, long_txt_hash] + [short_img_hash[k] for k in keys] + [short_txt_hash[k] for k in keys]
        want = [2 * self.long_dim] * 2 + [2 * int(k) for k in keys] * 2
        for t, w in zip(xs, want):
            need_cuda(t)
            if t.dim() != 2 or tuple(t.shape) != (B, w):
                raise ValueError("TwDH loss: a code of shape %s where [%d, %d] is expected" % (tuple(t.shape), B, w))
        if torch.as_tensor(labels).shape[0] != B:
            raise ValueError("TwDH loss: %d label rows for a batch of %d" % (torch.as_tensor(labels).shape[0], B))
        dev = long_img_hash.device
        targets = self.hash_targets(labels, dev, ties)
        out = _Objective.apply(self, targets, len(keys), *xs)
        v, n = out.detach(), 1 + len(keys)
        loss_dict = {"All loss": v[0],
                     "Long": {"NCE": {"image": v[1], "text": v[1 + 2 * n]}, "Quan": {"image": v[2], "text": v[2 + 2 * n]}},
                     "Short": {k: {"NCE": v[1 + 4 * n + 2 * (i + 1)], "Quan": v[2 + 4 * n + 2 * (i + 1)]} for i, k in enumerate(keys)}}
        return out[0], loss_dict

    def object_function(self, long_img_hash, long_txt_hash, short_img_hash, short_txt_hash, labels=None, indexs=None, **kwags):
        """reference :186-190 -- without labels every sample is its own class"""
        if labels is None:
            labels = torch.ones([long_img_hash.shape[0]], dtype=torch.int).diag()
        return self.compute_loss(long_img_hash, long_txt_hash, short_img_hash, short_txt_hash, labels, indexs, **kwags)

    @classmethod
    def from_config(cls, cfg, output_dim=16, train_num=10000):
        long_dim = cfg.get("long_dim", 512)
        trans = cfg.get("trans_matrix", "./data/transformer/TwDH/center/trans")
        if trans != "synthetic":
            trans = os.path.join(trans, str(long_dim))
        long_center = cfg.get("long_center", "./data/transformer/TwDH/center/long")
        if long_center != "synthetic":
            long_center = os.path.join(long_center, str(long_dim) + ".pkl")
        return cls(cfg=cfg, long_dim=long_dim, short_dim=output_dim, clipPath=cfg.get("clip_path", "./ViT-B-32.pt"), train_num=train_num,
                   hash_func=cfg.get("hash_func", "softmax"), trans=trans, short_dims=cfg.get("short_dims", None),
                   quan_alpha=cfg.get("quan_alpha", 0.5), low_rate=cfg.get("low_rate", 0), long_center=long_center,
                   short_center=cfg.get("short_center", "./data/transformer/TwDH/center/short"), num_classes=cfg.get("num_classes", 80))


def _short_forward(long_hash, trans_t):
    """xmh_twdh_short_forward -> (p_short [B, 2S], the long code as the kernel read it)"""
    x = long_hash.detach().float().contiguous()
    S2, L2 = trans_t.shape
    if x.dim() != 2 or x.shape[1] != L2:
        raise ValueError("TwDH short codes: a long code of shape %s for transforms of %d rows" % (tuple(x.shape), L2))
    p = torch.empty(x.shape[0], S2, dtype=torch.float32, device=x.device)
    check(lib.xmh_twdh_short_forward(ptr(x), ptr(trans_t), x.shape[0], L2, S2, ptr(p), current_stream()), "xmh_twdh_short_forward")
    return p, x


class _Quant(torch.autograd.Function):
    """forward = xmh_quant_loss, backward = xmh_quant_loss_grad (-4 (2 code - 1) / n times the upstream, read on the device)"""

    @staticmethod
    def forward(ctx, code):
        c = code.detach().float().contiguous()
        out = torch.empty(1, dtype=torch.float64, device=c.device)
        check(lib.xmh_quant_loss(ptr(c), c.numel(), ptr(out), current_stream()), "xmh_quant_loss")
        ctx.meta = (code.shape, code.dtype)
        ctx.save_for_backward(c)
        return out.float().reshape(())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        c, = ctx.saved_tensors
        up = g.detach().float().reshape(1).contiguous()
        grad = torch.empty_like(c)
        check(lib.xmh_quant_loss_grad(ptr(c), c.numel(), 1.0, ptr(up), ptr(grad), 0, current_stream()), "xmh_quant_loss_grad")
        return grad.reshape(ctx.meta[0]).to(ctx.meta[1])


class _ShortCodes(torch.autograd.Function):
    """forward = xmh_twdh_short_forward (pair_softmax(long . T_cat)), backward = xmh_twdh_short_backward; the transforms are
    constants and get no gradient"""

    @staticmethod
    def forward(ctx, long_hash, trans, trans_t):
        p, _ = _short_forward(long_hash, trans_t)
        ctx.meta = (long_hash.shape, long_hash.dtype)
        ctx.save_for_backward(p, trans)                 # p is the output: autograd notices if the caller writes into it
        return p

    @staticmethod
    @torch.autograd.function.once_differentiable      # the gradient kernels are not themselves differentiable
    def backward(ctx, g):
        p, trans = ctx.saved_tensors
        B, S2 = p.shape
        L2 = trans.shape[0]
        g = g.detach().float().contiguous()
        gl = torch.empty(B, L2, dtype=torch.float32, device=p.device)
        ws = _lib.workspace(B * S2 * 4, p.device)
        check(lib.xmh_twdh_short_backward(ptr(g), ptr(p), ptr(trans), B, L2, S2, ptr(gl), 0, ptr(ws), ws.numel(), current_stream()),
              "xmh_twdh_short_backward")
        return gl.reshape(ctx.meta[0]).to(ctx.meta[1]), None, None


def _side_by_side(ts):
    """the short codes of one modality as one contiguous [B, 2S] matrix: the matrix they are views of when they are the slices
    _short_train hands out (no copy), else their concatenation"""
    B, S2 = ts[0].shape[0], sum(t.shape[1] for t in ts)
    at = ts[0].storage_offset()
    same = all(t.dtype == torch.float32 and t.untyped_storage().data_ptr() == ts[0].untyped_storage().data_ptr() for t in ts)
    for t in ts:
        same = same and t.stride() == (S2, 1) and t.storage_offset() == at
        at += t.shape[1]
    if same:
        return ts[0].detach().as_strided((B, S2), (S2, 1), ts[0].storage_offset())
    return torch.cat([t.detach().float() for t in ts], 1).contiguous()


class _Objective(torch.autograd.Function):
    """forward = xmh_twdh_loss -> fp32 [1 + 6 n] (element 0 the loss, then xmh_twdh_loss's layout), backward = xmh_twdh_loss_grad,
    one call per modality that needs a gradient.  inputs: long image, long text, the n - 1 short image codes, the n - 1 short text
    codes.  With low_rate == 0 the short codes get no gradient (an exact zero) and their kernel work is skipped."""

    @staticmethod
    def forward(ctx, model, targets, ns, *inputs):
        c = model._constants(targets.device)
        B = inputs[0].shape[0]
        longs = [inputs[m].detach().float().contiguous() for m in range(2)]
        shorts = [_side_by_side(inputs[2 + m * ns:2 + (m + 1) * ns]) if ns else None for m in range(2)]
        n = 1 + ns
        out = torch.empty(1 + 6 * n, dtype=torch.float64, device=targets.device)
        nbytes = lib.xmh_twdh_loss_ws_bytes(B, n)
        ws = _lib.workspace(nbytes, targets.device)
        check(lib.xmh_twdh_loss(ctypes.byref(c["streams"]), ptr(longs[0]), ptr(shorts[0]), ptr(longs[1]), ptr(shorts[1]), ptr(targets), B,
                                float(model.quan_alpha), float(model.low_rate), ptr(out), ptr(ws), nbytes, current_stream()), "xmh_twdh_loss")
        ctx.streams, ctx.ns = c["streams"], ns
        ctx.weights = (float(model.quan_alpha), float(model.low_rate))
        ctx.meta = [(t.shape, t.dtype) for t in inputs]
        ctx.has_short = ns > 0
        ctx.save_for_backward(targets, longs[0], longs[1], *([shorts[0], shorts[1]] if ns else []))
        return out.float()

    @staticmethod
    @torch.autograd.function.once_differentiable      # the gradient kernel is not itself differentiable: fail loudly on double backward
    def backward(ctx, g):
        targets, *saved = ctx.saved_tensors
        longs, shorts = saved[:2], (saved[2:] if ctx.has_short else [None, None])
        need, ns = ctx.needs_input_grad[3:], ctx.ns
        qa, lr = ctx.weights
        up = g.detach().float()[:1].contiguous()      # only element 0 (the loss) carries a gradient
        B = longs[0].shape[0]
        grads = [None] * (2 + 2 * ns)
        for m in range(2):
            short_need = need[2 + m * ns:2 + (m + 1) * ns]
            d_long = torch.empty_like(longs[m]) if need[m] else None
            d_short = torch.empty_like(shorts[m]) if ns and any(short_need) and lr != 0.0 else None
            if d_long is None and d_short is None:
                continue
            check(lib.xmh_twdh_loss_grad(ctypes.byref(ctx.streams), ptr(longs[m]), ptr(shorts[m]), ptr(targets), B, qa, lr, ptr(up), ptr(d_long),
                                         ptr(d_short), current_stream()), "xmh_twdh_loss_grad")
            if d_long is not None:
                grads[m] = d_long.reshape(ctx.meta[m][0]).to(ctx.meta[m][1])
            at = 0
            for i in range(ns):
                j = 2 + m * ns + i
                w = ctx.meta[j][0][1]
                if d_short is not None and short_need[i]:
                    grads[j] = d_short[:, at:at + w].to(ctx.meta[j][1])
                at += w
        return (None, None, None, *grads)
