"""Per-method runners registered under the reference's names (runners/<METHOD>/runner.py).

``from_config(rank, world_size, distributed, cfg, logger)`` keeps the positional order mp.spawn relies on
(main.py:44-49, runners/DCMHT/runner.py:40-80); like in the reference, constructing a runner builds dataset and
model and then calls ``run()``."""
from __future__ import annotations

import os

import torch

from .. import retrieval as R
from .. import towers
from ..common.register import registry
from .base import BaseTrainer


class _MethodTrainer(BaseTrainer):
    """What a method declares, as data: MODEL_ARCH; LOSS_INPUTS, the keyword names of its objective's inputs in the order compute_loss
    takes them; BITS_FROM, the one of them whose last extent over ``hash_scale`` is the code length of the display line; FORWARD, the
    model's train-forward method, FORWARD_MASK whether it takes the key padding mask, and FORWARD_OUTPUTS, the keyword names of its
    outputs in its own order (None: they go to compute_loss positionally); LOSS_OPTIONAL, the inputs a caller may leave out (None then)."""
    LOSS_INPUTS = ("img_hash", "txt_hash")
    LOSS_OPTIONAL = ()
    BITS_FROM = "img_hash"
    FORWARD, FORWARD_MASK, FORWARD_OUTPUTS = "forward_train", False, LOSS_INPUTS

    def __init__(self, cfg, is_train=True, logger=None, device=None, world_size=torch.cuda.device_count(), output_dim=16,
                 train_num=10000, query_num=5000, epochs=100, save_dir="./result", batch_size=128, num_workers=4, pin_memory=True,
                 shuffle=True, display_step=20, top_k=5000, model_state="", distributed=False, autorun=True, **kwags):
        super().__init__(cfg=cfg, is_train=is_train, logger=logger, device=device, output_dim=output_dim, train_num=train_num,
                         distributed=distributed, query_num=query_num, epochs=epochs, save_dir=save_dir, display_step=display_step,
                         top_k=top_k, model_state=model_state, batch_size=batch_size, world_size=world_size)
        self.build_dataset(cfg.dataset, train_num=train_num, query_num=query_num, batch_size=batch_size, num_workers=num_workers,
                           pin_memory=pin_memory, shuffle=shuffle)
        self.build_model(cfg.model, output_dim=output_dim)
        if autorun:
            self.run()

    @classmethod
    def from_config(cls, rank=0, world_size=torch.cuda.device_count(), distributed=False, cfg=None, logger=None, **extra):
        assert cfg is not None, "config is None!"
        run = cfg.run
        return cls(cfg, is_train=run.get("is_train", False), logger=logger, device=rank if distributed else run.get("device", 0),
                   output_dim=run.get("output_dim", 16), train_num=run.get("train_num", 10000), query_num=run.get("query_num", 5000),
                   epochs=run.get("epochs", 10), save_dir=run.get("save_dir", "./result"), batch_size=run.get("batch_size", 128),
                   num_workers=run.get("num_workers", 4), pin_memory=run.get("pin_memory", True), shuffle=run.get("shuffle", True),
                   model_state=run.get("resume_model", ""), display_step=run.get("display_step", 20), top_k=run.get("top_k", None),
                   world_size=world_size, distributed=distributed, **extra)

    def build_model(self, cfg_model, output_dim=16, **kwags):
        """the base class's, and with distributed=True every BatchNorm head takes its batch statistics over all ranks:
        what the reference gets from nn.SyncBatchNorm.convert_sync_batchnorm (runners/base.py:111)"""
        super().build_model(cfg_model, output_dim=output_dim, **kwags)
        if self.distributed:
            from torch import distributed as dist
            for head in _sync_heads(self.model):
                head.sync_group = dist.group.WORLD

    def loss_extras(self, inputs, label):
        """further keywords of the model's object_function, made from the batch (MITH: label_sim)"""
        return {}

    def compute_loss(self, *args, label=None, index=None, epoch=0, times=0, global_step=0, **kwags):
        """The objective of one batch, the reference's compute_loss of every runner (the lines are with each class): LOSS_INPUTS
        positionally or by keyword, handed to the model's object_function.  The returned loss is differentiable with respect to what
        the class names.  The display line needs the training loop's loader and optimiser and is skipped without them."""
        inputs = dict(zip(self.LOSS_INPUTS, args))
        rest = self.LOSS_INPUTS[len(args):]
        missing = [n for n in rest if n not in kwags and n not in self.LOSS_OPTIONAL]
        if missing or len(args) > len(self.LOSS_INPUTS):
            raise TypeError("%s.compute_loss takes %s (missing: %s)" % (type(self).__name__, ", ".join(self.LOSS_INPUTS), ", ".join(missing) or "none"))
        inputs.update((n, kwags.pop(n, None)) for n in rest)
        all_loss, loss_dict = self.model.object_function(**inputs, labels=label, indexs=index, **self.loss_extras(inputs, label), **kwags)
        if global_step % self.display_step == 0 and getattr(self, "train_loader", None) is not None and getattr(self, "optimizer", None) is not None:
            self.print_loss_dict(loss_dict, bits=inputs[self.BITS_FROM].shape[-1] // self.hash_scale, epoch=epoch, times=times)
        return all_loss


def _step(trainer, image, text, key_padding_mask, label, index, epoch, times):
    """one batch: the outputs of the model's train-forward (trainer.FORWARD) into the objective (trainer.FORWARD_OUTPUTS).  DCMHT /
    DSPH: the two codes; MITH (runners/MITH/runner.py:109-115): the eight outputs of the head over both towers, the text tower with
    the key padding mask; TwDH (runners/TwDH/runner.py:129-130): the long code and the short codes of both modalities; DNPH
    (runners/DNPH/runner.py:126-127): the code and the class logits; DIMCH (runners/DIMCH/runner.py:132-133): the token embeddings
    and the codes."""
    forward = getattr(trainer.model, trainer.FORWARD)
    out = forward(image, text, key_padding_mask=key_padding_mask) if trainer.FORWARD_MASK else forward(image, text)
    args, names = (out, ()) if trainer.FORWARD_OUTPUTS is None else ((), trainer.FORWARD_OUTPUTS)
    return trainer.compute_loss(*args, **dict(zip(names, out)), label=label, index=index, epoch=epoch, times=times,
                                global_step=trainer.global_step)


# why an epoch does not run with distributed=True although the all-reduce of the gradients (xmh/ddp.py) exists
_NO_DDP_STATE = ("%s is per-rank state that DistributedDataParallel reconciles by a per-forward buffer broadcast beside the all-reduce "
                 "of the gradients; the buffer broadcast is not built")
_NO_DDP_UNCHECKED = ("the all-reduce of the gradients (xmh/ddp.py) is built and checked for the epochs of DCMHT and DSPH; this method's "
                     "distributed step has no float64 restatement yet")


def _sync_heads(model):
    """the BatchNorm heads of a model: the modules whose batch statistics must span the ranks of a distributed step"""
    from ..models.heads import DCMHTModalityHash
    return [m for m in model.modules() if isinstance(m, DCMHTModalityHash) and isinstance(m.norm, torch.nn.BatchNorm1d)]


def _no_ddp_local_batchnorm(trainer):
    """DCMHT: a reason unless every BatchNorm head of the model has its process group (build_model gives it with distributed=True)"""
    model = getattr(trainer, "model", None)
    if model is not None and all(m.sync_group is not None for m in _sync_heads(model)):
        return None
    return ("the image head's BatchNorm has no process group (build_model sets sync_group; the reference converts to SyncBatchNorm): "
            "its statistics would be the local batch's, and the all-reduce of the gradients would average gradients of different functions")


def _train_epoch(trainer, epoch: int, step=_step, no_ddp=None):
    """runners/DCMHT/runner.py:107-128 and runners/DSPH/runner.py:104-127 (the latter also steps the proxies' optimiser); with MITH's
    declaration, runners/MITH/runner.py:98-123.  `step(trainer, image, text, key_padding_mask, label, index, epoch, times)`
    returns the loss of one batch.  The optimiser is built on the first call, when the instance has none yet.  A batch of raw
    photos (uint8, stacked or a list of different sizes: the file layout's training split) goes through the GPU training
    transform; a float batch goes on as it is.

    distributed=True: every rank runs its share of the batch (build_loader's DistributedSampler, the same number of
    steps on every rank), and between ``loss.backward()`` and the optimisers' steps the GradReducer averages every gradient of
    ``model.parameters()`` -- DSPH's proxies among them -- over the ranks in one collective.  The reducer is built with the optimiser
    on the first call and rank 0's parameters are broadcast once.  Each rank logs its own loss, as in the reference.  `no_ddp`: the
    reason why the calling method's epoch does not run distributed, or a function of the trainer that gives it (None: it does)."""
    if trainer.distributed:
        reason = no_ddp(trainer) if callable(no_ddp) else no_ddp
        if reason is not None:
            raise NotImplementedError("train_epoch with distributed=True: " + reason)
    if getattr(trainer, "optimizer", None) is None:
        built = trainer.build_optimizer(trainer.cfg.get("optimizer"))
        trainer.optimizer, trainer.lr_schedu = built[0], built[-1]
        trainer.optimizer_loss = built[1] if len(built) == 3 else None
    optimizer_loss = getattr(trainer, "optimizer_loss", None)      # DSPH: the proxies' own optimiser
    trainer.change_state(mode="train")
    reducer = None
    if trainer.distributed:
        reducer = getattr(trainer, "reducer", None)
        if reducer is None:                                        # after change_state: requires_grad is what training sees
            from ..ddp import GradReducer
            reducer = trainer.reducer = GradReducer(trainer.model, trainer.world_size)
            reducer.broadcast_parameters()
    trainer.logger.info(">>>>>> epochs: %d/%d" % (epoch, trainer.epochs))
    all_loss = 0
    times = 0
    for image, text, key_padding_mask, label, index in trainer.train_loader:
        trainer.global_step += 1
        times += 1
        if isinstance(image, (list, tuple)) or image.dtype == torch.uint8:      # raw RGB bytes: the training transform runs on the GPU
            image = trainer._train_image_transform()(image)                     # (dataset/transformer_dataset.py:34-40, Pillow-exact)
        else:
            image = image.to(trainer.device, non_blocking=True)
        text = text.to(trainer.device, non_blocking=True)
        index = index.numpy()
        loss = step(trainer, image, text, key_padding_mask, label, index, epoch, times)
        all_loss += loss.detach()
        trainer.optimizer.zero_grad()
        if optimizer_loss is not None:
            optimizer_loss.zero_grad()
        loss.backward()
        if reducer is not None:
            reducer.reduce()
        trainer.optimizer.step()
        if optimizer_loss is not None:
            optimizer_loss.step()
    rates = "-".join("%.9f" % r for r in sorted(set(trainer.optimizer.get_lr())))
    trainer.logger.info(f">>>>>> [{epoch}/{trainer.epochs}] loss: {all_loss / len(trainer.train_loader)}, lr: {rates}")


@registry.register_runner("DCMHTTrainer")
class DCMHTTrainer(_MethodTrainer):
    """runners/DCMHT/runner.py: the model emits 2K pair probabilities; bit j = +1 iff p[j,1] > p[j,0] (:82-95).
    compute_loss (:97-105): differentiable with respect to img_hash / txt_hash (xmh_loss.hip behind torch.autograd), and through them
    -- when they come from `model.hash` in .train() mode -- with respect to every parameter of the heads (xmh_head_grad.hip)."""

    MODEL_ARCH = "DCMHT"

    def __init__(self, cfg, *a, **k):
        self.hash_func = cfg.model.get("hash_func", "softmax")
        assert self.hash_func == "softmax", "DCMHT must adopt the 'softmax' hash technique."
        self.hash_scale = 2
        self.loss_type = k.get("loss_type", "l1")               # runners/DCMHT/runner.py:26-30: only named in the display line
        super().__init__(cfg, *a, **k)

    @classmethod
    def make_hash_code(cls, code):
        if isinstance(code, list):
            code = torch.stack(code).permute(1, 0, 2)
        return R.pack_pair_argmax(code.reshape(code.shape[0], -1)).unpack()

    @classmethod
    def pack_hash_code(cls, code, out, row_index, flags):
        R.pack_pair_argmax(code.reshape(code.shape[0], -1), out=out, row_index=row_index)

    def train_epoch(self, epoch: int):
        """runners/DCMHT/runner.py:107-128"""
        _train_epoch(self, epoch, no_ddp=_no_ddp_local_batchnorm)


@registry.register_runner("DSPHTrainer")
class DSPHTrainer(_MethodTrainer):
    """runners/DSPH/runner.py: base generate_hash + sign quantiser.  compute_loss (:93-101): the HyP objective (xmh_hyp.hip behind
    torch.autograd), differentiable with respect to img_hash / txt_hash and the model's hyp.proxies."""

    MODEL_ARCH = "DSPH"
    hash_scale = 1                                              # runners/DSPH/runner.py:38
    loss_type = "l1"                                            # runners/DSPH/runner.py:27-31: only named in the display line

    def build_optimizer(self, cfg_optimizer=None, parameters=None):
        """runners/DSPH/runner.py:83-91: BertAdam as in the base class, and a stock SGD over the HyP proxies from the config's
        ``hyp`` sub-section -> (optimizer, optimizer_loss, None)"""
        optimizer, lr_schedu = super().build_optimizer(cfg_optimizer=cfg_optimizer, parameters=parameters)
        hyp = (cfg_optimizer.get("hyp") if cfg_optimizer is not None else None) or {}
        optimizer_loss = torch.optim.SGD(params=self.model.hyp.parameters(), lr=hyp.get("lr", 0.02), momentum=hyp.get("momentum", 0.9),
                                         weight_decay=hyp.get("weight_decay", 0.0005))
        self.logger.info("Building optimizer!")
        return optimizer, optimizer_loss, lr_schedu

    def train_epoch(self, epoch: int):
        """runners/DSPH/runner.py:104-127: as DCMHT's, and the proxies' SGD steps beside BertAdam"""
        _train_epoch(self, epoch)


@registry.register_runner("MITHTrainer")
class MITHTrainer(_MethodTrainer):
    """runners/MITH/runner.py:125-131: code = sign(cls_hash + tokens_hash); the text tower gets the padding mask.  compute_loss
    (:84-96): the objective of xmh_mith_loss.hip behind torch.autograd, differentiable with respect to the eight head outputs."""

    MODEL_ARCH = "MITH"
    LOSS_INPUTS = ("res_img_cls", "img_cls_hash", "tokens_hash_i", "trans_tokens_i", "res_txt_cls", "txt_cls_hash", "tokens_hash_t",
                   "trans_tokens_t")
    BITS_FROM = "img_cls_hash"
    FORWARD, FORWARD_MASK, FORWARD_OUTPUTS = "forward_train_towers", True, None
    EPOCH = "train_epoch_towers"
    train = BaseTrainer.train                                   # the one loop, entered in this class too: train() is MITH's own entry point
    hash_scale = 1                                              # runners/MITH/runner.py:39
    loss_type = "l1"                                            # runners/MITH/runner.py:28-32: only named in the display line

    def loss_extras(self, inputs, label):
        """label_sim = calc_label_sim(train_labels, label), [train_num, B], formed on the codes' device, with the packed train labels
        kept there between calls"""
        dev = inputs["img_cls_hash"].device
        cached = getattr(self, "_train_lab", None)
        if cached is None or cached[0] is not self.train_labels or cached[1] != dev:
            tl = torch.as_tensor(self.train_labels)
            cached = self._train_lab = (self.train_labels, dev, R.pack_labels(tl.to(dev)), tl.shape[1])
        return {"label_sim": R.label_sim(cached[2], R.pack_labels(torch.as_tensor(label).to(dev)), cached[3])}

    def train_epoch(self, epoch: int):
        raise NotImplementedError("MITHTrainer.train_epoch: the epoch that trains MITH's head and both towers, the reference's, is "
                                  "train_epoch_towers (train() runs it); over a frozen backbone the head trains through "
                                  "MITH.forward_train_heads with compute_loss and build_optimizer")

    def train_epoch_towers(self, epoch: int):
        """runners/MITH/runner.py:98-123: the backbone at backbone_lr and the head at lr, the text tower with the key padding mask"""
        _train_epoch(self, epoch, no_ddp=_NO_DDP_STATE % "MITH's feature bank")

    def generate_hash(self, image, text, key_padding_mask=None):
        _, img_cls_hash, tokens_hash_i, _, _, txt_cls_hash, tokens_hash_t, _ = self.model(image, text, key_padding_mask=key_padding_mask)
        return img_cls_hash + tokens_hash_i, txt_cls_hash + tokens_hash_t


@registry.register_runner("TwDHTrainer")
class TwDHTrainer(DCMHTTrainer):
    """runners/TwDH/runner.py: one forward yields the long code and every short code (:138-143); evaluation reports the four
    mAPs per code length (:181-228).  Code streams: "long" (long_dim bits) and one per short length, all quantised by the
    DCMHT pair-argmax (:82-95 of the DCMHT runner, inherited).  compute_loss (:106-114): the objective of xmh_twdh.hip behind
    torch.autograd, differentiable with respect to the long codes and every short code."""

    MODEL_ARCH = "TwDH"
    LOSS_INPUTS = ("long_img_hash", "long_txt_hash", "short_img_hash", "short_txt_hash")
    BITS_FROM = "long_img_hash"
    FORWARD, FORWARD_OUTPUTS = "forward_train_codes", ("long_img_hash", "short_img_hash", "long_txt_hash", "short_txt_hash")
    EPOCH = "train_epoch_codes"

    def __init__(self, cfg, *a, **k):
        self.long_dim = cfg.model.get("long_dim", 512)
        self.max_short, self.best_epoch_short = {}, {}
        super().__init__(cfg, *a, **k)

    def train_epoch(self, epoch: int):
        raise NotImplementedError("TwDHTrainer.train_epoch: TwDH's head yields the long code and its short codes, four outputs where "
                                  "the shared epoch expects a pair; the reference's epoch is train_epoch_codes (train() runs it)")

    def train_epoch_codes(self, epoch: int):
        """runners/TwDH/runner.py:116-137: one BertAdam over the backbone and the hash layer; the transforms and centres are constants"""
        _train_epoch(self, epoch, no_ddp=_NO_DDP_UNCHECKED)

    def build_model(self, cfg_model, output_dim=16):
        super().build_model(cfg_model, output_dim=output_dim)
        for item in self.model.get_short_dims():
            self.max_short[str(item)] = {"i2t": 0, "t2i": 0}
            self.best_epoch_short[str(item)] = {"i2t": 0, "t2i": 0}

    def generate_hash(self, image, text, key_padding_mask=None):
        (long_image_hash, short_image_hash), (long_text_hash, short_text_hash) = towers.run_both(
            lambda: self.model.encode_image(image), lambda: self.model.encode_text(text))
        return long_image_hash, short_image_hash, long_text_hash, short_text_hash

    def generate_hashes(self, image, text, key_padding_mask=None):
        li, si, lt, st = self.generate_hash(image, text, key_padding_mask)
        out = {"long": (li, lt)}
        for key in si:
            out[key] = (si[key], st[key])
        return out

    def code_streams(self):
        dims = {"long": self.long_dim}
        for d in self.model.get_short_dims():
            dims[str(d)] = int(d)
        return dims

    def encode_shard(self, data_loader, length):
        return self.encode_streams(data_loader, length)["long"]

    def get_code(self, data_loader, length):
        """reference :145-179 -- (long_img, long_txt, {short: img}, {short: txt}) fp32 +-1 buffers, complete on every rank."""
        streams = self.encode_streams(data_loader, length)
        full = {n: (self._gather_packed(i, length).unpack(), self._gather_packed(t, length).unpack()) for n, (i, t) in streams.items()}
        return (full["long"][0], full["long"][1], {n: v[0] for n, v in full.items() if n != "long"},
                {n: v[1] for n, v in full.items() if n != "long"})

    def _evaluate_streams(self, k):
        self._qlab = self._rlab = None
        qs = self.encode_streams(self.query_loader, self.query_num)
        rs = self.encode_streams(self.retrieval_loader, self.retrieval_num)
        out = {}
        for name in qs:
            q_img, q_txt = self._gather_packed(qs[name][0], self.query_num), self._gather_packed(qs[name][1], self.query_num)
            r_img, r_txt = rs[name]
            maps = (self._map(q_img, r_txt, k), self._map(q_txt, r_img, k), self._map(q_img, r_img, k), self._map(q_txt, r_txt, k))
            out[name] = (maps, (q_img, q_txt, r_img, r_txt))
        return out

    def valid(self, epoch, k=None):
        assert self.query_loader is not None and self.retrieval_loader is not None
        save_dir = os.path.join(self.save_dir, "mat_files")
        os.makedirs(save_dir, exist_ok=True)
        self.logger.info("Valid.")
        results = self._evaluate_streams(k)
        for name, ((mAPi2t, mAPt2i, mAPi2i, mAPt2t), codes) in results.items():
            bits = codes[0].K
            if name == "long":                                   # reference valid_each, short is None (:194-208)
                if self.max_mapi2t < mAPi2t:
                    self.best_epoch_i = epoch
                    self._save_codes(codes, os.path.join(save_dir, "i2t-long.mat"))
                    if self._is_writer():
                        self.save_model(save_dir=self.save_dir, epoch=epoch)
                self.max_mapi2t = max(self.max_mapi2t, mAPi2t)
                if self.max_mapt2i < mAPt2i:
                    self.best_epoch_t = epoch
                    self._save_codes(codes, os.path.join(save_dir, "t2i-long.mat"))
                    if self._is_writer():
                        self.save_model(save_dir=self.save_dir, epoch=epoch)
                self.max_mapt2i = max(self.max_mapt2i, mAPt2i)
                self.logger.info(f">>>>>> [{epoch}/{self.epochs}], Long, {bits} Bit, MAP(i->t): {mAPi2t}, MAP(t->i): {mAPt2i}, MAP(t->t): {mAPt2t}, "
                                 f"MAP(i->i): {mAPi2i}, MAX MAP(i->t): {self.max_mapi2t}, epoch: {self.best_epoch_i}, MAX MAP(t->i): {self.max_mapt2i}, "
                                 f"epoch: {self.best_epoch_t}")
            else:                                                # short codes (:209-228)
                if self.max_short[name]["i2t"] < mAPi2t:
                    self.best_epoch_short[name]["i2t"] = epoch
                    self._save_codes(codes, os.path.join(save_dir, f"i2t-short-{name}.mat"))
                self.max_short[name]["i2t"] = max(self.max_short[name]["i2t"], mAPi2t)
                if self.max_short[name]["t2i"] < mAPt2i:
                    self.best_epoch_short[name]["t2i"] = epoch
                    self._save_codes(codes, os.path.join(save_dir, f"t2i-short-{name}.mat"))
                self.max_short[name]["t2i"] = max(self.max_short[name]["t2i"], mAPt2i)
                self.logger.info(f">>>>>> [{epoch}/{self.epochs}], Short, {bits} Bit, MAP(i->t): {mAPi2t}, MAP(t->i): {mAPt2i}, MAP(t->t): {mAPt2t}, "
                                 f"MAP(i->i): {mAPi2i}, MAX MAP(i->t): {self.max_short[name]['i2t']}, epoch: {self.best_epoch_short[name]['i2t']}, "
                                 f"MAX MAP(t->i): {self.max_short[name]['t2i']}, epoch: {self.best_epoch_short[name]['t2i']}")
        return {name: maps for name, (maps, _) in results.items()}


@registry.register_runner("DNPHTrainer")
class DNPHTrainer(_MethodTrainer):
    """runners/DNPH/runner.py: the model's encoders return (code, class logits); evaluation quantises the code by its sign.
    compute_loss (:102-110): the objective of xmh_dnph.hip behind torch.autograd, differentiable with respect to the codes, the class
    logits and the model's loss.proxies."""

    MODEL_ARCH = "DNPH"
    LOSS_INPUTS = FORWARD_OUTPUTS = ("img_hash", "txt_hash", "img_pre", "txt_pre")
    hash_scale = 1                                              # runners/DNPH/runner.py:41
    loss_type = "l1"                                            # runners/DNPH/runner.py:30-34: only named in the display line

    def __init__(self, cfg, *a, **k):
        self.hash_func = cfg.model.get("hash_func", "tanh")
        assert self.hash_func == "tanh", "DNPH must adopt the 'tanh' hash technique."
        super().__init__(cfg, *a, **k)

    def build_optimizer(self, cfg_optimizer=None, parameters=None):
        """runners/DNPH/runner.py:86-92: BertAdam as in the base class, and a stock SGD over the loss's proxies at the rate of the
        config's ``loss`` sub-section -> (optimizer, optimizer_loss, None)"""
        optimizer, lr_schedu = super().build_optimizer(cfg_optimizer=cfg_optimizer, parameters=parameters)
        loss = (cfg_optimizer.get("loss") if cfg_optimizer is not None else None) or {}
        optimizer_loss = torch.optim.SGD(params=self.model.loss.parameters(), lr=loss.get("lr", 0.0001))
        self.logger.info("Building optimizer!")
        return optimizer, optimizer_loss, lr_schedu

    def train_epoch(self, epoch: int):
        """runners/DNPH/runner.py:113-136: the four outputs of the head over both towers into the objective; the proxies' SGD steps
        beside BertAdam"""
        _train_epoch(self, epoch, no_ddp=_NO_DDP_STATE % "DNPH's noise assignment")

    def generate_hash(self, image, text, key_padding_mask=None):
        """runners/DNPH/runner.py:138-141: the codes alone; the class logits are a training signal"""
        (image_hash, _), (text_hash, _) = towers.run_both(lambda: self.model.encode_image(image), lambda: self.model.encode_text(text))
        return image_hash, text_hash


@registry.register_runner("DIMCHTrainer")
class DIMCHTrainer(_MethodTrainer):
    """runners/DIMCH/runner.py: the model's encoders return (token embeddings, code); evaluation quantises the tanh code by its sign.
    With ``hash_func: softmax`` the code is 2K wide and the reference writes it into its K-wide buffer and fails (:147-149 with
    runners/base.py get_code); ``valid`` says so instead.  compute_loss (:109-117): the objective of xmh_dimch.hip behind
    torch.autograd, differentiable with respect to the token embeddings and the codes."""

    MODEL_ARCH = "DIMCH"
    LOSS_INPUTS = FORWARD_OUTPUTS = ("img_embeds", "img_hash", "txt_embeds", "txt_hash")
    BITS_FROM = "img_embeds"
    loss_type = "l1"                                            # runners/DIMCH/runner.py:33: only named in the display line

    def __init__(self, cfg, *a, **k):
        self.hash_func = cfg.model.get("hash_func", "softmax")
        self.hash_scale = 2 if self.hash_func == "softmax" else 1   # runners/DIMCH/runner.py:39-42
        super().__init__(cfg, *a, **k)

    def model_kwargs(self):
        """runners/DIMCH/runner.py:87-107: the text token count ``dataset.max_word`` handed on"""
        return {"txt_token_size": self.cfg.dataset.get("max_word", 32)}

    def train_epoch(self, epoch: int):
        """runners/DIMCH/runner.py:119-140"""
        _train_epoch(self, epoch, no_ddp=_NO_DDP_UNCHECKED)

    def merge_hash(self, image_embed, text_embed):
        """runners/DIMCH/runner.py:142-145"""
        return torch.sign((image_embed + text_embed).detach() / 2)

    def generate_hash(self, image, text, key_padding_mask=None):
        """runners/DIMCH/runner.py:147-149: the two codes; the token embeddings are a training signal"""
        _, image_hash, _, text_hash = self.model(image, text)
        return image_hash, text_hash

    def valid(self, epoch, k=None):
        if self.hash_func == "softmax":
            raise NotImplementedError("DIMCHTrainer.valid with hash_func: softmax: the code is %d wide for %d bits, and the reference "
                                      "writes it into its %d-wide buffer and fails; evaluation is built for hash_func: tanh"
                                      % (2 * self.output_dim, self.output_dim, self.output_dim))
        return super().valid(epoch, k=k)


@registry.register_runner("UMoEDTrainer")
class UMoEDTrainer(_MethodTrainer):
    """runners/UMoED/runner.py: the model's encoders return (token logits, code); evaluation reports four mAPs (i->t, t->i, i->i, t->t),
    keeps a best epoch for each and writes four .mat files with a fusion stream beside the usual keys.  The linear-subspace and tanh codes
    are quantised by their sign, the pair softmax by its argmax.  Training (:134-155) is ``train_epoch_decoder`` / ``train_decoder``, which
    ``run()`` enters with ``is_train: true``: the decoder head in train mode with its backward and both towers; ``train_epoch``
    and ``train()`` keep raising and name them.  compute_loss (:126-134): the objective of xmh_umoed.hip behind torch.autograd, differentiable with respect to the two logit tensors."""

    MODEL_ARCH = "UMoED"
    # the six outputs of the model's forward and of its forward_train
    LOSS_INPUTS = FORWARD_OUTPUTS = ("img_embeds", "img_hash", "txt_embeds", "txt_hash", "fusion_embeds", "fusion_hash")
    LOSS_OPTIONAL = ("fusion_embeds", "fusion_hash")
    BITS_FROM = "img_embeds"
    loss_type = "l1"                                            # runners/UMoED/runner.py:35: only named in the display line
    MAP_NAMES = ("i2t", "t2i", "i2i", "t2t")

    def __init__(self, cfg, *a, **k):
        if k.get("distributed", False):
            raise NotImplementedError("UMoEDTrainer with distributed=True: the four-mAP evaluation and its .mat files are built for one process")
        self.hash_func = cfg.model.get("hash_func", "softmax")
        self.hash_scale = 2 if self.hash_func == "softmax" else 1   # runners/UMoED/runner.py:43-46
        for name in self.MAP_NAMES:
            setattr(self, "max_map" + name, 0)
            setattr(self, "best_epoch_" + name, 0)
        super().__init__(cfg, *a, **k)

    def model_kwargs(self):
        """runners/UMoED/runner.py:104-124: the text token count ``dataset.max_word`` handed on"""
        return {"txt_token_size": self.cfg.dataset.get("max_word", 32)}

    def train_epoch(self, epoch: int):
        raise NotImplementedError("UMoEDTrainer.train_epoch: the backward of the decoder head is not built behind this name (xmh_head_umoed is "
                                  "inference only); the reference's epoch, through the train-mode head and both towers, is train_epoch_decoder "
                                  "(train_decoder() and run() with is_train run it)")

    def train_epoch_decoder(self, epoch: int):
        """runners/UMoED/runner.py:134-155: the backbone at backbone_lr and the hash layer at lr through UMoED.forward_train"""
        _train_epoch(self, epoch, no_ddp=_NO_DDP_UNCHECKED)

    def train_decoder(self):
        """the reference's train() with this epoch: every epoch followed by valid(), then the FINISHED line"""
        for epoch in range(self.epochs):
            self.train_epoch_decoder(epoch)
            self.valid(epoch, k=self.top_k)
        self._log_finished()

    def run(self):
        if self.is_train:
            self.train_decoder()
        else:
            self.test()

    def _log_finished(self):
        """runners/UMoED/runner.py:245-251: the line that ends train_decoder()"""
        self.logger.info(f">>>>>>> FINISHED >>>>>> Best epoch, I-T: {self.best_epoch_i2t}, mAP: {self.max_mapi2t}, T-I: {self.best_epoch_t2i}, "
                         f"mAP: {self.max_mapt2i}, I-I: {self.best_epoch_i2i}, MAP: {self.max_mapi2i}, T-T: {self.best_epoch_t2t}, MAP: {self.max_mapt2t}")

    def generate_hash(self, image, text, key_padding_mask=None):
        """runners/UMoED/runner.py:163-165 -> (image_hash, text_hash, fusion_hash); the model's forward leaves the fusion code None"""
        _, image_hash, _, text_hash, _, fusion_hash = self.model(image, text)
        return image_hash, text_hash, fusion_hash

    def generate_hashes(self, image, text, key_padding_mask=None):
        image_hash, text_hash, _ = self.generate_hash(image, text, key_padding_mask)
        return {"": (image_hash, text_hash)}

    def pack_hash_code(self, code, out, row_index, flags):
        if self.hash_func == "softmax":
            R.pack_pair_argmax(code.reshape(code.shape[0], -1), out=out, row_index=row_index)
        else:
            R.pack_sign(code, out=out, row_index=row_index, flags=flags)

    def _check_code_width(self):
        layer = self.model.hash
        width = (layer.hash_module if layer.fusion else layer.img_token_hash).code_width
        if width != self.output_dim * self.hash_scale:
            raise NotImplementedError("UMoEDTrainer: hash_func %s with merge_func mean gives a code %d wide for %d bits (the vocabulary "
                                      "2^(output_dim / setDim)), which the reference writes into its %d-wide buffer and fails; evaluation is "
                                      "built for codes of output_dim bits" % (self.hash_func, width, self.output_dim, self.output_dim))

    def get_code(self, data_loader, length: int):
        """runners/UMoED/runner.py:167-190 -> (image, text, fusion) fp32 [length, K]; the reference allocates the fusion buffer and never
        fills it (uninitialised memory): here it is all zero"""
        self._check_code_width()
        img, txt = super().get_code(data_loader, length)
        return img, txt, torch.zeros_like(img)

    def _save_codes(self, codes, save_file):
        """one .mat with the reference's eight keys (:253-268); the four files of an epoch share the unpacked codes, and a second file
        of the same codes is another name of the first"""
        from ..utils import matfile
        memo = self.__dict__.get("_mat_memo")
        if memo is None or memo[0] is not codes:
            q_img, q_txt, r_img, r_txt = (t.unpack() for t in codes)
            memo = self._mat_memo = [codes, (q_img, q_txt, torch.zeros_like(q_img), r_img, r_txt, torch.zeros_like(r_img)), None]
        if memo[2] is not None and os.path.exists(memo[2]):
            matfile.link_or_copy(memo[2], save_file)
            return
        names = ("q_img", "q_txt", "q_fus", "r_img", "r_txt", "r_fus", "q_l", "r_l")
        matfile.write_mat5(save_file, dict(zip(names, (*memo[1], self.query_labels, self.retrieval_labels))))
        memo[2] = save_file

    def valid(self, epoch, k=None):
        """runners/UMoED/runner.py:192-243: four mAPs through the packed scan, four maxima and best epochs, four .mat files"""
        assert self.query_loader is not None and self.retrieval_loader is not None
        self._check_code_width()
        save_dir = os.path.join(self.save_dir, "mat_files")
        os.makedirs(save_dir, exist_ok=True)
        self.logger.info("Valid.")
        maps, codes = self._evaluate(k)
        for name, value in zip(self.MAP_NAMES, maps):
            if getattr(self, "max_map" + name) < value:
                setattr(self, "best_epoch_" + name, epoch)
                self._save_codes(codes, os.path.join(save_dir, name + "-best.mat"))
            setattr(self, "max_map" + name, max(getattr(self, "max_map" + name), value))
        self._mat_memo = None
        mAPi2t, mAPt2i, mAPi2i, mAPt2t = maps
        self.logger.info(f">>>>>> [{epoch}/{self.epochs}], MAP(i->t): {mAPi2t}, MAP(t->i): {mAPt2i}, MAP(t->t): {mAPt2t}, MAP(i->i): {mAPi2i}, "
                         f"MAX MAP(i->t): {self.max_mapi2t}, epoch: {self.best_epoch_i2t}, MAX MAP(t->i): {self.max_mapt2i}, epoch: {self.best_epoch_t2i}, "
                         f"MAX MAP(i->i): {self.max_mapi2i}, epoch: {self.best_epoch_i2i}, MAX MAP(t->t): {self.max_mapt2t}, epoch: {self.best_epoch_t2t}, ")
        return mAPi2t, mAPt2i, mAPi2i, mAPt2t
