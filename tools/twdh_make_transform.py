#!/usr/bin/env python3
"""Make, or check, one of TwDH's short-code transforms (xmh/models/twdh_transform.py), with the flag names of the
reference's runners/TwDH/transform_matrix_generation/train.py.

  make:   python tools/twdh_make_transform.py --label-file dataset/coco/label.mat --long-dim 512 --output-dim 16 \\
              --long-center-path data/transformer/TwDH/coco/long/512.pkl --short-center-path data/transformer/TwDH/coco/short/16.pkl \\
              --save-dir data/transformer/TwDH/coco/trans
          writes <save-dir>/<long-dim>/<output-dim>.pkl after every epoch and <output-dim>_zeros.pkl once the matrix is lossless, the
          layout TwDH's `trans_matrix` reads.  (TwDH reads every file of <trans_matrix>/<long-dim>/ as a code length: move the _zeros copy
          away before pointing a config at the directory.)  The label rows are those of the training split: set_seed(--seed), then
          split_data(..., --query-num, --train-num) of xmh/dataset/transformer_dataset.py, as the runner draws it.
  check:  python tools/twdh_make_transform.py --check-only --long-dim 512 --long-center-path .../long --short-center-path .../short \\
              --save-dir .../trans
          prints the wrong-bit count of every <save-dir>/<long-dim>/<short>.pkl whose short centre <short-center-path>/<short>.pkl exists
          (with --output-dim: of that one; the centre paths may name the .pkl files themselves).  Exit status 1 when a matrix is not
          lossless.

Both need the GPU; there is no CPU fallback."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "clip-based-cross-modal-hash_amd"))


def get_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--label-file", type=str, default="./dataset/label.mat", help="label.mat")
    ap.add_argument("--query-num", type=int, default=5000, help="query set size")
    ap.add_argument("--train-num", type=int, default=10000, help="training dataset size")
    ap.add_argument("--seed", type=int, default=1814)
    ap.add_argument("--batch-size", type=int, default=200)
    ap.add_argument("--post-epochs", type=int, default=100)
    ap.add_argument("--long-dim", type=int, default=512)
    ap.add_argument("--output-dim", type=int, default=None, help="short length (make: default 16; check: default every length found)")
    ap.add_argument("--post-lr", type=float, default=0.001)
    ap.add_argument("--weight-decay", type=float, default=0.2)
    ap.add_argument("--warmup-proportion", type=float, default=0.1)
    ap.add_argument("--long-center-path", type=str, default="./data/transformer/TwDH/coco/long/512.pkl")
    ap.add_argument("--short-center-path", type=str, default="./data/transformer/TwDH/coco/short/16.pkl")
    ap.add_argument("--save-dir", type=str, default="./")
    ap.add_argument("--check-only", action="store_true", help="print the fidelity of existing matrices instead of training one")
    return ap.parse_args(argv)


def _centre(path, name):
    """a centre path names the .pkl itself or the directory that holds <name>.pkl"""
    return os.path.join(path, "%d.pkl" % name) if os.path.isdir(path) else path


def _short_centre(path, short):
    """the centre file of one short length: <path>/<short>.pkl, or <path> itself when it is that file; None when there is none"""
    if os.path.isdir(path):
        f = os.path.join(path, "%s.pkl" % short)
        return f if os.path.isfile(f) else None
    return path if os.path.basename(path).split(".")[0] == short and os.path.isfile(path) else None


def _load(path):
    return torch.load(path, map_location="cpu").float()


def train_labels(a):
    """the label rows of the training split, through the dataset code the runner uses"""
    import scipy.io as scio
    from xmh.dataset.transformer_dataset import _first_key, split_data
    from xmh.runners.base import set_seed
    labels = _first_key(scio.loadmat(a.label_file), ("category", "LAll", "labels"), "label")
    set_seed(a.seed)
    rows = np.arange(len(labels))
    _, _, (_, train, _) = split_data(rows, rows, labels, query_num=a.query_num, train_num=a.train_num)
    return torch.as_tensor(np.asarray(train))


def check_only(a):
    from xmh.models.twdh_transform import transform_fidelity
    long_c = _load(_centre(a.long_center_path, a.long_dim))
    folder = os.path.join(a.save_dir, str(a.long_dim))
    names = ["%d.pkl" % a.output_dim] if a.output_dim is not None else sorted(os.listdir(folder))
    bad = 0
    for item in names:
        key = item.split(".")[0]
        centre = _short_centre(a.short_center_path, key.split("_")[0])      # <short>_zeros.pkl is checked against <short>'s centre
        if centre is None:
            print("%s: no short centre for it, skipped" % os.path.join(folder, item))
            continue
        short_c = _load(centre)
        n, wrong = transform_fidelity(long_c, short_c, _load(os.path.join(folder, item)))
        where = [tuple(x) for x in wrong.nonzero().tolist()]
        print("%s: %d wrong of %d (class, bit)%s" % (os.path.join(folder, item), n, wrong.numel(),
                                                    " at %s%s" % (where[:16], " ..." if n > 16 else "") if n else ": lossless"))
        bad += n > 0
    return 1 if bad else 0


def main(argv=None):
    a = get_args(argv)
    if not torch.cuda.is_available():
        sys.exit("twdh_make_transform: no GPU (the objective, its gradient and the check are HIP kernels; there is no CPU fallback)")
    if a.check_only:
        return check_only(a)
    from xmh.models.twdh_transform import generate_transform
    from xmh.runners.base import set_seed
    S = 16 if a.output_dim is None else a.output_dim
    long_c, short_c = _load(_centre(a.long_center_path, a.long_dim)), _load(_centre(a.short_center_path, S))
    if long_c.shape[1] != a.long_dim or short_c.shape[1] != S:
        sys.exit("twdh_make_transform: centres of shape %s and %s for --long-dim %d --output-dim %d"
                 % (tuple(long_c.shape), tuple(short_c.shape), a.long_dim, S))
    labels = train_labels(a)
    set_seed(a.seed)                                                        # the matrix, the order and the ties start from the seed
    out = generate_transform(labels, long_c, short_c, batch_size=a.batch_size, post_epochs=a.post_epochs, post_lr=a.post_lr,
                             weight_decay=a.weight_decay, warmup=a.warmup_proportion, save_dir=a.save_dir, logger=print)
    print("%s after epoch %d: %s" % (os.path.join(a.save_dir, str(a.long_dim), "%d.pkl" % S), out.epoch,
                                    "lossless" if out.lossless else "NOT lossless"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
