#!/usr/bin/env python3
"""Goldens of the training image transform, made with Pillow (12.2 when this was written) and torch on the CPU:
python tools/make_golden_train_transform.py [DIR] -> tests/golden/train_transform.npz (or DIR/).  Nothing at test time runs
or imports this.

Cases, sources and the file layout come from tests/train_transform_cases.py.  Per case `<name>`:
  img_<name>      the source, uint8 [H, W, 3]; cases of one shape share a source, stored once under the first of them
                  (TC.golden_source), and the sources made by an integer formula are left out: the test regenerates them
  params_<name>   int64 [5] = (top, left, h, w, flip), r_<name> the output size
  u8_<name>       Image.fromarray(img) [.transpose(FLIP_LEFT_RIGHT)] .crop(box) .resize((r, r), Image.BILINEAR), uint8 [r, r, 3]
  f32_<name>      torch: ToTensor (HWC uint8 -> CHW float32 / 255) and Normalize (sub_(mean).div_(std)) on u8_<name>, [3, r, r];
                  only for TC.F32_CASES: the float stage is one function of the uint8 result per pixel
and the same for every image of every batch, `<batch>.<i>`.  The numpy restatement of the cases module is asserted equal to
every array before the file is written."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import train_transform_cases as TC  # noqa: E402
from oracle.fixtures import out_path  # noqa: E402


def torch_tensor(u8):
    x = torch.from_numpy(u8.copy()).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    mean, std = torch.tensor(TC.CLIP_MEAN, dtype=torch.float32), torch.tensor(TC.CLIP_STD, dtype=torch.float32)
    return x.sub_(mean[:, None, None]).div_(std[:, None, None]).numpy()


def main():
    import PIL
    out = {"pillow_version": np.asarray(PIL.__version__)}
    items = [(n,) + TC.case_inputs(n) + (TC.case_stored(n),) for n in TC.CASES]
    for b, spec in TC.BATCHES.items():
        imgs, params = TC.batch_inputs(b)
        items += [("%s.%d" % (b, i), im, p, TC.R, spec[i][3] != "formula" and TC.batch_source_of(b, i) == i) for i, (im, p) in enumerate(zip(imgs, params))]
    for name, img, params, r, stored in items:
        u8 = TC.pillow_resize_u8(img, params, r)
        assert np.array_equal(u8, TC.resize_u8(img, params, r)), name
        if stored:
            out["img_" + name] = img
        out["params_" + name], out["r_" + name], out["u8_" + name] = params, np.int64(r), u8
        if name in TC.F32_CASES:
            out["f32_" + name] = torch_tensor(u8)
            assert np.array_equal(out["f32_" + name], TC.to_tensor_normalize(u8)), name
    path = out_path("train_transform.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays of %d cases, %d bytes (Pillow %s)" % (path, len(out), len(items), os.path.getsize(path), PIL.__version__))


if __name__ == "__main__":
    main()
