"""CPU side of the encoder numerics (tests/encode_numerics.py): the float64-capable oracle, the outlier weights and the plane-split
emulation that tests/test_gpu_encode_numerics.py holds the kernels to."""
import contextlib
import os

import numpy as np
import torch

import encode_numerics as N
from conftest import GOLDEN
from oracle import encode as enc


def _weights():
    from xmh.models import weights
    return weights


@contextlib.contextmanager
def _threads(n):
    before = torch.get_num_threads()
    torch.set_num_threads(n)
    try:
        yield
    finally:
        torch.set_num_threads(before)


def test_oracle_keeps_fp32_and_computes_in_float64():
    g = np.load(os.path.join(GOLDEN, "encode_clip_b2.npz"))
    W = _weights()
    seed = int(g["seed"])
    sd = enc.fp16_round_like_reference(W.synth_clip_state_dict(seed))
    image, (ids, pad) = W.synth_images(seed, 2), W.synth_text(seed, 2)
    with torch.no_grad(), _threads(8):
        cls = enc.clip_image(sd, image)
        eos = enc.clip_text(sd, ids)
        assert cls.dtype == torch.float32 and eos.dtype == torch.float32
        assert N.rel_rows(cls, g["img_cls"]) < 2e-5 and N.rel_rows(eos, g["txt_eos"]) < 2e-5
        sd64 = N.f64(sd)
        cls64, tok64 = enc.clip_image(sd64, image.double(), return_patches=True)
        eos64, ttok64, nm = enc.clip_text(sd64, ids, key_padding_mask=pad, return_patches=True)
        assert {cls64.dtype, tok64.dtype, eos64.dtype, ttok64.dtype} == {torch.float64}
        assert np.array_equal(nm.numpy(), g["txt_mask_rp"])
        # the fp32 oracle (and so the reference, per the golden) sits within fp32 roundoff of float64
        e_img, e_txt = N.rel_rows(cls, cls64), N.rel_rows(eos, eos64)
        assert 0 < e_img < 1e-5 and 0 < e_txt < 1e-5, (e_img, e_txt)
        assert N.rel_rows(g["img_cls"], cls64) < 2e-5 and N.rel_rows(g["txt_eos"], eos64) < 2e-5


def test_rel_rows_sees_a_small_row():
    want = torch.tensor([[1000.0, -2000.0], [1e-3, 2e-3]], dtype=torch.float64)
    got = want.clone()
    got[1, 0] += 1e-4
    assert abs(N.rel_rows(got, want) - 0.05) < 1e-9                            # a global max-normalised error would say 5e-8
    assert N.rel_rows(want, want) == 0.0


def test_outlier_weights_are_deterministic_fp16_exact_and_in_range():
    W = _weights()
    a, b = N.outlier_clip_state_dict(5, vision_layers=2, transformer_layers=2), N.outlier_clip_state_dict(5, vision_layers=2, transformer_layers=2)
    assert all(torch.equal(a[k], b[k]) for k in a)
    plain = W.synth_clip_state_dict(5, vision_layers=2, transformer_layers=2)
    assert set(a) == set(plain) and any(not torch.equal(a[k], plain[k]) for k in a)
    r = enc.fp16_round_like_reference(a)
    for k in r:                                                                 # the GEMM weights are fp16 values ...
        if ".attn." in k or ".mlp." in k or k.endswith("conv1.weight") or k in ("visual.proj", "text_projection"):
            assert torch.equal(r[k].half().float(), r[k]), k
    # ... and the full-size towers' activations stay inside the fp16 range while reaching real-CLIP magnitudes
    sd64 = N.f64(enc.fp16_round_like_reference(N.outlier_clip_state_dict(1814)))
    rec, probs = [], []
    with torch.no_grad(), _threads(8), N.linear_probe(record=rec), N.softmax_probe(probs):
        enc.clip_image(sd64, W.synth_images(1814, 2).double())
        n_img = len(rec)
        enc.clip_text(sd64, W.synth_text(1814, 2)[0])
    assert n_img == 48 and len(rec) == 96 and len(probs) == 24
    # one head per layer (layer % heads) near one-hot: its mean largest probability over the query rows that see 9 keys or more
    # (the text tower is causal) is above 0.75 in every layer of both towers; the other heads stay below 0.3
    for i, p in enumerate(probs):
        heads = 12 if i < 12 else 8
        L = p.shape[-1]
        peak = p.view(2, heads, L, L)[:, :, 8:].amax(-1).mean(dim=(0, 2))
        h = (i % 12) % heads
        assert peak[h] > 0.75 and torch.cat([peak[:h], peak[h + 1:]]).max() < 0.3, (i, peak.tolist())
    big = max(max(x, y) for x, y in rec)
    assert 100 < big < N.F16_MAX, big
    fc_pre = [rec[4 * i + 2][1] for i in range(24)]                             # c_fc outputs of every layer, both towers
    assert min(fc_pre) > 40 and max(fc_pre) > 100, fc_pre
    for tower in (rec[:48], rec[48:]):
        assert max(y for _, y in tower[3::4]) > 250                            # the residual channels pass through c_proj


def _h(x):
    return np.array(x, dtype=np.float16)


def test_split_emulation_at_every_edge():
    cases = [
        # x                         hi                      lo
        (0.0,                       0.0,                    0.0),
        (1.0 + 2.0 ** -23,          1.0,                    2.0 ** -23),       # lo normal: the full 24-bit mantissa survives
        (1.0 + 2.0 ** -10 + 2.0 ** -11, 1.0 + 2.0 ** -10,   2.0 ** -11),
        (2.0 ** -20,                2.0 ** -20,             0.0),              # hi an fp16 subnormal, exact
        (2.0 ** -20 * (1 + 2.0 ** -10), 2.0 ** -20,         0.0),              # ... bits below 2^-24 are lost (mask kept them)
        (2.0 ** -25,                0.0,                    0.0),              # below the smallest fp16 subnormal
        (2.0 ** -24 * 1.5,          2.0 ** -24,             0.0),
        (2.0 ** -14,                2.0 ** -14,             0.0),              # smallest fp16 normal
        (2.0 ** -4 * (1 + 2.0 ** -12), 2.0 ** -4,           2.0 ** -16),       # lo subnormal (below 2^-14), exact
        (2.0 ** -4 * (1 + 2.0 ** -22), 2.0 ** -4,           0.0),              # lo below 2^-24: lost
        (2.0 ** -3 * (1 + 2.0 ** -13), 2.0 ** -3,           2.0 ** -16),
        (1e-40,                     0.0,                    0.0),              # fp32 subnormal
        (65504.0,                   65504.0,                0.0),
        (65535.0,                   65504.0,                31.0),             # [65504, 65536): hi + lo still holds x
        (65536.0,                   65504.0,                0.0),              # saturation: hi clamps, lo cannot make up for it
        (70000.0,                   65504.0,                48.0),             # 70000 - 69952 (the masked value)
        (3.0e38,                    65504.0,                65504.0),
    ]
    for x, hi, lo in cases:
        for s in (1.0, -1.0):
            h, l = N.split_planes(np.array([s * x], np.float32))
            assert h[0] == _h(s * hi) and l[0] == _h(s * lo), (s * x, float(h[0]), float(l[0]))
    h, l = N.split_planes(np.array([np.inf, -np.inf, np.nan], np.float32))
    assert h[0] == np.inf and h[1] == -np.inf and np.isnan(h[2]) and np.isnan(l).all()
    assert N.split_value(np.array([65535.5], np.float32))[0] == np.float32(65535.5)
    assert N.fast_value(np.array([65519.0, 65520.0, 1.0 + 2.0 ** -11], np.float32)).tolist() == [65504.0, np.inf, 1.0]
    # the stated accuracy over a sweep: 2^-21 relative from 2^-3 up, 2^-23 absolute below, up to (not including) 65536
    rng = np.random.default_rng(3)
    x = (np.exp2(rng.uniform(-30, 16, 100000)) * rng.choice([-1, 1], 100000)).astype(np.float32)
    x = x[np.abs(x) < 65536]
    err = np.abs(N.split_value(x).astype(np.float64) - x)
    assert (err <= np.maximum(2.0 ** -21 * np.abs(x), 2.0 ** -23)).all()
    assert (err[np.abs(x) >= 0.125] <= 2.0 ** -21 * np.abs(x[np.abs(x) >= 0.125])).all()
