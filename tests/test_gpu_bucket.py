"""GPU: xmh_bucket_pack / xmh_bucket_unpack (csrc/xmh_bucket.hip), the one-launch multi-tensor copy behind xmh/ddp.py.

Tensors of 1, chunk - 1, chunk, chunk + 1 and 3 chunk + 5 elements, one of them a slice of a larger tensor that starts 4 bytes past a
16-byte boundary (the dword route), one row without a tensor (zeros, flag 0); scales 1, 0.5 and 1 / 3.  Everything is compared to the
bit: the packed ranges against ``t * scale`` of torch (one fp32 product each), the padding between the tensors against the pattern the
buffer held before, the flag tail against the rows' presence; unpack(pack(x, 1)) against x, with the elements around an unaligned
destination untouched."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SCALES = (1.0, 0.5, 1.0 / 3.0)


def _lib():
    from xmh import _lib
    return _lib


def _upload(a: np.ndarray):
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def case():
    """the tensors (one None), their layout, and the device copies of the table and the chunk map"""
    from xmh import ddp
    L = _lib()
    chunk = int(L.lib.xmh_bertadam_chunk())
    gen = torch.Generator().manual_seed(1814)
    numels = [1, chunk - 1, chunk, chunk + 1, 3 * chunk + 5, 77, 2 * chunk + 3]
    big = torch.randn(numels[6] + 8, generator=gen).cuda()
    tensors = [torch.randn(n, generator=gen).cuda() for n in numels[:6]] + [big[1:1 + numels[6]]]
    assert big.data_ptr() % 16 == 0 and tensors[6].data_ptr() % 16 == 4
    tensors[5] = None                                                                    # a parameter without a gradient on this rank
    offsets, tail, total = ddp.bucket_layout(numels)
    cmap = ddp.chunk_map(numels, chunk)
    table = ddp.bucket_table([None if t is None else t.data_ptr() for t in tensors], numels)
    return dict(chunk=chunk, numels=numels, tensors=tensors, big=big, offsets=offsets, tail=tail, total=total, cmap=cmap, table=table,
                d_map=_upload(cmap), d_table=_upload(table))


def _pack(case, scale, flat, d_table=None):
    L = _lib()
    L.check(L.lib.xmh_bucket_pack(L.ptr(case["d_table"] if d_table is None else d_table), len(case["table"]), L.ptr(case["d_map"]),
                                  len(case["cmap"]), scale, L.ptr(flat), L.current_stream()), "xmh_bucket_pack")


@pytest.mark.parametrize("scale", SCALES)
def test_pack_is_the_scaled_concatenation_at_the_documented_offsets(case, scale):
    assert all(o % 64 == 0 for o in case["offsets"]) and case["tail"] % 64 == 0
    fill = torch.full((case["total"],), -7.25, device="cuda")
    flat = fill.clone()
    _pack(case, scale, flat)
    torch.cuda.synchronize()
    touched = torch.zeros(case["total"], dtype=torch.bool, device="cuda")
    for t, o, n in zip(case["tensors"], case["offsets"], case["numels"]):
        want = torch.zeros(n, device="cuda") if t is None else t.flatten() * scale
        assert torch.equal(_bits(flat[o:o + n]), _bits(want)), (n, scale)
        touched[o:o + n] = True
    n_t = len(case["numels"])
    flags = torch.tensor([0.0 if t is None else 1.0 for t in case["tensors"]], device="cuda")
    assert torch.equal(flat[case["tail"]:case["tail"] + n_t], flags)
    touched[case["tail"]:case["tail"] + n_t] = True
    assert not touched.all()                                                             # there IS padding to look at
    assert torch.equal(_bits(flat[~touched]), _bits(fill[~touched]))


def test_unpack_of_pack_is_the_identity_and_stays_inside_its_tensors(case):
    from xmh import ddp
    L = _lib()
    flat = torch.zeros(case["total"], device="cuda")
    _pack(case, 1.0, flat)
    big2 = torch.full_like(case["big"], 3.5)
    outs = [None if t is None else torch.full_like(t, 3.5) for t in case["tensors"][:6]] + [big2[1:1 + case["numels"][6]]]
    table = ddp.bucket_table([None if t is None else t.data_ptr() for t in outs], case["numels"], flags=False)
    L.check(L.lib.xmh_bucket_unpack(L.ptr(_upload(table)), len(table), L.ptr(case["d_map"]), len(case["cmap"]), L.ptr(flat),
                                    L.current_stream()), "xmh_bucket_unpack")
    torch.cuda.synchronize()
    for t, got in zip(case["tensors"], outs):
        if t is not None:
            assert torch.equal(_bits(got), _bits(t))
    assert float(big2[0]) == 3.5 and bool((big2[1 + case["numels"][6]:] == 3.5).all())  # the elements around the unaligned slice


def test_pack_in_place_scales_a_view_of_the_bucket(case):
    """a gradient that already is its range of the bucket (an optimiser that zeroes gradients instead of dropping them)"""
    from xmh import ddp
    flat = torch.zeros(case["total"], device="cuda")
    _pack(case, 1.0, flat)
    want = flat.clone()
    views = [flat[o:o + n] for o, n in zip(case["offsets"], case["numels"])]
    table = ddp.bucket_table([v.data_ptr() for v in views], case["numels"])
    _pack(case, 0.5, flat, d_table=_upload(table))
    torch.cuda.synchronize()
    for o, n in zip(case["offsets"], case["numels"]):
        assert torch.equal(_bits(flat[o:o + n]), _bits(want[o:o + n] * 0.5))


def test_no_tensors_is_a_successful_no_op_and_bad_arguments_are_reported(case):
    L = _lib()
    assert L.lib.xmh_bucket_pack(None, 0, None, 0, 1.0, None, None) == 0
    assert L.lib.xmh_bucket_unpack(None, 0, None, 0, None, None) == 0
    flat = torch.zeros(case["total"] + 1, device="cuda")
    assert L.lib.xmh_bucket_pack(L.ptr(case["d_table"]), -1, L.ptr(case["d_map"]), 1, 1.0, L.ptr(flat), None) == -22
    assert L.lib.xmh_bucket_pack(None, 1, L.ptr(case["d_map"]), 1, 1.0, L.ptr(flat), None) == -22
    assert L.lib.xmh_bucket_pack(L.ptr(case["d_table"]), 2, L.ptr(case["d_map"]), 1, 1.0, L.ptr(flat), None) == -22
    assert L.lib.xmh_bucket_pack(L.ptr(case["d_table"]), 1, L.ptr(case["d_map"]), 1, 1.0, L.ptr(flat[1:]), None) == -22
    assert b"16-byte" in L.lib.xmh_last_error()
