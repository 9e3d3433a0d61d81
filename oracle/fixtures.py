"""TEST INFRASTRUCTURE ONLY -- what the golden writers (oracle/make_golden_*.py) and the tests that read their files share: where the
fixtures live, the seeded label generators, the comparison of a gradient against a reference's fp32 one, a host buffer for the
argument-check tests.  Imports neither the reference nor the package."""
import ctypes
import os
import sys

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")


def out_path(name):
    """where a golden writer puts <name>: tests/golden/, or the directory given as its first argument"""
    return os.path.join(sys.argv[1] if len(sys.argv) > 1 else GOLDEN, name)


# ---- labels drawn from a torch generator --------------------------------------------------------------------------------------
def labels_random(g, B, C, p=0.05):
    L = (torch.rand(B, C, generator=g) < p).float()
    L[torch.arange(B), torch.randint(0, C, (B,), generator=g)] = 1.0
    return L


def labels_single(g, B, C):
    L = torch.zeros(B, C)
    L[torch.arange(B), torch.randint(0, C, (B,), generator=g)] = 1.0
    return L


def labels_shared(g, B, C):
    """multi-label rows all carry class 0: no pair of them is disjoint (Z = 0, M > 0)"""
    L = labels_random(g, B, C, 0.08)
    multi = L.sum(1) > 1
    L[multi, 0] = 1.0
    return L


def q64(t):
    """rounded to multiples of 1/64: keeps a stored feature tensor small"""
    return torch.round(t * 64.0) / 64.0


# ---- comparisons ------------------------------------------------------------------------------------------------------------
def grads_close(got, ref):
    """the references differentiate in fp32 (DCMHT through cdist's matmul route): compare relative to the largest entry of the tensor"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(got - ref).max()) <= 2e-5 * float(np.abs(ref).max()) + 1e-9


def grads_close_rows(got, ref):
    """grads_close for a matrix with rows clamped by F.normalize's eps: such (its
    gradient ~1e12 larger) is compared on its own, so that it does not loosen the comparison of the others"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    big = np.abs(ref).max(axis=1) > 1e6 * max(np.median(np.abs(ref).max(axis=1)), 1e-30)
    ok = True
    for rows in (big, ~big):
        if rows.any():
            ok &= float(np.abs(got[rows] - ref[rows]).max()) <= 2e-5 * float(np.abs(ref[rows]).max()) + 1e-9
    return ok


def aligned_host(n):
    """a 256-byte aligned host address with n bytes behind it (never dereferenced by a call that fails its checks)"""
    buf = np.zeros(n + 256, dtype=np.uint8)
    return buf, ctypes.c_void_p((buf.ctypes.data + 255) & ~255)
