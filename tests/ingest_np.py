"""numpy statement of what the ingest kernel (amx_prep_ingest*) must produce: the float32 image of core.py:136 from the image in its
stored dtype, with the NIfTI header's scaling applied the way nibabel applies it (float64 product, float64 sum), then the NaN / Inf
handling of core.py:152-158 on that float32 image (tests/badvox_np.py).

    no scaling     out = np.float32(raw)
    (slope, inter) out = np.float32(np.float64(raw) * slope + inter)

The GPU tests (tests/test_gpu_ingest.py) compare the kernel with `convert` / `ingest` bit for bit; nothing here imports the package.
"""
from fractions import Fraction

import numpy as np

import badvox_np as B

DTYPES = [np.uint8, np.int16, np.uint16, np.int32, np.float32, np.float64]


def convert(raw, scaling=None):
    """-> the float32 array numpy makes of `raw` (same shape, same memory order)"""
    raw = np.asarray(raw)
    with np.errstate(over='ignore', invalid='ignore'):
        if scaling is None:
            return raw.astype(np.float32)
        slope, inter = scaling
        wide = raw.astype(np.float64)
        prod = wide * np.float64(slope)              # rounded once ...
        return (prod + np.float64(inter)).astype(np.float32)      # ... and once more, then narrowed


def ingest(raw, scaling=None, replace=None):
    """-> (float32 image after the optional replacement, number of NaN / Inf samples of the converted image)"""
    img = convert(raw, scaling)
    n = B.count(img)
    return (img if replace is None else B.replace(img, replace)), n


def same_bits(a, b):
    """bit for bit outside NaN positions; NaN positions must coincide (a NaN's payload is not part of the value rule)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != np.float32 or b.dtype != np.float32 or a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def fma_float32(r, slope, inter):
    """float32(fma(r, slope, inter)): the product exact, ONE rounding to float64, then the cast -- what a fused multiply-add gives"""
    exact = Fraction(float(r)) * Fraction(float(slope)) + Fraction(float(inter))
    return np.float32(np.float64(float(exact)))        # float(Fraction) rounds correctly (to nearest even)


def fma_sensitive_case(slope=0.1):
    """Searches an int16 sample r and an intercept for which float32(fma(r, slope, inter)) != float32(float64(r) * slope + inter).
    For an r whose product r * slope is inexact in float64 (error e), the intercept is chosen so that the rounded product plus the
    intercept lands EXACTLY half way between two float32 values: product-then-sum rounds that tie to even, the fused form sees the tie
    moved by e and rounds to the other neighbour.  -> (r, slope, inter)"""
    slope = float(slope)
    for r in range(3, 32768):
        t = float(np.float64(r) * np.float64(slope))
        e = Fraction(r) * Fraction(slope) - Fraction(t)
        if e == 0:
            continue
        # ties at 2^-20 * (1 + (2 k + 1) 2^-24): k even -> the even neighbour is below, k odd -> above
        k = 0 if e > 0 else 1
        tie = Fraction(1, 2 ** 20) * (1 + Fraction(2 * k + 1, 2 ** 24))
        inter = tie - Fraction(t)
        if Fraction(float(inter)) != inter:
            continue                                   # the intercept must be a float64
        inter = float(inter)
        two = np.float32(np.float64(r) * np.float64(slope) + np.float64(inter))
        if two.view(np.uint32) != fma_float32(r, slope, inter).view(np.uint32):
            return r, slope, inter
    raise AssertionError('no int16 sample separates the fused from the two-step form')
