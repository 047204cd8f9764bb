"""numpy restatement of load_data's NaN / Inf handling (core.py:152-158 on the raw image, core.py:270-276 on the pre-processed one):

    if np.isnan(img).any() or np.isinf(img).any():
        if replace_bad_voxels is not None:
            np.nan_to_num(img, copy=False, nan=r, posinf=r, neginf=r)
        else:
            ERROR(...)

`count` is the number of samples that make the reference's test true; `replace` is its nan_to_num call on a copy.  The GPU tests
(tests/test_gpu_badvox.py) compare the kernels with these two, bit for bit.
"""
import numpy as np


def bad(img):
    """the samples core.py:153 / 271 react to"""
    img = np.asarray(img)
    return np.isnan(img) | np.isinf(img)


def count(img):
    return int(bad(img).sum())


def replace(img, r):
    """-> a copy of `img` (same dtype, same memory order) after np.nan_to_num(copy=False, nan=r, posinf=r, neginf=r)"""
    out = np.array(img, copy=True, order='K')
    np.nan_to_num(out, copy=False, nan=r, posinf=r, neginf=r)
    return out


def bits(a):
    """integer view for bit-for-bit comparisons (-0.0 and 0.0, or two NaN payloads, differ here)"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)
