"""Gibbs ringing removed from an image by local sub-voxel shifts (Kellner et al., MRM 2016; `Evaluation`'s key doUnring).

Truncation of k-space leaves ringing beside every sharp edge.  Per slice -- one position of the third spatial axis, one volume -- the image
is split by a Fourier filter into a part that rings along the first in-plane axis and a part that rings along the second; along every line
of each part, every pixel takes the value of the one of 41 sub-voxel shifts (|s| <= 1/2, in steps of 1/40) whose neighbourhood oscillates
least, interpolated back to the pixel's own position.  include/amico_amd.h fixes the arithmetic (`amx_prep_unring_device`); the shifted
copies are products with circulant matrices on the fp64 matrix cores, all in float64, rounded to float32 once.  A slice that holds a NaN or
Inf sample is passed through unchanged.  The mask plays no part: the operation needs the whole field of view.  There is no CPU fallback.
"""
import numpy as np

from . import _capi

KELLNER = 'KELLNER'                   # the value of doUnring that names the method (any letter case); True means the same
MIN_EXTENT, MAX_EXTENT = 8, 256       # in-plane extents the kernels take (include/amico_amd.h)


def is_unring(value):
    """doUnring: 'kellner' in any letter case or True -> True; False / None -> False; anything else is a ValueError"""
    if value is None or value is False:
        return False
    if value is True or (isinstance(value, str) and value.upper() == KELLNER):
        return True
    raise ValueError("doUnring must be 'kellner', True or False, got %r" % (value,))


def check_axes(axes):
    """unring_axes: two different spatial axes out of 0, 1, 2 (ValueError otherwise), as a tuple of ints"""
    try:
        ax = tuple(axes)
    except TypeError:
        ax = ()
    if len(ax) != 2 or any(isinstance(a, bool) or not isinstance(a, (int, np.integer)) for a in ax) \
            or any(int(a) not in (0, 1, 2) for a in ax) or int(ax[0]) == int(ax[1]):
        raise ValueError('unring_axes must be two different spatial axes out of 0, 1, 2, got %r' % (axes,))
    return int(ax[0]), int(ax[1])


def check_extents(shape3, axes):
    """the sentence Evaluation.set_data raises for a slice the kernels do not take"""
    ext = tuple(int(shape3[a]) for a in axes)
    if min(ext) < MIN_EXTENT or max(ext) > MAX_EXTENT:
        raise RuntimeError(f'doUnring: each in-plane extent must be {MIN_EXTENT} to {MAX_EXTENT} pixels; along unring_axes {tuple(axes)} '
                           f'the image is {ext[0]} x {ext[1]}')


def unring_device(plan, d_img, axes=(0, 1), stream=None):
    """plan: a `_capi.Prep`; d_img: device pointer (int) of the float32 image's element buffer in the plan's layout (left as it is).
    -> {'image': a float32 device tensor of plan.extent elements in the image's layout, 'slices': slices in the image, 'passed_through':
    those copied through for a NaN / Inf sample}.  The kernels of every chunk on `stream`, one wait behind the last, the two counts home."""
    import torch
    axes = check_axes(axes)
    check_extents(plan.shape[:3], axes)
    dev = torch.device('cuda', torch.cuda.current_device())
    # (zeros: memory between the elements of a view that is no permutation of a block is not written by the launch)
    out = torch.zeros(plan.extent, dtype=torch.float32, device=dev)
    slices, passed = plan.unring_device(d_img, out.data_ptr(), axes, stream)
    return {'image': out, 'slices': slices, 'passed_through': passed}


def unring(img, axes=(0, 1), ctx=None):
    """img float32 [X, Y, Z] or [X, Y, Z, nS] (numpy, C or Fortran order; anything else is copied to C-order float32) -> the dict of
    `unring_device` with 'image' as float32 numpy of img's shape and memory order.  Uploads, one wait, numpy out."""
    import torch
    from .models import get_context
    axes = check_axes(axes)
    img = np.asarray(img)
    if img.ndim not in (3, 4):
        raise ValueError('img must be [X, Y, Z] or [X, Y, Z, nS]')
    if img.dtype != np.float32 or not (img.flags.c_contiguous or img.flags.f_contiguous):
        img = np.ascontiguousarray(img, dtype=np.float32)
    if not img.flags.writeable:
        img = img.copy(order='K')                             # (torch takes no read-only array)
    v = img if img.ndim == 4 else img[..., None]
    check_extents(v.shape[:3], axes)
    if img.ndim == 3:
        v = np.lib.stride_tricks.as_strided(img, shape=img.shape + (1,), strides=img.strides + (4 * img.size,))
    ctx = ctx if ctx is not None else get_context()
    rank = np.arange(int(np.prod(v.shape[:3])), dtype=np.int32).reshape(v.shape[:3])
    plan = _capi.Prep(ctx, v.shape, tuple(s // 4 for s in v.strides), rank, [[i] for i in range(v.shape[3])], np.zeros(0, dtype=np.int32))
    try:
        dev = torch.device('cuda', torch.cuda.current_device())
        d_img = torch.from_numpy(np.lib.stride_tricks.as_strided(img, shape=(img.size,), strides=(4,))).to(dev)
        res = unring_device(plan, d_img.data_ptr(), axes)
        res['image'] = np.lib.stride_tricks.as_strided(res['image'].cpu().numpy()[:img.size], shape=img.shape, strides=img.strides)
    finally:
        plan.close()
    return res
