#!/usr/bin/env python3
"""The mask gather on long protocols (k_prep_long, csrc/amx_volume.hip) beside the two-tile route (k_prep_gather) at 288 volumes:
plain preparation (identity groups, b0 normalisation, float64 rows), planar and interleaved image, the box and blob mask of
`bench.py --model prep` (128 x 128 x 80, about half of it masked).  The image is made on the device (2.7 GB at 512 volumes).

Per case: the kernel that ran with its grid and LDS (amx_prep_last_launch), median / min / max of the device-event times, and the
rate as IMAGE bytes per second (masked voxels x volumes x 4 B / time: the rows written, 8 B a sample, are not counted).  Every line
starts with the library's amx_build_id.

    python tools/time_prep_long.py [--reps 7] [--shape 128,128,80]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
CASES = ((288, 'F'), (288, 'C'), (512, 'F'), (512, 'C'))


def case(n, order, shape, reps):
    import torch
    from amico_amd import _capi, prep, synthetic as S
    tag = _capi.build_id()
    sc = S.make_scheme(n_b0=9, shells=((700.0, 30), (2000.0, n - 39)), seed=0)
    like = np.empty(shape + (n,), dtype=np.float32, order=order)          # geometry only: never touched
    xx, yy, zz = np.meshgrid(*[np.linspace(-1, 1, s) for s in shape], indexing='ij')
    mask = ((xx * xx + yy * yy + zz * zz) < 0.92).astype(np.uint8)
    sp = prep.SignalPreparation(sc, like, mask)
    ctx, L = sp.ctx, _capi.lib()
    d_img = torch.rand(like.size, dtype=torch.float32, device='cuda:0') * 900.0 + 100.0
    d_y = torch.zeros((sp.n_vox, sp.n_out), dtype=torch.float64, device='cuda:0')
    d_m = torch.zeros(sp.n_vox, dtype=torch.float32, device='cuda:0')
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for _ in range(reps + 2):                                             # two warm-up launches
        ev[0].record()
        ctx.check(L.amx_prep_gather_device(ctx._h, sp._plan._h, d_img.data_ptr(), 1, 0.0, d_y.data_ptr(), d_m.data_ptr(), None))
        ev[1].record()
        torch.cuda.synchronize()
        ms.append(ev[0].elapsed_time(ev[1]))
    t, lo, hi = float(np.median(ms[2:])), min(ms[2:]), max(ms[2:])
    name, grid, block, lds = sp._plan.last_launch()
    image_bytes = sp.n_vox * n * 4
    print(f'{tag} | {n} volumes, {"planar" if order == "F" else "interleaved"}: {name} grid {grid} x {block} threads, {lds} B LDS, '
          f'{sp.n_vox} masked voxels: median {t:.3f} ms (min {lo:.3f}, max {hi:.3f}, {reps} launches) -> '
          f'{image_bytes / t / 1e6:.1f} GB/s of image', flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--shape', default='128,128,80')
    a = ap.parse_args()
    shape = tuple(int(v) for v in a.shape.split(','))
    for n, order in CASES:
        case(n, order, shape, a.reps)


if __name__ == '__main__':
    main()
