#!/usr/bin/env python3
"""What the tensor maps (amx_dti_fit*, doSaveTensorMaps, tensor_maps=True) cost on one GPU.

  python tools/time_dti_maps.py [--shape 100 95 62] [--reps 7] [--skip-fit]

The default shape is 589 000 voxels; 99-volume scheme, float32 rows.  The signals are a 50 000-voxel synthetic NODDI block repeated
to the requested size: the fits depend on the voxel only.
Part 1: the tensor pass on rows resident in HBM, HIP events around the device entry point, per method (OLS, WLS, NLLS) without map
outputs (amx_dti_directions_device_f32's kernel) and with them; one warm-up each, then `reps` rounds that alternate all six; medians.
Part 2: everything ahead of the model fit in the volume pipeline (image -> y, mean b0, directions), OLS: the fused gather (the
default), gather + tensor pass (fused=False), gather + tensor pass with maps (tensor_maps=True); alternating, medians.
Part 3: Evaluation.fit() (NODDI, OLS) with doSaveTensorMaps off and on, alternating, wall time of the whole call; medians.
Prints one line per figure and `amx_build_id`.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', type=int, nargs=3, default=[100, 95, 62])
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--skip-fit', action='store_true')
    args = ap.parse_args()
    import torch
    import amico_amd
    from amico_amd import _capi, dti, pipeline, synthetic as S
    if not torch.cuda.is_available():
        raise SystemExit('time_dti_maps.py: no GPU')
    dev = torch.device('cuda', 0)
    dirs500 = S.fibonacci_hemisphere(500)
    ht = S.build_htable(dirs500)
    sc = S.make_scheme()
    K = S.noddi_kernels(sc, dirs500)
    block, _ = S.noddi_signals(50000, K, ht, sc, seed=5)
    shape = tuple(args.shape)
    n = int(np.prod(shape))
    y = np.tile(block.astype(np.float32), ((n + len(block) - 1) // len(block), 1))[:n]
    build = _capi.build_id()
    print(f'{build}: {n} voxels x {sc.nS} volumes, float32 rows, {args.reps} rounds, medians [min, max]')

    def events(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def rounds(legs):
        """legs: name -> callable returning ms; one warm-up each, then alternating"""
        for fn in legs.values():
            fn()
        ts = {k: [] for k in legs}
        for _ in range(args.reps):
            for k, fn in legs.items():
                ts[k].append(fn())
        return {k: (float(np.median(v)), min(v), max(v)) for k, v in ts.items()}

    # ---- part 1: the tensor pass
    d_y = torch.from_numpy(y).to(dev)
    d_dirs = torch.zeros((n, 3), dtype=torch.float64, device=dev)
    d_ev = torch.zeros((n, 3), dtype=torch.float64, device=dev)
    d_sc = torch.zeros((n, 4), dtype=torch.float64, device=dev)
    legs = {}
    for m in ('OLS', 'WLS', 'NLLS'):
        est = dti.TensorDirections.from_scheme(sc, fit_method=m)
        legs[m + ' directions'] = lambda e=est: events(lambda: e.fit_device(d_y.data_ptr(), n, d_dirs.data_ptr(), f32=True))
        legs[m + ' directions + maps'] = lambda e=est: events(lambda: e.fit_device(d_y.data_ptr(), n, d_dirs.data_ptr(), f32=True,
                                                                                  d_evals=d_ev.data_ptr(), d_scalars=d_sc.data_ptr()))
    res = rounds(legs)
    for m in ('OLS', 'WLS', 'NLLS'):
        a, b = res[m + ' directions'], res[m + ' directions + maps']
        print(f'{build}: tensor pass {m}: directions {a[0]:.3f} ms [{a[1]:.3f}, {a[2]:.3f}], with maps {b[0]:.3f} ms [{b[1]:.3f}, {b[2]:.3f}], '
              f'ratio {b[0] / a[0]:.3f}')
    del d_y, d_dirs, d_ev, d_sc

    # ---- part 2: image -> y, directions (OLS): fused gather against the two-kernel routes
    img = (y.reshape(shape + (-1,)) * 1000.0).astype(np.float32)
    del y
    mask = np.ones(shape, dtype=np.uint8)
    d_img = torch.from_numpy(img.reshape(-1)).to(dev)
    pipes = {'fused gather (default)': pipeline.NoddiVolumePipeline(sc, img, mask, K, ht),
             'gather + tensor pass': pipeline.NoddiVolumePipeline(sc, img, mask, K, ht, fused=False),
             'gather + tensor pass with maps': pipeline.NoddiVolumePipeline(sc, img, mask, K, ht, tensor_maps=True)}
    res = rounds({k: (lambda p=p: events(lambda: p._enqueue_signals(d_img, None))) for k, p in pipes.items()})
    base = res['fused gather (default)'][0]
    for k, v in res.items():
        print(f'{build}: image -> y + directions, OLS, {k}: {v[0]:.3f} ms [{v[1]:.3f}, {v[2]:.3f}], {v[0] - base:+.3f} ms against the fused gather')
    del pipes, d_img

    # ---- part 3: Evaluation.fit()
    if not args.skip_fit:
        def fit(on):
            ae = amico_amd.Evaluation()
            ae.set_config('doSaveTensorMaps', on)
            ae.set_data(img, sc, None)
            ae.set_model('NODDI')
            ae.set_kernels(K, ht)
            t = time.perf_counter()
            ae.fit()
            return (time.perf_counter() - t) * 1e3
        res = rounds({'off': lambda: fit(False), 'on': lambda: fit(True)})
        a, b = res['off'], res['on']
        print(f'{build}: Evaluation.fit() NODDI OLS: doSaveTensorMaps off {a[0]:.1f} ms [{a[1]:.1f}, {a[2]:.1f}], on {b[0]:.1f} ms [{b[1]:.1f}, {b[2]:.1f}], '
              f'{b[0] - a[0]:+.1f} ms (two float32 volumes more come to the host: {n * 7 * 4 / 1e6:.1f} MB)')


if __name__ == '__main__':
    main()
