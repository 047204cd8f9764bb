#!/usr/bin/env python3
"""Time the three tensor fits (OLS, WLS, NLLS) of amx_dti_directions_device_f32 on one GPU, and the share of the direction
step in Evaluation.fit().

  python tools/time_dti_methods.py [--voxels 1000000] [--reps 7] [--shape 80 80 50]

Part 1: float32 NODDI signals (99-volume scheme) resident in HBM, HIP events around the device entry point, one warm-up
call per method, then `reps` rounds that alternate the methods; medians in ms, the ratio to OLS, and NLLS' trip counters
(trips its voxels needed / trips their wavefronts ran for them).  The signals are a 50 000-voxel synthetic block repeated
to the requested size: the fits depend on the voxel only.
Part 2: Evaluation.fit() on a raw volume of `shape` (all voxels in the mask), once per method after a warm-up fit:
dirs_precomputing_time (upload + gather + tensor fit) and fit_time from the configuration, and the tensor fit's own event
time as a share of their sum.  Prints one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--voxels', type=int, default=1000000)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--shape', type=int, nargs=3, default=[80, 80, 50])
    ap.add_argument('--skip-fit', action='store_true')
    args = ap.parse_args()
    import torch
    import amico_amd
    from amico_amd import dti, synthetic as S
    if not torch.cuda.is_available():
        raise SystemExit('time_dti_methods.py: no GPU')
    dev = torch.device('cuda', 0)
    dirs500 = S.fibonacci_hemisphere(500)
    ht = S.build_htable(dirs500)
    sc = S.make_scheme()
    K = S.noddi_kernels(sc, dirs500)
    block, _ = S.noddi_signals(50000, K, ht, sc, seed=5)
    n = args.voxels
    y = np.tile(block.astype(np.float32), ((n + len(block) - 1) // len(block), 1))[:n]
    d_y = torch.from_numpy(y).to(dev)
    d_dirs = torch.zeros((n, 3), dtype=torch.float64, device=dev)
    methods = ('OLS', 'WLS', 'NLLS')
    est = {m: dti.TensorDirections.from_scheme(sc, fit_method=m) for m in methods}
    ctx = est['OLS'].ctx

    def timed(m):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        est[m].fit_device(d_y.data_ptr(), n, d_dirs.data_ptr(), f32=True)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    for m in methods:
        timed(m)
    ts = {m: [] for m in methods}
    for _ in range(args.reps):
        for m in methods:
            ts[m].append(timed(m))
    out = {'voxels': n, 'volumes': int(sc.nS), 'reps': args.reps}
    for m in methods:
        out[m + '_ms'] = round(float(np.median(ts[m])), 4)
        out[m + '_ms_min_max'] = [round(float(min(ts[m])), 4), round(float(max(ts[m])), 4)]
    out['WLS_over_OLS'] = round(out['WLS_ms'] / out['OLS_ms'], 2)
    out['NLLS_over_OLS'] = round(out['NLLS_ms'] / out['OLS_ms'], 2)
    vt, wt = est['NLLS']._dti.last_trips()
    out['NLLS_trips_per_voxel'] = round(vt / n, 2)
    out['NLLS_idle_trip_share'] = round(1.0 - vt / max(wt, 1), 3)
    out['NLLS_unconverged'] = est['NLLS'].last_unconverged()
    if not args.skip_fit:
        shape = tuple(args.shape)
        nv = int(np.prod(shape))
        img = (np.tile(block, ((nv + len(block) - 1) // len(block), 1))[:nv].reshape(shape + (-1,)) * 1000.0).astype(np.float32)
        for i, m in enumerate(('OLS',) + methods):             # the first fit is the warm-up
            ae = amico_amd.Evaluation()
            ae.set_config('DTI_fit_method', m)
            ae.set_data(img, sc, None)
            ae.set_model('NODDI')
            ae.set_kernels(K, ht)
            ae.fit()
            if i == 0:
                continue
            d_v = ae._dev['y']
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            est[m].fit_device(d_v.data_ptr(), nv, d_dirs.data_ptr(), f32=True)
            b.record()
            torch.cuda.synchronize()
            total = ae.get_config('dirs_precomputing_time') + ae.get_config('fit_time')
            out['fit_' + m] = {'voxels': nv, 'dirs_precomputing_s': round(ae.get_config('dirs_precomputing_time'), 4),
                               'fit_s': round(ae.get_config('fit_time'), 4), 'tensor_fit_ms': round(a.elapsed_time(b), 4),
                               'tensor_fit_share': round(a.elapsed_time(b) * 1e-3 / total, 5)}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
