#!/usr/bin/env python3
"""Gibbs unringing (amico_amd/unring.py, csrc/amx_unring.hip): the whole of amx_prep_unring_device -- tables, and per chunk the
gather, four DFT passes, two shift passes and the scatter, with its wait for the last chunk -- on float32 images in HBM, axes (0, 1), one
process per leg under a time limit of its own, median of 5, host clock around the call (it waits itself) and device events around it:

  c99, f99      96 x 96 x 60 x 99: C order (the volume index fastest) | Fortran order (nibabel's: axis 0 fastest)
  c306, f306    128 x 128 x 70 x 306

The flop count is that of the shifted copies alone: 2 axes x 40 shifts x 2 n^2 per line x n lines a slice.  Every line starts with the
library's amx_build_id.

    python tools/time_unring.py [--reps 5] [--leg NAME] [--out FILE]      (no --leg: every leg, each in a process of its own)
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
LEGS = {'c99': ((96, 96, 60, 99), 'C'), 'f99': ((96, 96, 60, 99), 'F'), 'c306': ((128, 128, 70, 306), 'C'), 'f306': ((128, 128, 70, 306), 'F')}
LIMIT = {'c99': 120, 'f99': 120, 'c306': 240, 'f306': 240}           # seconds a leg may take


def leg(name, reps):
    import torch
    from amico_amd import _capi, get_context
    shape, order = LEGS[name]
    total = int(np.prod(shape))
    strides = (shape[1] * shape[2] * shape[3], shape[2] * shape[3], shape[3], 1) if order == 'C' else \
        (1, shape[0], shape[0] * shape[1], shape[0] * shape[1] * shape[2])
    ctx = get_context()
    rank = np.arange(int(np.prod(shape[:3])), dtype=np.int32).reshape(shape[:3])
    plan = _capi.Prep(ctx, shape, strides, rank, [[i] for i in range(shape[3])], np.zeros(0, dtype=np.int32))
    g = torch.Generator(device='cuda').manual_seed(1)
    d_img = (900.0 + 45.0 * torch.randn(plan.extent, generator=g, device='cuda', dtype=torch.float32)).abs_()
    out = torch.empty(plan.extent, dtype=torch.float32, device='cuda')
    rt = _capi.unring_route(shape[0], shape[1])
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    host, dev = [], []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev[0].record()
        slices, passed = plan.unring_device(d_img.data_ptr(), out.data_ptr(), (0, 1))
        ev[1].record()
        torch.cuda.synchronize()
        host.append((time.perf_counter() - t0) * 1e3)
        dev.append(ev[0].elapsed_time(ev[1]))
    host, dev = host[1:], dev[1:]
    n_a, n_b = shape[:2]
    flop = slices * 40.0 * (2.0 * n_a * n_a * n_b + 2.0 * n_b * n_b * n_a)
    t = float(np.median(dev))
    print(f'{_capi.build_id()} | {name}: {shape[0]} x {shape[1]} x {shape[2]} x {shape[3]} {order} order ({4 * total / 1e6:.0f} MB), {slices} slices, '
          f'{passed} passed through, chunks of {rt["chunk"]} slices ({-(-slices // rt["chunk"])} of them), LDS {rt["lds_dft"]} / {rt["lds_shift"]} B | '
          f'amx_prep_unring_device: device events median {t:.1f} ms (min {min(dev):.1f}, max {max(dev):.1f}), host clock median '
          f'{np.median(host):.1f} ms; shifted copies {flop / 1e12:.2f} TFLOP: {flop / t / 1e9:.1f} TFLOP/s; {1e3 * t / slices:.1f} us per slice',
          flush=True)
    plan.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--leg', choices=sorted(LEGS))
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'profiles', 'unring_rate.txt'))
    a = ap.parse_args()
    if a.leg:
        return leg(a.leg, a.reps)
    lines = ['tools/time_unring.py on an MI355X: amx_prep_unring_device, axes (0, 1), float32 images in HBM (|900 + 45 N(0, 1)|), one process per '
             'leg, median of %d after one warm-up call; device events and the host clock around the call, which waits for its last chunk itself.' % a.reps, '']
    for name in LEGS:                                       # a fresh child process per leg, each under its own time limit
        res = subprocess.run([sys.executable, os.path.abspath(__file__), '--reps', str(a.reps), '--leg', name], timeout=LIMIT[name],
                             stdout=subprocess.PIPE, text=True, check=True)
        sys.stdout.write(res.stdout)
        sys.stdout.flush()
        lines += [l for l in res.stdout.splitlines() if ' | ' in l]
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
