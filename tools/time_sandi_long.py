#!/usr/bin/env python3
"""SANDI without the directional average (csrc/amx_sandi_long.hip): the default acquisition, 306 volumes x 15 atoms, 1 M voxels, signals
resident in HBM.  One process per leg, device events, warm-up, median of 7; every leg runs twice, so the spread of the same leg is on
the page next to the differences between legs:

  float32-lane   float32 signals (the image's dtype), k_sandi_project<float> -> k_sandi_gram_lane<15>        (the default route)
  float64-lane   float64 signals
  float32-wave   AMX_WAVE_PER_VOXEL=1: k_sandi_project<float> -> k_sandi_gram_wave (the route of dictionaries of 17 .. 64 atoms)
  float64-wave

Per leg: ms per fit, voxels/s, and voxels/s x bytes of y per voxel / 8.0e12 -- the roofline form of BASELINE.md (1 224 B per voxel for
float32, 2 448 B for float64: y is the only stream that grows with the protocol), then the two kernels apart (amx_last_kernel_ms: 2 = the
projection, 1 = the solver) in a profiled fit of their own, which says which one dominates.  Every line starts with the library's
amx_build_id.

    python tools/time_sandi_long.py [--voxels 1000000] [--reps 7] [--leg NAME]      (no --leg: every leg twice, each in a process of its own)
"""
import argparse
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
LEGS = ('float32-lane', 'float64-lane', 'float32-wave', 'float64-wave')
HBM_PEAK = 8.0e12


def leg(name, n, reps):
    import torch
    from amico_amd import _capi, get_context, synthetic as S
    tag = _capi.build_id()
    dtype, route = name.split('-')
    sch = S.make_sandi_scheme()
    K, Rs, d_in, d_isos = S.sandi_kernels(sch)
    # 65 536 voxels made on the host, repeated on the device: the solver's work per voxel follows the signals, the repetition keeps their mix
    base = S.sandi_signals(min(n, 65536), K, sch, seed=1, navg=1)
    d_y = torch.from_numpy(base.astype(np.float32 if dtype == 'float32' else np.float64)).cuda()
    d_y = d_y.repeat(-(-n // d_y.shape[0]), 1)[:n].contiguous()
    ctx = get_context()
    lut = _capi.upload_sandi(ctx, K, Rs, d_in, d_isos)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for _ in range(reps + 2):                                  # two warm-up fits (tables, workspace), then the timed ones
        ev[0].record()
        _capi.sandi_fit_device(ctx, lut, d_y, 0.0, 5e-3)
        ev[1].record()
        torch.cuda.synchronize()
        ms.append(ev[0].elapsed_time(ev[1]))
    ctx.sync()
    path, st = ctx.last_path(), ctx.last_stats()
    t, lo, hi = float(np.median(ms[2:])), min(ms[2:]), max(ms[2:])
    bytes_y = sch.nS * d_y.element_size()
    rate = n / t * 1e3
    print(f'{tag} | {name}: SANDI {n} voxels x {sch.nS} volumes x {lut.n_atoms} atoms: median {t:.3f} ms (min {lo:.3f}, max {hi:.3f}, {reps} fits), '
          f'{rate / 1e6:.1f} M voxels/s, {bytes_y} B of y per voxel -> {100.0 * rate * bytes_y / HBM_PEAK:.1f} % of 8 TB/s '
          f'({rate * bytes_y / 1e12:.2f} TB/s of y)')
    ctx.set_profiling(True)
    _capi.sandi_fit_device(ctx, lut, d_y, 0.0, 5e-3)
    ctx.sync()
    proj, solv, whole = ctx.last_kernel_ms(2), ctx.last_kernel_ms(1), ctx.last_kernel_ms(0)
    ctx.set_profiling(False)
    print(f'{tag} | {name}: profiled fit {whole:.3f} ms = projection {proj:.3f} ms ({n * bytes_y / proj / 1e9:.2f} TB/s of y) + solver {solv:.3f} ms: '
          f'the {"projection" if proj > solv else "solver"} dominates [{path}] {st}')
    lut.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--voxels', type=int, default=1000000)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--leg', choices=LEGS)
    a = ap.parse_args()
    if a.leg:
        return leg(a.leg, a.voxels, a.reps)
    for k in (1, 2):                                           # the same legs twice: their spread
        for name in LEGS:                                      # a fresh child process per leg (the switch is read when a context is made)
            env = dict(os.environ)
            env.pop('AMX_WAVE_PER_VOXEL', None)
            if name.endswith('wave'):
                env['AMX_WAVE_PER_VOXEL'] = '1'
            print(f'run {k}:', flush=True)
            subprocess.check_call([sys.executable, os.path.abspath(__file__), '--voxels', str(a.voxels), '--reps', str(a.reps), '--leg', name],
                                  env=env, timeout=280)        # (a leg that hangs ends the run; a failed one does too: check_call)


if __name__ == '__main__':
    main()
