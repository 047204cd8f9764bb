#!/usr/bin/env python3
"""The wild bootstrap (amico_amd/bootstrap.py, csrc/amx_bootstrap.hip), 300 000 voxels in HBM as Evaluation.fit() holds them (float32
signals, float64 directions), one process per leg, median of 7:

  noddi       99 volumes, 145 atoms      freewater   65 volumes, 11 atoms

Per leg: k_boot_resample alone beside k_fw_corrected (rows form) on the same geometry -- the project's streaming yardstick, here on a
Free-Water dictionary of the leg's scheme --, the accumulate step, and the time per replicate of the driver beside a plain
`*_fit_device` of the same size in the same process (the overhead ratio).  Every line starts with the library's amx_build_id.

    python tools/time_bootstrap.py [--voxels 300000] [--reps 7] [--samples 20] [--leg NAME]     (no --leg: every leg, each in a process of its own)
    python tools/time_bootstrap.py --bench PARENT      bench.py plain NODDI in the built checkout of the parent commit under PARENT and in
                                                       this tree, alternating (twice each), ms per step of every run; then
                                                       --dump-outputs of both, compared byte for byte
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
LEGS = ('noddi', 'freewater')
ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


def leg(model, n, reps, samples):
    import torch
    from amico_amd import _capi, bootstrap, get_context, synthetic as S
    tag = _capi.build_id()
    dirs = S.fibonacci_hemisphere(500)
    ht = S.build_htable(dirs)
    if model == 'noddi':
        sch = S.make_scheme(seed=0)
        K = S.noddi_kernels(sch, dirs)
        y, d = S.noddi_signals_parallel(n, K, ht, sch, seed=1)
        lambdas, extras = (0.5, 1e-3), (3,)
    else:
        sch = S.make_scheme(5, ((1000.0, 60),), seed=3)
        K = S.freewater_kernels(sch, dirs)
        y, d = S.freewater_signals(n, K, ht, sch, seed=1)
        lambdas, extras = (0.0, 1e-3), (0,)
    ctx = get_context()
    lut = _capi.upload_noddi(ctx, K, ht, sch.dwi_idx) if model == 'noddi' else _capi.upload_freewater(ctx, K, ht)
    row = _capi.FIT[model]
    nS = sch.nS
    d_y, d_dirs = torch.from_numpy(y.astype(np.float32)).cuda(), torch.from_numpy(d).cuda()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def events(fn):
        ms = []
        for _ in range(reps + 2):
            ev[0].record()
            fn()
            ev[1].record()
            torch.cuda.synchronize()
            ms.append(ev[0].elapsed_time(ev[1]))
        return float(np.median(ms[2:])), min(ms[2:]), max(ms[2:])

    def fit(**k):
        return _capi._fit_device(row, ctx, lut, d_y, d_dirs, *lambdas, extras, {}, None, k.get('return_x', False), False, into=k.get('into'))
    x = fit(return_x=True)[-1]
    y_est = _capi.predict_device(ctx, lut, x, d_dirs)
    ctx.sync()
    # ---- the kernels alone
    y_b = torch.empty_like(d_y)
    t, lo, hi = events(lambda: _capi.bootstrap_resample_device(ctx, d_y, y_est, 0, 1, into=y_b))
    gb = n * nS * (4 + 8 + 4) / 1e9
    print(f'{tag} | k_boot_resample<float> {model} {n} voxels x {nS}: median {t:.3f} ms (min {lo:.3f}, max {hi:.3f}), {gb / t * 1e3:.0f} GB/s '
          f'of y + y_est + y_b traffic ({gb * 1e3:.0f} MB)')
    fw = lut if model == 'freewater' else _capi.upload_freewater(ctx, S.freewater_kernels(sch, dirs), ht)
    xi = torch.rand((n, fw.n_iso), dtype=torch.float64, device='cuda') * 0.3
    yc = torch.empty((n, nS), dtype=torch.float64, device='cuda')
    tc, lo, hi = events(lambda: _capi.freewater_corrected_device(ctx, fw, d_y, xi, into=yc))
    gbc = n * (nS * (4 + 8) + 8 * fw.n_iso) / 1e9
    print(f'{tag} | k_fw_corrected (rows form) on the same geometry: median {tc:.3f} ms (min {lo:.3f}, max {hi:.3f}), {gbc / tc * 1e3:.0f} GB/s '
          f'of y + x_iso + y_corrected traffic ({gbc * 1e3:.0f} MB); k_boot_resample / k_fw_corrected = {t / tc:.2f}')
    est = torch.empty((n,) + row.outputs[0].shape(lut, extras), dtype=torch.float64, device='cuda')
    mean, m2 = torch.empty_like(est), torch.empty_like(est)
    fit(into=est)
    _capi.bootstrap_accumulate_device(ctx, est, 1, mean, m2)
    ta, lo, hi = events(lambda: _capi.bootstrap_accumulate_device(ctx, est, 2, mean, m2))
    print(f'{tag} | k_boot_accumulate {n} voxels x {est.shape[1]} maps: median {ta:.3f} ms (min {lo:.3f}, max {hi:.3f}), '
          f'{est.numel() * 8 * 5 / ta * 1e-6:.0f} GB/s of maps + moments traffic')
    # ---- a replicate of the driver beside a plain fit, host clock around work that ends in a synchronise
    def clock(fn, count):
        s = []
        for _ in range(reps + 2):
            ctx.sync()
            t0 = time.perf_counter()
            fn()
            ctx.sync()
            s.append((time.perf_counter() - t0) * 1e3 / count)
        return float(np.median(s[2:])), min(s[2:]), max(s[2:])
    tf, lo, hi = clock(lambda: [fit(into=est) for _ in range(samples)], samples)
    print(f'{tag} | plain {model} fit_device, {n} voxels x {nS}, {samples} in a row: median {tf:.3f} ms per fit (min {lo:.3f}, max {hi:.3f})   '
          f'[{ctx.last_path()}]')
    tb, lo, hi = clock(lambda: bootstrap.wild_bootstrap(ctx, row, lut, d_y, d_dirs, *lambdas, extras, x, samples), samples)
    print(f'{tag} | wild_bootstrap, {samples} replicates (+ one prediction, the std): median {tb:.3f} ms per replicate (min {lo:.3f}, '
          f'max {hi:.3f}); replicate / plain fit = {tb / tf:.2f}; {samples} replicates of {n} voxels: {tb * samples:.1f} ms')


def bench_ab(parent):
    """bench.py in the parent's built checkout and in this tree, alternating; then the dumped maps of both, byte for byte"""
    import filecmp
    import json
    import tempfile
    base = [sys.executable, 'bench.py', '--gpus', '1', '--steps', '20', '--warmup', '3', '--no-cpu-baseline', '--no-other-configs']
    trees = (('parent', os.path.abspath(parent)), ('this', ROOT))
    for k in (1, 2):
        for who, cwd in trees:
            with open(os.devnull, 'w') as null:
                line = subprocess.check_output(base, cwd=cwd, stderr=null, timeout=280).decode().strip().splitlines()[-1]
            d = json.loads(line)
            flat = {key: v for key, v in d.items() if not isinstance(v, (dict, list)) and key in ('metric', 'value', 'unit', 'ms_per_step', 'vs_baseline')}
            print('noddi %-6s run %d: %s' % (who, k, flat), flush=True)
    with tempfile.TemporaryDirectory() as tmp:
        for who, cwd in trees:
            with open(os.devnull, 'w') as null:
                subprocess.check_call(base[:4] + ['--steps', '2', '--warmup', '1', '--no-cpu-baseline', '--no-other-configs', '--dump-outputs',
                                                  os.path.join(tmp, who)], cwd=cwd, stdout=null, stderr=null, timeout=280)
        names = sorted(os.listdir(os.path.join(tmp, 'parent')))
        same = [filecmp.cmp(os.path.join(tmp, 'parent', f), os.path.join(tmp, 'this', f), shallow=False) for f in names]
        print('--dump-outputs: %s; parent and this tree byte for byte: %s' % (
            ', '.join('%s (%d bytes)' % (f, os.path.getsize(os.path.join(tmp, 'parent', f))) for f in names),
            'identical' if names and all(same) and names == sorted(os.listdir(os.path.join(tmp, 'this'))) else 'DIFFERENT'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--voxels', type=int, default=300000)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--samples', type=int, default=20)
    ap.add_argument('--leg', choices=LEGS)
    ap.add_argument('--bench', metavar='PARENT')
    a = ap.parse_args()
    if a.leg:
        return leg(a.leg, a.voxels, a.reps, a.samples)
    if a.bench:
        return bench_ab(a.bench)
    for name in LEGS:                                       # a fresh child process per leg
        subprocess.check_call([sys.executable, os.path.abspath(__file__), '--voxels', str(a.voxels), '--reps', str(a.reps), '--samples', str(a.samples),
                               '--leg', name], timeout=280)     # (a leg that hangs ends the run; a failed one does too: check_call)


if __name__ == '__main__':
    main()
