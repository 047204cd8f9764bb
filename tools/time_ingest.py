#!/usr/bin/env python3
"""What taking the DWI image in its stored dtype buys: 300 000 masked of 360 000 voxels, the 99-volume NODDI image and the 65-volume
Free-Water one (DESIGN section 7d's geometry), one process per leg, each under its own time limit, median of 7 after a warm-up.

  e2e      Evaluation.set_data() + Evaluation.fit() wall time from the stored array to RESULTS, for int16 + scaling, float64 and float32
           input.  On a tree without the feature (--compare-root: a checkout of the parent commit, built) the stored array goes
           through the numpy expression first -- np.float32(np.float64(raw) * slope + inter) / raw.astype(np.float32) -- inside the
           timed region, which is what a caller had to do there.  Trees alternate: this, other, this, other.
  kernel   k_ingest<...> alone for every dtype (HIP events), beside k_sanitize_flat<f32> on the float32 image of the same geometry

    python tools/time_ingest.py [--compare-root variants/parent] [--reps 7] [--images noddi99 fw65]
"""
import argparse
import inspect
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPE = (100, 60, 60)
N_MASKED = 300000
SCALING = (0.05, -3.5)


def make_image(S, image, htable):
    """-> (scheme, kernels, model name, float64 signals [X, Y, Z, nS] in Fortran order, mask)"""
    dirs, ht = htable
    if image == 'noddi99':
        sch = S.make_scheme(seed=0)
        K = S.noddi_kernels(sch, dirs)
        y, _ = S.noddi_signals(20000, K, ht, sch, seed=6)
        model = 'NODDI'
    else:
        sch = S.make_scheme(5, ((1000.0, 60),), seed=3)
        K = S.freewater_kernels(sch, dirs)
        y, _ = S.freewater_signals(20000, K, ht, sch, seed=1)
        model = 'FreeWater'
    n_total = int(np.prod(SHAPE))
    mask = np.zeros(n_total, dtype=np.uint8)
    mask[np.random.default_rng(0).permutation(n_total)[:N_MASKED]] = 1
    sig = np.empty((sch.nS, n_total))                       # Fortran order of [X, Y, Z, nS], as nibabel hands it out
    sig[:] = (y[np.arange(n_total) % len(y)] * 800.0).T
    sig = sig.reshape((sch.nS,) + SHAPE[::-1]).transpose(3, 2, 1, 0)
    assert sig.flags.f_contiguous
    return sch, K, model, sig, mask.reshape(SHAPE)


def stored(sig, dtype):
    if dtype == 'int16':
        return np.rint((sig - SCALING[1]) / SCALING[0]).astype(np.int16), SCALING
    if dtype == 'float64':
        return sig, None
    return sig.astype(np.float32), None


def leg_e2e(a):
    sys.path.insert(0, a.root)
    import torch
    import amico_amd
    from amico_amd import _capi, synthetic as S
    dirs = S.fibonacci_hemisphere(500)
    ht = S.build_htable(dirs)
    sch, K, model, sig, mask = make_image(S, a.image, (dirs, ht))
    raw, scaling = stored(sig, a.dtype)
    del sig
    has = 'scaling' in inspect.signature(amico_amd.Evaluation.set_data).parameters
    t_set, t_fit = [], []
    for _ in range(a.reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ae = amico_amd.Evaluation()
        if has:
            ae.set_data(raw, sch, mask, scaling=scaling)
        else:
            with np.errstate(over='ignore'):
                img = raw.astype(np.float32, copy=False) if scaling is None else (raw.astype(np.float64) * scaling[0] + scaling[1]).astype(np.float32)
            ae.set_data(img, sch, mask)
        t1 = time.perf_counter()
        ae.set_model(model)
        ae.set_kernels(K, ht)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        ae.fit()
        t3 = time.perf_counter()
        t_set.append((t1 - t0) * 1e3)
        t_fit.append((t3 - t2) * 1e3)
    tot = np.add(t_set, t_fit)[1:]
    print(json.dumps({'leg': 'e2e', 'image': a.image, 'dtype': a.dtype, 'build': _capi.build_id(), 'feature': has,
                      'set_data_ms': round(float(np.median(t_set[1:])), 2), 'fit_ms': round(float(np.median(t_fit[1:])), 2),
                      'total_ms': round(float(np.median(tot)), 2), 'min_ms': round(float(tot.min()), 2), 'max_ms': round(float(tot.max()), 2),
                      'bad_samples_raw': ae.get_config('bad_samples_raw')}))


def leg_kernel(a):
    sys.path.insert(0, a.root)
    import torch
    from amico_amd import _capi, prep, synthetic as S
    nS = 99 if a.image == 'noddi99' else 65
    b = np.where(np.arange(nS) % 11 == 0, 0.0, 1000.0)
    sch = S.SimpleScheme(np.column_stack([np.tile([1.0, 0.0, 0.0], (nS, 1)), b]))
    shape = SHAPE + (nS,)
    n = int(np.prod(shape))
    mask = np.ones(SHAPE, dtype=np.uint8)
    rng = np.random.default_rng(0)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def events(fn):
        ms = []
        for _ in range(a.reps + 2):
            ev[0].record()
            fn()
            ev[1].record()
            torch.cuda.synchronize()
            ms.append(ev[0].elapsed_time(ev[1]))
        return float(np.median(ms[2:]))
    out = {'leg': 'kernel', 'image': a.image, 'build': _capi.build_id(), 'elements': n, 'kernels': {}}
    d_img = torch.empty(n, dtype=torch.float32, device='cuda')
    for dt in (np.uint8, np.int16, np.uint16, np.int32, np.float32, np.float64):
        dt = np.dtype(dt)
        raw = rng.integers(0, 200, size=n).astype(dt)
        sp = prep.SignalPreparation(sch, raw.reshape(shape, order='F'), mask, do_normalize=False)
        d_raw = torch.from_numpy(raw.view(np.uint8)).cuda()
        for scaling in (None, SCALING):
            ms = events(lambda: sp._plan.ingest_device(d_raw.data_ptr(), dt, d_img.data_ptr(), scaling, 0.0))
            assert sp.ctx.sanitize_last() == 0
            out['kernels']['k_ingest<%s%s>' % (dt.name, ',scaled' if scaling else '')] = {'ms': round(ms, 4), 'GB_per_s': round(n * (dt.itemsize + 4) / ms / 1e6, 1)}
        del d_raw
    ms = events(lambda: sp._plan.sanitize_device(d_img.data_ptr(), 0.0))
    out['kernels']['k_sanitize_flat<f32> (clean image: read only)'] = {'ms': round(ms, 4), 'GB_per_s': round(n * 4 / ms / 1e6, 1)}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--leg', choices=['e2e', 'kernel'])
    ap.add_argument('--image', default='noddi99')
    ap.add_argument('--images', nargs='+', default=['noddi99', 'fw65'])
    ap.add_argument('--dtype', default='int16')
    ap.add_argument('--root', default=os.path.join(HERE, '..'))
    ap.add_argument('--compare-root', default=None)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--leg-timeout', type=int, default=150)
    a = ap.parse_args()
    if a.leg == 'e2e':
        return leg_e2e(a)
    if a.leg == 'kernel':
        return leg_kernel(a)
    me = os.path.abspath(__file__)
    roots = [os.path.abspath(a.root)] + ([os.path.abspath(a.compare_root)] if a.compare_root else [])

    def run(args):
        # a fresh process per leg, under its own time limit; a leg that fails ends the run (nothing more is started on the GPU)
        r = subprocess.run(['timeout', '-k', '10', str(a.leg_timeout), sys.executable, me, '--reps', str(a.reps)] + args,
                           stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            sys.exit('leg %s ended with status %d' % (' '.join(args), r.returncode))
        print(r.stdout.strip().splitlines()[-1], flush=True)
    for image in a.images:
        run(['--leg', 'kernel', '--image', image, '--root', roots[0]])
        for dtype in ('int16', 'float64', 'float32'):
            for _ in range(2):
                for root in roots:
                    run(['--leg', 'e2e', '--image', image, '--dtype', dtype, '--root', root])


if __name__ == '__main__':
    main()
