#!/usr/bin/env python3
"""Rate of the Rician debias (amx_prep_debias_device) on a 300 000 x 99 image held in HBM, and for comparison the rate of a CPU
route on the same host: scipy's L-BFGS-B over all samples of one voxel (how the reference solves it) on this project's own statement
of the functional (scipy's `ive`, analytic gradient), a few hundred voxels.

    python tools/time_debias.py [--voxels 300000] [--cpu-voxels 200] [--snr 30]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--voxels', type=int, default=300000)
    ap.add_argument('--cpu-voxels', type=int, default=200)
    ap.add_argument('--snr', type=float, default=30.0)
    ap.add_argument('--reps', type=int, default=10)
    a = ap.parse_args()
    import torch
    from amico_amd import _capi, prep, synthetic as S
    nS, b0_idx = 99, np.arange(0, 99, 11)
    sch = S.SimpleScheme(np.column_stack([np.tile([1.0, 0.0, 0.0], (nS, 1)), np.where(np.isin(np.arange(nS), b0_idx), 0.0, 1000.0)]))
    rng = np.random.default_rng(0)
    shape = (100, 60, a.voxels // 6000)
    n = int(np.prod(shape))
    amp = rng.uniform(400.0, 1600.0, size=(n, 1))
    att = rng.uniform(0.0, 1.0, size=(n, nS)) ** 2
    att[:, b0_idx] = 1.0
    sg = amp / a.snr
    rows = np.abs(amp * att + sg * rng.standard_normal((n, nS)) + 1j * sg * rng.standard_normal((n, nS))).astype(np.float32)
    print(_capi.build_id())
    for order in ('F', 'C'):
        img = np.asarray(rows.reshape(shape + (nS,)), order=order)
        sp = prep.SignalPreparation(sch, img, np.ones(shape, dtype=np.uint8), do_normalize=False, debias_snr=a.snr)
        src = torch.from_numpy(np.array(sp._plan._img_buffer(img))).to('cuda')
        work = torch.empty_like(src)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ms = []
        for _ in range(a.reps + 2):
            work.copy_(src)
            ev[0].record()
            sp._plan.debias_device(work.data_ptr(), a.snr)
            ev[1].record()
            torch.cuda.synchronize()
            ms.append(ev[0].elapsed_time(ev[1]))
        ms = np.array(ms[2:])
        print(f'GPU  {order}-order image {n} voxels x {nS} samples, SNR {a.snr:g}: median {np.median(ms):.3f} ms (min {ms.min():.3f}, max {ms.max():.3f}, '
              f'{a.reps} runs), {n * nS / np.median(ms) * 1e3:.3e} samples/s, unconverged {sp.ctx.debias_last_unconverged()}')
    # the CPU route: scipy's L-BFGS-B over all samples of one voxel from E = S, the way the reference drives it (preproc.py:33), on this
    # project's own statement of the functional: mu from the exponentially scaled Bessel functions and its analytic derivative
    # mu'(e) = sqrt(pi/2) (e / 2 sigma) [I0e + I1e](e^2 / 4 sigma^2)   
    from scipy.optimize import minimize
    from scipy.special import ive

    def F_and_grad(E, y, sigma):
        x = E * E / (2.0 * sigma * sigma)
        i0, i1 = ive(0, 0.5 * x), ive(1, 0.5 * x)
        r = y - sigma * np.sqrt(np.pi / 2.0) * ((1.0 + x) * i0 + x * i1)
        return np.sum(r * r), -2.0 * r * (np.sqrt(np.pi / 2.0) * 0.5 * (E / sigma) * (i0 + i1))

    t = time.perf_counter()
    for i in range(a.cpu_voxels):
        y = rows[i].astype(np.float64)
        minimize(F_and_grad, y, args=(y, float(y[b0_idx].mean()) / a.snr), method='L-BFGS-B', jac=True)
    dt = time.perf_counter() - t
    print(f'CPU  scipy L-BFGS-B per voxel on the same functional (ive-based mu, analytic gradient), {a.cpu_voxels} voxels x {nS} samples: {dt / a.cpu_voxels * 1e3:.2f} ms per voxel, '
          f'{a.cpu_voxels * nS / dt:.3e} samples/s ({dt / a.cpu_voxels * n / 60.0:.0f} min for {n} voxels)')


if __name__ == '__main__':
    main()
