#!/usr/bin/env python3
"""The noise estimate from the b0 repeats (amico_amd/noise.py, csrc/amx_noise.hip): 300 000 masked voxels of a 100 x 100 x 60
image (every second voxel), 99 volumes of which 9 are b0, float32 in HBM, one process per leg, median of 7:

  planar           the volume axis is the slowest (nibabel's Fortran order): a b0 volume of consecutive voxels is one run of memory
  volume_fastest   C order: the 99 samples of a voxel are consecutive, every b0 sample of a voxel is a line of its own

Per leg: k_noise_b0 beside amx_prep_mean_b0_device on the same image (it reads the same samples: the yardstick of the per-voxel kernel),
one exact median and its bytes per pass, the whole estimate as Evaluation.fit() runs it (one launch, two medians, the small copy home),
and the mask gather of the same plan, which every fit runs anyway.  Every line starts with the library's amx_build_id.

    python tools/time_noise.py [--reps 7] [--leg NAME]      (no --leg: every leg, each in a process of its own)
    python tools/time_noise.py --bench PARENT               bench.py plain NODDI in the built checkout of the parent commit under PARENT
                                                            and in this tree, alternating; then --dump-outputs of both, byte for byte
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
LEGS = ('planar', 'volume_fastest')
SHAPE, N_B0 = (100, 100, 60), 9


def leg(name, reps):
    import torch
    from amico_amd import _capi, get_context, noise, prep, synthetic as S
    tag = _capi.build_id()
    sch = S.make_scheme(N_B0, seed=0)
    nS = sch.nS
    shape = SHAPE + (nS,)
    total = int(np.prod(SHAPE))
    if name == 'planar':
        strides = (1, SHAPE[0], SHAPE[0] * SHAPE[1], total)
    else:
        strides = (SHAPE[1] * SHAPE[2] * nS, SHAPE[2] * nS, nS, 1)
    mask = np.zeros(SHAPE, dtype=np.uint8)
    mask.reshape(-1)[::2] = 1
    rank = np.full(SHAPE, -1, dtype=np.int32)
    rank[mask == 1] = np.arange(int(mask.sum()), dtype=np.int32)
    ctx = get_context()
    plan = _capi.Prep(ctx, shape, strides, rank, prep.volume_groups(sch), sch.b0_idx)
    n = plan.n_vox
    g = torch.Generator(device='cuda').manual_seed(1)
    d_img = (900.0 * (1.0 + 0.05 * torch.randn(plan.extent, generator=g, device='cuda', dtype=torch.float32))).abs_()
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

    head = f'{tag} | {name}: {n} masked voxels of {total}, {nS} volumes, {N_B0} b0 |'
    out = torch.empty((3, n), dtype=torch.float64, device='cuda')
    t, lo, hi = events(lambda: plan.noise_b0_device(d_img.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr()))
    mb = (n * (N_B0 * 4 + 24) + total * 4) / 1e6
    print(f'{head} k_noise_b0: median {t:.3f} ms (min {lo:.3f}, max {hi:.3f}), {mb / t:.0f} GB/s of b0 samples + rank + three outputs ({mb:.1f} MB)')
    d_vol = torch.empty(SHAPE, dtype=torch.float32, device='cuda')
    tm, lo, hi = events(lambda: plan.mean_b0_device(d_img.data_ptr(), d_vol.data_ptr()))
    mbm = total * (N_B0 * 4 + 4) / 1e6
    print(f'{head} k_mean_b0 (every voxel, float32): median {tm:.3f} ms (min {lo:.3f}, max {hi:.3f}), {mbm / tm:.0f} GB/s of b0 samples + output '
          f'({mbm:.1f} MB); k_noise_b0 / k_mean_b0 = {t / tm:.2f}')
    words = torch.empty(6, dtype=torch.float64, device='cuda')
    t1, lo, hi = events(lambda: _capi.nanmedian_device(ctx, out[2].data_ptr(), n, words.data_ptr(), words.data_ptr() + 32))
    passes = 6                                   # kMedPasses of csrc/amx_noise.hip: five digits of 11 bits and one of 9
    print(f'{head} one exact median of {n} values ({passes} passes of k_median_hist + k_median_pick): median {t1:.3f} ms (min {lo:.3f}, '
          f'max {hi:.3f}); {n * 8 / 1e6:.1f} MB read per pass, {n * 8 * passes / 1e6 / t1:.0f} GB/s over the call')
    t2, lo, hi = events(lambda: noise._medians(ctx, out[2], out[1], words))
    print(f'{head} the two medians: median {t2:.3f} ms (min {lo:.3f}, max {hi:.3f})')

    def clock(fn):
        s = []
        for _ in range(reps + 2):
            ctx.sync()
            t0 = time.perf_counter()
            fn()
            ctx.sync()
            s.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(s[2:])), min(s[2:]), max(s[2:])
    te, lo, hi = clock(lambda: noise.estimate_device(plan, d_img.data_ptr()))
    est = noise.estimate_device(plan, d_img.data_ptr())
    print(f'{head} the whole estimate (host clock: launch, two medians, the copy home and its wait, the buffers): median {te:.3f} ms '
          f'(min {lo:.3f}, max {hi:.3f}); SNR {est["snr"]:.3f} (made at 20), sigma {est["sigma"]:.3f} (made at 45), {est["voxels"]} voxels')
    d_y = torch.empty((n, nS), dtype=torch.float32, device='cuda')
    d_mb0 = torch.empty(n, dtype=torch.float32, device='cuda')
    tg, lo, hi = events(lambda: plan.gather_device(d_img.data_ptr(), d_y.data_ptr(), d_mb0.data_ptr(), True))
    print(f'{head} the mask gather of the same plan [{plan.last_launch()[0]}]: median {tg:.3f} ms (min {lo:.3f}, max {hi:.3f}); '
          f'(k_noise_b0 + two medians) / gather = {(t + t2) / tg:.2f}')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--leg', choices=LEGS)
    ap.add_argument('--bench', metavar='PARENT')
    a = ap.parse_args()
    if a.leg:
        return leg(a.leg, a.reps)
    if a.bench:
        from time_bootstrap import bench_ab          # the same alternating A/B of bench.py and its dumped maps
        return bench_ab(a.bench)
    for name in LEGS:                                       # a fresh child process per leg
        subprocess.check_call([sys.executable, os.path.abspath(__file__), '--reps', str(a.reps), '--leg', name], timeout=280)


if __name__ == '__main__':
    main()
