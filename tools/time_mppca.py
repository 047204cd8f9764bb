#!/usr/bin/env python3
"""The Marchenko-Pastur noise estimator (amico_amd/noise.py, csrc/amx_mppca.hip): 300 000 masked voxels of a 100 x 100 x 60 image
(the half x < 50, so that every cube inside it is full and those at its face hold three fifths), float32 in HBM, planar (the volume axis
slowest: nibabel's Fortran order), one process per leg, median of 7, device events:

  v99_w3, v99_w5      99 volumes (9 b0), patch edge 3 | 5
  v306_w3, v306_w5    306 volumes (9 b0)
  split               w = 5 at 125, 250 and 500 volumes on 60 000 voxels: r = 125 in all three, so the eigenvalue stage costs the same and the
                      staging + Gram stage grows with q = the volumes -- the line through the three times gives the two parts

  den_v99_w3 .. den_v306_w5   the denoiser on the four images above: k_mppca alone and k_mppca_denoise behind its device copy
                      of the image, in the same process, and the whole of noise.denoise_mppca_device

Per leg: k_mppca, the b0 estimator's k_noise_b0 on the same image, and the whole estimate as Evaluation.fit() runs it (one launch, two
medians, the small copy home).  Every line starts with the library's amx_build_id.

    python tools/time_mppca.py [--reps 7] [--leg NAME]      (no --leg: every leg, each in a process of its own)
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
LEGS = ('v99_w3', 'v99_w5', 'v306_w3', 'v306_w5', 'split', 'den_v99_w3', 'den_v99_w5', 'den_v306_w3', 'den_v306_w5')
SHAPE, N_B0 = (100, 100, 60), 9
SHELLS = {99: ((700.0, 30), (2000.0, 60)), 306: ((700.0, 99), (2000.0, 198)), 125: ((1000.0, 116),), 250: ((1000.0, 241),), 500: ((1000.0, 491),)}


def setup(nS, x_hi):
    import torch
    from amico_amd import _capi, get_context, prep, synthetic as S
    sch = S.make_scheme(N_B0, SHELLS[nS], seed=0)
    assert sch.nS == nS
    total = int(np.prod(SHAPE))
    strides = (1, SHAPE[0], SHAPE[0] * SHAPE[1], total)
    mask = np.zeros(SHAPE, dtype=np.uint8)
    mask[:x_hi] = 1
    rank = np.full(SHAPE, -1, dtype=np.int32)
    rank[mask == 1] = np.arange(int(mask.sum()), dtype=np.int32)
    ctx = get_context()
    plan = _capi.Prep(ctx, SHAPE + (nS,), strides, rank, prep.volume_groups(sch), sch.b0_idx)
    g = torch.Generator(device='cuda').manual_seed(1)
    # volumes of different brightness (a rank-one signal) plus noise of standard deviation 45
    level = 900.0 * torch.linspace(1.0, 0.3, nS, device='cuda').repeat_interleave(total)
    d_img = (level + 45.0 * torch.randn(plan.extent, generator=g, device='cuda', dtype=torch.float32)).abs_()
    return ctx, plan, d_img


def events(fn, reps):
    import torch
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for _ in range(reps + 2):
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        ms.append(ev[0].elapsed_time(ev[1]))
    return float(np.median(ms[2:])), min(ms[2:]), max(ms[2:])


def leg(name, reps):
    import torch
    from amico_amd import _capi, noise
    tag = _capi.build_id()
    if name == 'split':
        pts = []
        for nS in (125, 250, 500):
            ctx, plan, d_img = setup(nS, 10)
            out = torch.empty((4, plan.n_vox), dtype=torch.float64, device='cuda')
            t, lo, hi = events(lambda: plan.noise_mppca_device(d_img.data_ptr(), 5, *[out[i].data_ptr() for i in range(4)]), reps)
            rt = _capi.mppca_route(nS, 5, 125, SHAPE)
            print(f'{tag} | split: {plan.n_vox} voxels, {nS} volumes, w 5, r {rt["r"]}, q {rt["q"]} | k_mppca<5>: median {t:.2f} ms (min {lo:.2f}, max {hi:.2f}), '
                  f'{1e3 * t / plan.n_vox:.2f} us per voxel')
            pts.append((nS, 1e3 * t / plan.n_vox))
            plan.close()
            del d_img
        slope, icpt = np.polyfit([p[0] for p in pts], [p[1] for p in pts], 1)
        print(f'{tag} | split: line through the three: {icpt:.2f} us per voxel that do not grow with q (tridiagonalisation, bisection, the rule) + '
              f'{1e3 * slope:.2f} ns per voxel and volume (staging and Gram matrix): at q = 125 the second part is {100 * slope * 125 / (icpt + slope * 125):.0f} % '
              f'of the time, at q = 306 {100 * slope * 306 / (icpt + slope * 306):.0f} %')
        return
    if name.startswith('den_'):
        return denoise_leg(name, reps)
    nS, w = int(name[1:name.index('_')]), int(name[-1])
    ctx, plan, d_img = setup(nS, 50)
    n = plan.n_vox
    rt = _capi.mppca_route(nS, w, w ** 3, SHAPE)
    head = f'{tag} | {name}: {n} masked voxels of {int(np.prod(SHAPE))}, {nS} volumes, w {w}, r {rt["r"]}, q {rt["q"]}, Gram over the {rt["side"]} |'
    out = torch.empty((4, n), dtype=torch.float64, device='cuda')
    t, lo, hi = events(lambda: plan.noise_mppca_device(d_img.data_ptr(), w, *[out[i].data_ptr() for i in range(4)]), reps)
    flop = 2.0 * rt['r'] * rt['r'] * rt['q'] / 2 + 2.0 * rt['r'] ** 3 + 56 * 3.0 * rt['r'] ** 2      # Gram (lower triangle), Householder (full storage), bisection
    print(f'{head} k_mppca<{w}> [{rt["waves"]} wavefronts per patch, {rt["patches"]} per workgroup, {rt["lds"]} B LDS]: median {t:.2f} ms '
          f'(min {lo:.2f}, max {hi:.2f}), {1e3 * t / n:.3f} us per voxel, about {flop / 1e6:.2f} MFLOP per voxel: {flop * n / t / 1e9:.2f} TFLOP/s')
    tb, lo, hi = events(lambda: plan.noise_b0_device(d_img.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr()), reps)
    print(f'{head} k_noise_b0 (the b0 estimator, same image): median {tb:.3f} ms (min {lo:.3f}, max {hi:.3f}); k_mppca / k_noise_b0 = {t / tb:.0f}')
    s = []
    for _ in range(reps + 2):
        ctx.sync()
        t0 = time.perf_counter()
        est = noise.estimate_mppca_device(plan, d_img.data_ptr(), w)
        ctx.sync()
        s.append((time.perf_counter() - t0) * 1e3)
    print(f'{head} the whole estimate (host clock: launch, two medians, the copy home and its wait): median {np.median(s[2:]):.2f} ms '
          f'(min {min(s[2:]):.2f}, max {max(s[2:]):.2f}); sigma {est["sigma"]:.3f} (made at 45), SNR {est["snr"]:.3f} (made at 20), {est["voxels"]} voxels')
    tb0 = []
    for _ in range(reps + 2):
        ctx.sync()
        t0 = time.perf_counter()
        est0 = noise.estimate_device(plan, d_img.data_ptr())
        ctx.sync()
        tb0.append((time.perf_counter() - t0) * 1e3)
    print(f'{head} the b0 estimator\'s whole estimate: median {np.median(tb0[2:]):.3f} ms; sigma {est0["sigma"]:.3f}, SNR {est0["snr"]:.3f}')


def denoise_leg(name, reps):
    import torch
    from amico_amd import _capi, noise
    tag = _capi.build_id()
    nS, w = int(name[5:name.rindex('_')]), int(name[-1])
    ctx, plan, d_img = setup(nS, 50)
    n = plan.n_vox
    rt = _capi.mppca_denoise_route(nS, w, w ** 3, SHAPE)
    head = f'{tag} | {name}: {n} masked voxels of {int(np.prod(SHAPE))}, {nS} volumes, w {w}, r {rt["r"]}, q {rt["q"]}, Gram over the {rt["side"]} |'
    out = torch.empty((4, n), dtype=torch.float64, device='cuda')
    image = torch.empty(plan.extent, dtype=torch.float32, device='cuda')
    status = torch.empty(n, dtype=torch.int32, device='cuda')
    t, lo, hi = events(lambda: plan.noise_mppca_device(d_img.data_ptr(), w, *[out[i].data_ptr() for i in range(4)]), reps)
    print(f'{head} k_mppca<{w}> alone: median {t:.2f} ms (min {lo:.2f}, max {hi:.2f}), {1e3 * t / n:.3f} us per voxel')
    td, lo, hi = events(lambda: plan.noise_mppca_denoise_device(d_img.data_ptr(), w, image.data_ptr(), *[out[i].data_ptr() for i in range(4)],
                                                                status.data_ptr()), reps)
    signal = out[1][~torch.isnan(out[1])]
    print(f'{head} the image copy + k_mppca_denoise<{w}> [{rt["lds"]} B LDS, {rt["capacity"]} vectors, cap {rt["cap"]}]: median {td:.2f} ms (min {lo:.2f}, '
          f'max {hi:.2f}), {1e3 * td / n:.3f} us per voxel; over k_mppca {td / t:.3f}; n_signal {int(signal.min())}..{int(signal.max())}, '
          f'{int((status == 0).sum())} voxels denoised')
    tc, lo, hi = events(lambda: image.copy_(d_img), reps)
    print(f'{head} the copy of the image alone ({4 * plan.extent / 1e6:.0f} MB): median {tc:.2f} ms')
    s = []
    for _ in range(reps + 2):
        ctx.sync()
        t0 = time.perf_counter()
        den = noise.denoise_mppca_device(plan, d_img.data_ptr(), w)
        ctx.sync()
        s.append((time.perf_counter() - t0) * 1e3)
    print(f'{head} the whole of denoise_mppca_device (host clock: buffers, copy, launch, two medians, the copies home): median {np.median(s[2:]):.2f} ms; '
          f'sigma {den["sigma"]:.3f} (made at 45), {den["denoised"]} denoised, {den["passed_through"]} passed through')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--leg', choices=LEGS)
    a = ap.parse_args()
    if a.leg:
        return leg(a.leg, a.reps)
    for name in LEGS:                                       # a fresh child process per leg
        subprocess.check_call([sys.executable, os.path.abspath(__file__), '--reps', str(a.reps), '--leg', name], timeout=280)


if __name__ == '__main__':
    main()
