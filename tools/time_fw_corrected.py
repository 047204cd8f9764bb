#!/usr/bin/env python3
"""Free-Water's corrected DWI volume, 300 000 masked voxels x 65 volumes, one process, median of 7:

  kernel   amx_prep_corrected_device alone (HIP events), beside k_prep_gather's rate on the same geometry
  (a)      the route before AMX_F_FW_ISO: fit with corrected=True (k_freewater_lane on a widened copy), the f64 rows and y to the
           host, two numpy passes, the host-array scatter (upload, scatter, download)
  (b)      fused fit with x_iso, the volume kernel, one copy home

Both routes start where Evaluation.fit() stands after the gather: y float32, directions and mean_b0 in HBM.

    python tools/time_fw_corrected.py [--voxels 300000] [--reps 7]
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
    ap.add_argument('--reps', type=int, default=7)
    a = ap.parse_args()
    import torch
    from amico_amd import _capi, prep, synthetic as S
    dirs = S.fibonacci_hemisphere(500)
    ht = S.build_htable(dirs)
    sch = S.make_scheme(5, ((1000.0, 60),), seed=3)
    K = S.freewater_kernels(sch, dirs)
    n, nS = a.voxels, sch.nS
    shape = (100, 60, -(-n * 6 // 5 // 6000))               # a sixth of the volume is background
    mask = np.zeros(int(np.prod(shape)), dtype=np.uint8)
    mask[np.random.default_rng(0).permutation(mask.size)[:n]] = 1
    mask = mask.reshape(shape)
    y, d = S.freewater_signals(n, K, ht, sch, seed=1)
    img = np.zeros(shape + (nS,), dtype=np.float32)
    img[mask == 1] = (y * 700.0).astype(np.float32)
    sp = prep.SignalPreparation(sch, img, mask)
    ctx, plan = sp.ctx, sp._plan
    lut = _capi.upload_freewater(ctx, K, ht)
    L = _capi.lib()
    print(_capi.build_id())
    d_img = torch.from_numpy(plan._img_buffer(img)).cuda()
    d_y = torch.empty((n, nS), dtype=torch.float32, device='cuda')
    d_mb0 = torch.empty(n, dtype=torch.float32, device='cuda')
    d_dirs = torch.from_numpy(d).cuda()
    vol = torch.empty(shape + (nS,), dtype=torch.float32, device='cuda')
    b0 = sch.b0_idx
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

    t_g = events(lambda: ctx.check(L.amx_prep_gather_device_f32(ctx._h, plan._h, d_img.data_ptr(), 1, 0.0, d_y.data_ptr(), d_mb0.data_ptr(), None)))
    x_iso = _capi.freewater_fit_device(ctx, lut, d_y, d_dirs, 0.0, 1e-3, False, iso=True)[-1]
    ctx.sync()
    t_c = events(lambda: plan.corrected_device(lut, d_y, x_iso, vol, d_mb0, b0))
    gb_g = (img.size * 4 + n * nS * 4) / 1e9                # image read (background included), y written
    gb_c = (n * nS * 4 + n * 12 + vol.numel() * 4) / 1e9    # y, x_iso and mean_b0 read, volume written
    print(f'k_prep_gather    {n} masked of {mask.size} voxels x {nS}: {t_g:.3f} ms, {gb_g / t_g * 1e3:.0f} GB/s, {n / t_g * 1e-6:.2f} G voxels/s')
    print(f'k_fw_corrected   (volume form, rescale + keep b0): {t_c:.3f} ms, {gb_c / t_c * 1e3:.0f} GB/s, {n / t_c * 1e-6:.2f} G voxels/s')

    def route_a():
        yc = _capi.freewater_fit_device(ctx, lut, d_y, d_dirs, 0.0, 1e-3, False, corrected=True)[3]
        ctx.sync()
        yc = yc.cpu().numpy()
        mb0 = d_mb0.cpu().numpy()
        y_h = d_y.cpu().numpy().astype(np.float64, copy=False)
        yc = yc * np.reshape(mb0, (-1, 1))
        yc[:, b0] = y_h[:, b0] * np.reshape(mb0, (-1, 1))
        return sp.scatter(yc)

    def route_b():
        xi = _capi.freewater_fit_device(ctx, lut, d_y, d_dirs, 0.0, 1e-3, False, iso=True)[-1]
        plan.corrected_device(lut, d_y, xi, vol, d_mb0, b0)
        ctx.sync()
        return vol.cpu().numpy()

    def wall(fn):
        ts, out = [], None
        for _ in range(a.reps + 1):
            torch.cuda.synchronize()
            t = time.perf_counter()
            out = fn()
            ts.append((time.perf_counter() - t) * 1e3)
        return float(np.median(ts[1:])), min(ts[1:]), max(ts[1:]), out

    ta, va = wall(route_a)[::3]
    pa = ctx.last_path()
    tb, lo, hi, vb = wall(route_b)
    pb = ctx.last_path()
    rel = np.abs(va - vb).max() / np.abs(va).max()
    print(f'(a) corrected=True fit + host block + host-array scatter: median {ta:.1f} ms   [{pa}]')
    print(f'(b) fused fit with x_iso + volume kernel + one copy home:  median {tb:.1f} ms (min {lo:.1f}, max {hi:.1f})   [{pb}]')
    print(f'(a) / (b) = {ta / tb:.1f}; max |volume (a) - volume (b)| / max |volume| = {rel:.1e}')


if __name__ == '__main__':
    main()
