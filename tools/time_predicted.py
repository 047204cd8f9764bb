#!/usr/bin/env python3
"""The predicted signal (amx_prep_predicted_device), 300 000 masked of 360 000 voxels, one process per leg, median of 7:

  noddi-kernel      the volume kernel on NODDI (99 volumes, 145 atoms), from the coefficients a fit left
  freewater-kernel  the same on Free-Water (65 volumes, 11 atoms), beside k_fw_corrected on the same geometry (the streaming yardstick)
  noddi-fit         the NODDI fit with and without the coefficient hand-over (AMX_F_DEBUG_X: 3 x 145 doubles per voxel written)
  noddi-dense       the NODDI volume kernel on hand-made coefficients of 4 / 16 / 17 / 145 non-zeros per voxel: the compacted list up to
                    its capacity (16), and the dense walk that takes over beyond it
  sandi-kernel      the volume kernel on SANDI (6 volumes, 15 atoms, one dictionary), whose optimum is dense (~12 atoms: just under the cap)

Every line starts with the library's amx_build_id.

    python tools/time_predicted.py [--voxels 300000] [--reps 7] [--leg NAME]      (no --leg: every leg, each in a process of its own)
    python tools/time_predicted.py --counters DIR      rocprofv3 --pmc over the two kernel legs, one counter set per process (a run of
                                                       their own: HIP-event times of a profiled process are not rates), k_predict's rows printed
    python tools/time_predicted.py --bench PARENT      bench.py plain NODDI and --model freewater, the built checkout of the parent commit
                                                       under PARENT and this tree alternating (twice each), ms per step of every run
"""
import argparse
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
LEGS = ('noddi-kernel', 'freewater-kernel', 'noddi-fit', 'noddi-dense', 'sandi-kernel')
ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


def scene(model, n):
    """dictionary, plan, signals in HBM as Evaluation.fit() holds them after the gather"""
    import torch
    from amico_amd import _capi, prep, synthetic as S
    dirs = S.fibonacci_hemisphere(500)
    ht = S.build_htable(dirs)
    if model == 'noddi':
        sch = S.make_scheme(seed=0)
        K = S.noddi_kernels(sch, dirs)
        y, d = S.noddi_signals_parallel(n, K, ht, sch, seed=1)
    elif model == 'sandi':
        sch = S.directional_average_scheme(S.make_sandi_scheme())
        K, Rs, d_in, d_isos = S.sandi_kernels(sch)
        y, d = S.sandi_signals(n, K, sch, seed=1), None
    else:
        sch = S.make_scheme(5, ((1000.0, 60),), seed=3)
        K = S.freewater_kernels(sch, dirs)
        y, d = S.freewater_signals(n, K, ht, sch, seed=1)
    shape = (100, 60, -(-n * 6 // 5 // 6000))               # a sixth of the volume is background
    mask = np.zeros(int(np.prod(shape)), dtype=np.uint8)
    mask[np.random.default_rng(0).permutation(mask.size)[:n]] = 1
    mask = mask.reshape(shape)
    sp = prep.SignalPreparation(sch, np.zeros(shape + (sch.nS,), dtype=np.float32), mask, do_normalize=False)
    ctx = sp.ctx
    if model == 'sandi':
        lut = _capi.upload_sandi(ctx, K, Rs, d_in, d_isos)
    else:
        lut = _capi.upload_noddi(ctx, K, ht, sch.dwi_idx) if model == 'noddi' else _capi.upload_freewater(ctx, K, ht)
    d_y = torch.from_numpy(y.astype(np.float32)).cuda()
    d_dirs = None if d is None else torch.from_numpy(d).cuda()
    d_mb0 = torch.from_numpy(np.random.default_rng(1).uniform(300.0, 900.0, n).astype(np.float32)).cuda()
    vol = torch.empty(shape + (sch.nS,), dtype=torch.float32, device='cuda')
    return ctx, sp._plan, lut, sch, mask, d_y, d_dirs, d_mb0, vol


def leg(name, n, reps):
    import torch
    from amico_amd import _capi
    tag = _capi.build_id()
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

    model = name.split('-')[0]
    ctx, plan, lut, sch, mask, d_y, d_dirs, d_mb0, vol = scene(model, n)
    nS = sch.nS
    if name == 'noddi-fit':
        def fit(**k):
            out = _capi.noddi_fit_device(ctx, lut, d_y, d_dirs, 0.5, 1e-3, 3, **k)
            return out
        for label, kw in (('maps only', {}), ('with the coefficient hand-over', dict(return_x=True)), ('maps only', {}),
                          ('with the coefficient hand-over', dict(return_x=True))):
            t, lo, hi = events(lambda: fit(**kw))
            ctx.sync()
            print(f'{tag} | NODDI fit, {n} voxels x {nS}, {label}: median {t:.3f} ms (min {lo:.3f}, max {hi:.3f})')
        print(f'{tag} | (the hand-over includes zeroing its buffer, {n * 3 * lut.n_atoms * 8 / 1e6:.0f} MB; path: {ctx.last_path()})')
        return
    if name == 'noddi-dense':
        rng = np.random.default_rng(2)
        for k in (4, 16, 17, lut.n_atoms):
            xh = np.zeros((n, lut.n_atoms))
            cols = np.argsort(rng.random((n, lut.n_atoms)), axis=1)[:, :k]
            np.put_along_axis(xh, cols, rng.uniform(0.01, 1.0, (n, k)), axis=1)
            x = torch.from_numpy(xh).cuda()
            t, lo, hi = events(lambda: plan.predicted_device(lut, x, vol, d_dirs, d_mb0))
            ctx.sync()
            print(f'{tag} | k_predict noddi, {k} non-zeros in every voxel ({"compacted list" if k <= 16 else "dense walk"}): median {t:.3f} ms '
                  f'(min {lo:.3f}, max {hi:.3f}), {n * nS * k / t * 1e-6:.1f} G gathers/s')
        return
    if model == 'noddi':
        x = _capi.noddi_fit_device(ctx, lut, d_y, d_dirs, 0.5, 1e-3, 3, return_x=True)[-1]
    elif model == 'sandi':
        x = _capi.sandi_fit_device(ctx, lut, d_y.double(), 0.0, 5e-3, return_x=True)[-1]
    else:
        x = _capi.freewater_fit_device(ctx, lut, d_y, d_dirs, 0.0, 1e-3, False, return_x=True)[-1]
    ctx.sync()
    xh = x.cpu().numpy()
    nnz = (xh[:, 2, :] if xh.ndim == 3 else xh) != 0
    t, lo, hi = events(lambda: plan.predicted_device(lut, x, vol, d_dirs, d_mb0))
    ctx.sync()
    per = nnz.sum(axis=1)
    gb = (vol.numel() * 4 + n * (lut.n_atoms * 8 + 24 + 4)) / 1e9        # volume written; x, directions, mean_b0 read (tile gathers not counted)
    gathers = float(per.sum()) * nS
    print(f'{tag} | k_predict {model} (volume form, rescale) {n} masked of {mask.size} voxels x {nS}: median {t:.3f} ms (min {lo:.3f}, max {hi:.3f}), '
          f'{gb / t * 1e3:.0f} GB/s of volume + x traffic, {n / t * 1e-6:.2f} G voxels/s')
    print(f'{tag} | non-zeros per voxel: mean {per.mean():.1f}, max {per.max()}, over 16: {int((per > 16).sum())} voxels; '
          f'{gathers / 1e6:.0f} M tile gathers = {gathers / t * 1e-6:.1f} G gathers/s')
    if model == 'freewater':
        xi = _capi.freewater_fit_device(ctx, lut, d_y, d_dirs, 0.0, 1e-3, False, iso=True)[-1]
        ctx.sync()
        tc, lo, hi = events(lambda: plan.corrected_device(lut, d_y, xi, vol, d_mb0, sch.b0_idx))
        print(f'{tag} | k_fw_corrected (volume form, rescale + keep b0) on the same geometry: median {tc:.3f} ms (min {lo:.3f}, max {hi:.3f}); '
              f'k_predict / k_fw_corrected = {t / tc:.1f}')


COUNTER_SETS = ('SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VMEM SQ_INSTS_VMEM_RD SQ_INSTS_LDS',
                'TA_TA_BUSY_sum TA_BUSY_avr TD_TD_BUSY_sum TCP_PENDING_STALL_CYCLES_sum',
                'TCP_TCC_READ_REQ_sum TCP_TCC_WRITE_REQ_sum TCP_TOTAL_CACHE_ACCESSES_sum TCP_TCC_READ_REQ_LATENCY_sum',
                'TCC_HIT_sum TCC_MISS_sum TCC_REQ_sum TCC_EA0_RDREQ_sum',
                'TCC_EA0_RDREQ_DRAM_32B_sum TCC_EA0_WRREQ_WRITE_DRAM_32B_sum')


def counters(out, n):
    """one profiled process per (leg, counter set); then the mean of every counter over k_predict's dispatches"""
    import collections
    import csv
    import glob
    me = os.path.abspath(__file__)
    for name in ('noddi-kernel', 'freewater-kernel'):
        acc = collections.defaultdict(list)
        for i, cs in enumerate(COUNTER_SETS):
            d = os.path.join(out, '%s_%d' % (name, i))
            with open(os.devnull, 'w') as null:
                rc = subprocess.call(['rocprofv3', '--pmc'] + cs.split() + ['--output-format', 'csv', '-d', d, '--', sys.executable, me, '--voxels', str(n),
                                      '--reps', '3', '--leg', name], stdout=null, stderr=null, timeout=280)
            if rc != 0:                                      # whatever the status: nothing more is started on the GPU behind a failed child
                print('%s: counter set %d failed (status %d), stopping: %s' % (name, i, rc, cs))
                return rc
            for f in glob.glob(d + '/**/*counter_collection.csv', recursive=True):
                for r in csv.DictReader(open(f)):
                    if 'k_predict' in r['Kernel_Name']:
                        acc[r['Counter_Name']].append(float(r['Counter_Value']))
        print('k_predict, %s, %d voxels: mean per dispatch' % (name, n))
        for c in sorted(acc):
            print('    %-34s n=%-3d %.6g' % (c, len(acc[c]), sum(acc[c]) / len(acc[c])))
    return 0


def bench_ab(parent):
    """bench.py in the parent's built checkout and in this tree, alternating: the maps-only fits must not differ by more than the
    parent's own run-to-run spread"""
    import json
    base = [sys.executable, 'bench.py', '--gpus', '1', '--steps', '20', '--warmup', '3', '--no-cpu-baseline', '--no-other-configs']
    for k in (1, 2):
        for more in ((), ('--model', 'freewater')):
            for who, cwd in (('parent', os.path.abspath(parent)), ('this', ROOT)):
                with open(os.devnull, 'w') as null:
                    line = subprocess.check_output(base + list(more), cwd=cwd, stderr=null, timeout=280).decode().strip().splitlines()[-1]
                d = json.loads(line)
                flat = {key: v for key, v in d.items() if not isinstance(v, (dict, list)) and key in ('metric', 'value', 'unit', 'ms_per_step', 'vs_baseline')}
                print('%-9s %-6s run %d: %s' % (more[-1] if more else 'noddi', who, k, flat), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--voxels', type=int, default=300000)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--leg', choices=LEGS)
    ap.add_argument('--counters', metavar='DIR')
    ap.add_argument('--bench', metavar='PARENT')
    a = ap.parse_args()
    if a.leg:
        return leg(a.leg, a.voxels, a.reps)
    if a.counters:
        return counters(a.counters, a.voxels)
    if a.bench:
        return bench_ab(a.bench)
    for name in LEGS:                                       # a fresh child process per leg
        subprocess.check_call([sys.executable, os.path.abspath(__file__), '--voxels', str(a.voxels), '--reps', str(a.reps), '--leg', name],
                              timeout=280)                  # (a leg that hangs ends the run; a failed one does too: check_call)


if __name__ == '__main__':
    main()
