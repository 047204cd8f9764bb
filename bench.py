#!/usr/bin/env python3
"""bench.py -- NODDI fit throughput on MI355X (BASELINE.json metric: voxels/sec, whole node).

A "step" is one pass of the whole hot path (direction -> LUT index, bucketing, the three
solver stages, maps) over one batch of synthetic voxels that is already resident in HBM.
Workload at N=1 (BASELINE.json configs[1]): NODDI, 1 M masked voxels, 99-volume 2-shell
scheme (9 b0 + 30 @ b700 + 60 @ b2000), 145 atoms, 500 LUT orientations.  With --gpus N each
rank fits its own 1 M-voxel shard (weak scaling) and one RCCL all_gather of the maps ends
every step.

    python bench.py --gpus 1 --steps 5 --warmup 1
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W

A plain run sets up, warms up, times the K steps and prints the headline line (metric, value, unit,
ms_per_step, ...).  --full adds what needs runs or checks of its own: the stage groups' HIP events, the
roofline and counter figures, solver statistics, parity against the CPU oracle, the size scan, the
host-buffer legs, the other protocols and models and the CPU baselines.  --dump-outputs DIR writes the
maps of the last timed step as DIR/estimates.npy; the synthetic inputs are seeded, so two builds run
with the same arguments can be compared output for output.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BYTES_PER_VOXEL = 8 * 99 + 24 + 24          # y f64[99] + DIRs f64[3] + 3 maps f64 = 840 B
HBM_PEAK_GBS = 8000.0                       # MI355X_MICROARCH.md: 8.0 TB/s spec


def physical_cores():
    try:
        import psutil
        return int(psutil.cpu_count(logical=False) or 0) or None
    except Exception:
        return None


def median_rate(fn, n, runs=5):
    """voxels/s of fn(): one warm-up, then the median of `runs` timed runs"""
    fn()
    ts = []
    for _ in range(runs):
        t = time.perf_counter(); fn(); ts.append(time.perf_counter() - t)
    return n / float(np.median(ts)), float(np.median(ts))


_PMC = {}


def pmc_json():
    """profiles/pmc_traffic.json -- but only when it was measured on THIS build: the summary carries the source hash of the library
    it profiled (`csrc_hash`, written by tools/r05/summarise.py from amx_build_id); counters of other kernels are not reported as
    this run's.  Returns (dict or None, note)."""
    if 'v' not in _PMC:
        t, note = None, None
        try:
            with open(os.path.join(ROOT, 'profiles', 'pmc_traffic.json')) as f:
                t = json.load(f)
            from amico_amd import _capi
            have = _capi.build_id().split()[-1]
            if t.get('csrc_hash') != have:
                note = 'profiles/pmc_traffic.json was measured on build %s, this library is %s: counter figures withheld' % (t.get('csrc_hash'), have)
                t = None
        except (OSError, ValueError) as e:
            note = 'profiles/pmc_traffic.json unreadable: %s' % e
        _PMC['v'] = (t, note)
    return _PMC['v']


def build_record():
    from amico_amd import _capi
    return {'build_id': _capi.build_id(), 'source_id': _capi.source_id(), 'library_matches_sources': _capi.build_is_current(),
            'pmc_summary_note': pmc_json()[1]}


def pmc_small(model, key):
    """per-launch counter figure of the lane kernels from the committed profile summary (profiles/pmc_traffic.json)"""
    try:
        return pmc_json()[0]['small_models'][model][key]
    except (KeyError, TypeError):
        return None


def small_model(model, n, steps, warmup, cpu=True, host_legs=True):
    """FreeWater (config 3) / SANDI (config 4) on one GPU: same timing protocol as the headline, returns the record"""
    import torch
    from amico_amd import _capi, synthetic as S
    from oracle import oracle
    dev = torch.device('cuda', 0)
    ctx = _capi.Context(0)
    L = _capi.lib()
    lut_dirs = S.fibonacci_hemisphere(500)
    htable = S.build_htable(lut_dirs)
    cores = physical_cores() or os.cpu_count() or 1        # one thread per physical core: SMT siblings slow this code down
    if model == 'freewater':
        scheme = S.make_scheme(1, ((1000.0, 64),), seed=3)
        K = S.freewater_kernels(scheme, lut_dirs)
        y_h, d_h = S.freewater_signals(n, K, htable, scheme, seed=1)
        lut = _capi.upload_freewater(ctx, K, htable)
        y = torch.from_numpy(y_h).to(dev); d = torch.from_numpy(d_h).to(dev)
        est = torch.zeros((n, 2), dtype=torch.float64, device=dev)
        bpv = 8 * scheme.nS + 24 + 16

        def step():
            ctx.check(L.amx_freewater_fit_device(ctx._h, lut._h, y.data_ptr(), d.data_ptr(), n, 0.0, 1e-3, 0, 0,
                                                 est.data_ptr(), None, None, None, None))
        ref = lambda m: oracle.freewater_fit(y_h[:m], d_h[:m], K, htable, nthreads=cores)['estimates']
        name = 'FreeWater fit, %d voxels, 65-volume single shell (1 b0 + 64@b1000), 11 atoms, ndirs=500' % n
        kernel = 'FreeWater: projection c = A\'y on the fp64 matrix cores (producer wavefront) + block-pivoting active-set solver (consumer wavefronts)'
    elif model == 'czb':
        # CylinderZeppelinBall (SURVEY 8 row a-M; not a BASELINE config): dictionary generated + resampled by this repository
        # (amico_amd.synthesis -> lut.rotate_kernel -> amx_lut_resample) on a 3-shell STEJSKALTANNER scheme
        import amico_amd
        scheme = S.make_sandi_scheme(bvals=(1000., 2500., 4000.), ndir_per_shell=30, n_b0=3)
        ae = amico_amd.Evaluation()
        ae.set_data(np.ones((2, 2, 2, scheme.nS), dtype=np.float32), scheme, np.ones((2, 2, 2), dtype=np.uint8))
        ae.set_model('CylinderZeppelinBall')
        ae.load_kernels(ae.generate_kernels(lut_dirs), lut_dirs)
        K, Rs_ = ae.KERNELS, ae.model.Rs
        rng = np.random.default_rng(1)
        ori = rng.integers(0, len(lut_dirs), n)
        a1, a2 = rng.integers(0, K['wmr'].shape[0], n), rng.integers(0, K['wmh'].shape[0], n)
        f = rng.dirichlet([2, 2, 1], n)
        y_h = (f[:, :1] * K['wmr'][a1, ori] + f[:, 1:2] * K['wmh'][a2, ori] + f[:, 2:] * K['iso'][0][None, :]).astype(np.float64)
        y_h = np.sqrt((y_h + rng.normal(0, 1 / 30, y_h.shape)) ** 2 + rng.normal(0, 1 / 30, y_h.shape) ** 2)
        d_h = np.ascontiguousarray(lut_dirs[ori])
        lut = _capi.upload_czb(ctx, K, Rs_, htable)
        y = torch.from_numpy(y_h).to(dev); d = torch.from_numpy(d_h).to(dev)
        est = torch.zeros((n, 3), dtype=torch.float64, device=dev)
        bpv = 8 * scheme.nS + 24 + 24

        def step():
            ctx.check(L.amx_czb_fit_device(ctx._h, lut._h, y.data_ptr(), d.data_ptr(), n, 0.0, 4.0, 0, est.data_ptr(), None, None, None))
        ref = lambda m: oracle.czb_fit(y_h[:m], d_h[:m], K, Rs_, htable, nthreads=cores)['estimates']
        name = 'CylinderZeppelinBall fit, %d voxels, %d volumes (3 shells), 26 atoms, ndirs=500' % (n, scheme.nS)
        kernel = 'CylinderZeppelinBall: projection z0 = M(A\'y - lambda1), c on the fp64 matrix cores, then block principal pivoting, one voxel per lane'
    else:
        full = S.make_sandi_scheme()
        avg = S.directional_average_scheme(full)
        K, Rs, d_in, d_isos = S.sandi_kernels(avg)
        y_h = S.sandi_signals(n, K, avg, seed=1)
        lut = _capi.upload_sandi(ctx, K, Rs, d_in, d_isos)
        y = torch.from_numpy(y_h).to(dev)
        est = torch.zeros((n, 6), dtype=torch.float64, device=dev)
        bpv = 8 * avg.nS + 48

        def step():
            ctx.check(L.amx_sandi_fit_device(ctx._h, lut._h, y.data_ptr(), n, 0.0, 5e-3, 0, est.data_ptr(), None, None, None))
        ref = lambda m: oracle.sandi_fit(y_h[:m], K, Rs, d_in, d_isos, nthreads=cores)['estimates']
        name = 'SANDI fit, %d voxels, 5 shells direction-averaged (6 values per voxel), 15 atoms' % n
        kernel = 'SANDI: row-space Woodbury solve, one voxel per lane'
    ctx.set_profiling(True, only=1)
    for _ in range(warmup):
        step(); ctx.sync()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    kms = 0.0
    for _ in range(steps):
        step(); ctx.sync()
        kms += ctx.last_kernel_ms(1)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    kms /= steps
    # the kernels that ran, as the library names them (amx_last_path) -- not a literal in this file (the FreeWater
    # label still named the kernel pair after the fused kernel had replaced it)
    launched = ctx.last_path()
    kernel = '%s  [%s]' % (launched, kernel)
    m = min(n, 20000)
    got = est[:m].cpu().numpy()
    want = ref(m)
    diff = np.abs(got - want)
    rel = diff / (np.abs(want) + 1e-3)
    ach = bpv * n / (kms * 1e-3) / 1e9
    out = {'metric': 'voxels/sec, %s fit' % model, 'value': n * steps / el, 'unit': 'voxels/s', 'n_gpus': 1, 'steps': steps,
           'warmup': warmup, 'ms_per_step': 1e3 * el / steps, 'dtype': 'f64', 'data': 'synthetic', 'config': {'workload': name},
           'roofline': {'bound': 'hbm', 'achieved': ach, 'peak': HBM_PEAK_GBS, 'unit': 'GB/s', 'frac': ach / HBM_PEAK_GBS,
                        'traffic': pmc_small(model, 'bytes_per_voxel_measured') and pmc_small(model, 'bytes_per_voxel_measured') * n,
                        'kernel': kernel, 'kernel_ms': kms, 'bytes_per_voxel': bpv},
           'parity': {'sample_voxels': m, 'max_abs_dmap': float(diff.max()), 'max_rel_dmap': float(rel.max())},
           'solver_stats': ctx.last_stats()}
    if model == 'freewater':
        # the same fit on float32 signals in HBM (amx_freewater_fit_device_f32: the image's own dtype, 260 B rows): reported beside
        # the float64 figure, never as `value` (BASELINE's boundary dtype is float64)
        y32 = y.to(torch.float32)
        est32 = torch.zeros_like(est)

        def step32():
            ctx.check(L.amx_freewater_fit_device_f32(ctx._h, lut._h, y32.data_ptr(), d.data_ptr(), n, 0.0, 1e-3, 0, 0,
                                                     est32.data_ptr(), None, None, None, None))
        for _ in range(warmup):
            step32(); ctx.sync()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        k32 = 0.0
        for _ in range(steps):
            step32(); ctx.sync()
            k32 += ctx.last_kernel_ms(1)
        torch.cuda.synchronize()
        el32 = time.perf_counter() - t1
        bpv32 = 4 * scheme.nS + 24 + 16
        out['float32_signals_in_hbm'] = {'value': n * steps / el32, 'unit': 'voxels/s', 'ms_per_step': 1e3 * el32 / steps, 'kernel_ms': k32 / steps,
                                         'bytes_per_voxel': bpv32, 'achieved_GBps': bpv32 * n / (k32 / steps * 1e-3) / 1e9,
                                         'frac_of_hbm_peak': bpv32 * n / (k32 / steps * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                         'max_abs_dmap_vs_f64_signals': float((est32 - est).abs().max())}
        del y32, est32
    if model in ('freewater', 'sandi') and host_legs:
        # host numpy in -> host numpy out (pageable memory; PCIe inclusive): the batches of the pipelined entry points hide the
        # solver behind the copies here, so this is a PCIe figure, reported beside the kernels' rate, never as `value`
        hb = {}
        for tag, yy in (('f64', y_h), ('f32', y_h.astype(np.float32))):
            call = (lambda: _capi.freewater_fit(ctx, lut, yy, d_h, 0.0, 1e-3, False)) if model == 'freewater' else \
                   (lambda: _capi.sandi_fit(ctx, lut, yy, 0.0, 5e-3))
            call()
            ts = []
            for _ in range(3):
                t1 = time.perf_counter(); call(); ts.append(time.perf_counter() - t1)
            hb[tag] = {'value': n / float(np.median(ts)), 'unit': 'voxels/s', 'ms_per_call': 1e3 * float(np.median(ts)),
                       'GB_per_s_uploaded': yy.nbytes / float(np.median(ts)) / 1e9}
        out['host_buffers'] = hb
    if cpu:
        oracle.use_fast_build(True)
        mc = n
        rate, dt = median_rate(lambda: ref(mc), mc, runs=5)
        oracle.use_fast_build(False)
        out['cpu_baseline'] = {'value': rate, 'unit': 'voxels/s', 'cores': cores, 'logical_cpus': os.cpu_count(), 'kind': 'port',
                               'sample': 'all %d voxels, oracle/amico_oracle.c -O3 -march=native, %d threads (one per physical core), warm-up + median of 5 runs (%.2f s)' % (mc, cores, dt)}
    del y, est
    torch.cuda.empty_cache()
    return out


def other_models(args):
    # (--no-cpu-baseline here also skips the host-buffer legs: profiling runs want the device-resident launches only)
    print(json.dumps(small_model(args.model, args.voxels, args.steps, args.warmup, cpu=not args.no_cpu_baseline, host_legs=not args.no_cpu_baseline)))


def dti_directions(args):
    """Principal-direction step before the fit (SURVEY section 8 f row 1): y f64[n, 99] -> dirs f64[n, 3], HBM-bound."""
    import torch
    from amico_amd import dti, synthetic as S
    from oracle import signal_np
    dev = torch.device('cuda', 0)
    n = args.voxels
    lut_dirs = S.fibonacci_hemisphere(500)
    scheme = S.make_scheme()
    K = S.noddi_kernels(scheme, lut_dirs)
    y_h, _ = S.noddi_signals(n, K, S.build_htable(lut_dirs), scheme, seed=1)
    est = dti.TensorDirections.from_scheme(scheme)
    ctx = est.ctx
    y = torch.from_numpy(y_h).to(dev)
    d = torch.zeros((n, 3), dtype=torch.float64, device=dev)
    ctx.set_profiling(True, only=4)
    for _ in range(args.warmup):
        est.fit_device(y.data_ptr(), n, d.data_ptr()); ctx.sync()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    kms = 0.0
    for _ in range(args.steps):
        est.fit_device(y.data_ptr(), n, d.data_ptr()); ctx.sync()
        kms += ctx.last_kernel_ms(4)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    kms /= args.steps
    m = min(n, 200000)
    t1 = time.perf_counter()
    ref, ev = signal_np.dti_directions(y_h[:m], scheme.b, scheme.raw[:, :3], return_evals=True)
    cpu = m / (time.perf_counter() - t1)
    ok = (ev[:, 0] - ev[:, 1]) > 1e-6 * np.abs(ev[:, 0])
    g = d[:m].cpu().numpy()
    err = np.linalg.norm(np.cross(g[ok], ref[ok]), axis=1)
    bpv = 8 * scheme.nS + 24
    # the same on float32 signals (what amx_prep_gather_device_f32 leaves in HBM; Evaluation.fit runs this variant)
    y32 = y.to(torch.float32)
    d32 = torch.zeros_like(d)
    for _ in range(args.warmup):
        est.fit_device(y32.data_ptr(), n, d32.data_ptr(), f32=True); ctx.sync()
    k32 = 0.0
    for _ in range(args.steps):
        est.fit_device(y32.data_ptr(), n, d32.data_ptr(), f32=True); ctx.sync()
        k32 += ctx.last_kernel_ms(4)
    k32 /= args.steps
    y32w = y32.to(torch.float64)
    est.fit_device(y32w.data_ptr(), n, d.data_ptr()); ctx.sync()
    f32 = {'kernel_ms': k32, 'bytes_per_voxel': 4 * scheme.nS + 24, 'achieved_GBs': (4 * scheme.nS + 24) * n / (k32 * 1e-3) / 1e9,
           'bit_identical_to_f64_input': bool(torch.equal(d, d32))}
    print(json.dumps({'metric': 'voxels/sec, principal directions (log-linear tensor fit)', 'value': n * args.steps / el,
                      'unit': 'voxels/s', 'n_gpus': 1, 'steps': args.steps, 'warmup': args.warmup,
                      'ms_per_step': 1e3 * el / args.steps, 'dtype': 'f64', 'data': 'synthetic',
                      'config': {'workload': 'DTI OLS directions, %d voxels, 99-volume 2-shell scheme' % n},
                      'roofline': {'bound': 'hbm', 'achieved': bpv * n / (kms * 1e-3) / 1e9, 'peak': HBM_PEAK_GBS,
                                   'unit': 'GB/s', 'frac': bpv * n / (kms * 1e-3) / 1e9 / HBM_PEAK_GBS, 'traffic': None,
                                   'kernel': 'k_dti_dirs', 'kernel_ms': kms, 'bytes_per_voxel': bpv},
                      'float32_signals_in_hbm': f32,
                      'parity': {'sample_voxels': int(ok.sum()), 'max_sin_angle': float(err.max())},
                      'cpu_baseline': {'value': cpu, 'unit': 'voxels/s', 'cores': 1, 'kind': 'port',
                                       'sample': '%d voxels, numpy restatement of dipy OLS (pinv + log + batched eigh)' % m}}))


def signal_preparation(args):
    """Mask gather + b0 normalisation + clip + float64 (SURVEY section 8 f rows 2-3): image f32 -> y f64, HBM-bound."""
    import torch
    from amico_amd import prep, synthetic as S
    from oracle import signal_np
    dev = torch.device('cuda', 0)
    scheme = S.make_scheme()
    shape = tuple(int(v) for v in os.environ.get('PREP_SHAPE', '128,128,80').split(','))      # (PREP_SHAPE=192,192,120: ~1.9 M masked voxels)
    rng = np.random.default_rng(1)
    out = {}
    for order in os.environ.get('PREP_ORDERS', 'F,C').split(','):
        img = rng.uniform(0.0, 900.0, shape + (scheme.nS,)).astype(np.float32)
        img[..., scheme.b0_idx] += 600.0
        img = np.asarray(img, order=order)
        xx, yy, zz = np.meshgrid(*[np.linspace(-1, 1, s) for s in shape], indexing='ij')
        mask = ((xx * xx + yy * yy + zz * zz) < 0.92).astype(np.uint8)           # brain-sized blob: ~50 % of the box
        sp = prep.SignalPreparation(scheme, img, mask)
        ctx = sp.ctx
        n = sp.n_vox
        flat = np.lib.stride_tricks.as_strided(img, shape=(img.size,), strides=(4,))
        d_img = torch.from_numpy(flat.copy()).to(dev)
        d_y = torch.zeros((n, scheme.nS), dtype=torch.float64, device=dev)
        d_m = torch.zeros(n, dtype=torch.float32, device=dev)
        L = _capi_lib()
        ctx.set_profiling(True, only=4)

        def step():
            ctx.check(L.amx_prep_gather_device(ctx._h, sp._plan._h, d_img.data_ptr(), 1, 0.0, d_y.data_ptr(),
                                               d_m.data_ptr(), None))
        for _ in range(args.warmup):
            step(); ctx.sync()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        kms = 0.0
        for _ in range(args.steps):
            step(); ctx.sync()
            kms += ctx.last_kernel_ms(4)
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        kms /= args.steps
        t1 = time.perf_counter()
        ref, _ = signal_np.prepare_signal(img, mask, scheme.b0_idx, scheme.dwi_idx)
        cpu = n / (time.perf_counter() - t1)
        exact = bool(np.array_equal(d_y.cpu().numpy(), ref))
        bpv = 4 * scheme.nS + 8 * scheme.nS + 4
        # float32 rows out (amx_prep_gather_device_f32: what Evaluation.fit and the volume pipeline use)
        d_y32 = torch.zeros((n, scheme.nS), dtype=torch.float32, device=dev)
        k32 = 0.0
        for it in range(args.warmup + args.steps):
            ctx.check(L.amx_prep_gather_device_f32(ctx._h, sp._plan._h, d_img.data_ptr(), 1, 0.0, d_y32.data_ptr(), d_m.data_ptr(), None))
            ctx.sync()
            if it >= args.warmup:
                k32 += ctx.last_kernel_ms(4)
        k32 /= args.steps
        bpv32 = 4 * scheme.nS + 4 * scheme.nS + 4
        out[order] = {'voxels': n, 'voxels_per_s': n * args.steps / el, 'kernel_ms': kms,
                      'achieved_GBs': bpv * n / (kms * 1e-3) / 1e9, 'bit_exact_vs_numpy': exact, 'numpy_voxels_per_s': cpu,
                      'float32_rows': {'kernel_ms': k32, 'bytes_per_voxel': bpv32, 'achieved_GBs': bpv32 * n / (k32 * 1e-3) / 1e9,
                                       'bit_exact_vs_numpy': bool(np.array_equal(d_y32.cpu().numpy().astype(np.float64), ref))}}
        del d_y32
    if os.environ.get('PREP_DIRAVG', '1') != '0':
        # SANDI preprocessing: 306 volumes (6 b0 + 5 shells x 60) -> b0 mean + 5 shell means per masked voxel (core.py:229-252)
        full = S.make_sandi_scheme()
        shp = tuple(int(v) for v in os.environ.get('PREP_DIRAVG_SHAPE', '128,128,40').split(','))
        img = np.asfortranarray(rng.uniform(0.0, 900.0, shp + (full.nS,)).astype(np.float32))
        xx, yy, zz = np.meshgrid(*[np.linspace(-1, 1, s) for s in shp], indexing='ij')
        mask = ((xx * xx + yy * yy + zz * zz) < 0.92).astype(np.uint8)
        sp = prep.SignalPreparation(full, img, mask, do_directional_average=True)
        ctx = sp.ctx
        n = sp.n_vox
        flat = np.lib.stride_tricks.as_strided(img, shape=(img.size,), strides=(4,))
        d_img = torch.from_numpy(flat.copy()).to(dev)
        d_y = torch.zeros((n, 6), dtype=torch.float64, device=dev)
        d_m = torch.zeros(n, dtype=torch.float32, device=dev)
        L = _capi_lib()
        ctx.set_profiling(True, only=4)
        kms = 0.0
        for it in range(args.warmup + args.steps):
            ctx.check(L.amx_prep_gather_device(ctx._h, sp._plan._h, d_img.data_ptr(), 1, 0.0, d_y.data_ptr(), d_m.data_ptr(), None))
            ctx.sync()
            if it >= args.warmup:
                kms += ctx.last_kernel_ms(4)
        kms /= args.steps
        ref, _ = signal_np.prepare_signal(img, mask, full.b0_idx, full.dwi_idx, shells=full.shells, do_directional_average=True)
        bpv = 4 * full.nS + 8 * 6 + 4
        out['diravg_F'] = {'voxels': n, 'kernel_ms': kms, 'achieved_GBs': bpv * n / (kms * 1e-3) / 1e9, 'bytes_per_voxel': bpv,
                           'bit_exact_vs_numpy': bool(np.array_equal(d_y.cpu().numpy(), ref))}
    best = out.get('F') or out['C']
    print(json.dumps({'metric': 'voxels/sec, signal preparation (mask gather + b0 normalisation + clip)',
                      'value': best['voxels_per_s'], 'unit': 'voxels/s', 'n_gpus': 1, 'steps': args.steps,
                      'warmup': args.warmup, 'dtype': 'f32->f64', 'data': 'synthetic',
                      'config': {'workload': '%s float32 image, %d masked voxels, Fortran order (nibabel) '
                                             '[C order alongside]' % ('x'.join(str(v) for v in shape + (scheme.nS,)), best['voxels'])},
                      'roofline': {'bound': 'hbm', 'achieved': best['achieved_GBs'], 'peak': HBM_PEAK_GBS, 'unit': 'GB/s',
                                   'frac': best['achieved_GBs'] / HBM_PEAK_GBS, 'traffic': None, 'kernel': 'k_prep_gather',
                                   'kernel_ms': best['kernel_ms'], 'bytes_per_voxel': 12 * scheme.nS + 4},
                      'layouts': out,
                      'cpu_baseline': {'value': best['numpy_voxels_per_s'], 'unit': 'voxels/s', 'cores': 1,
                                       'kind': 'reference', 'sample': 'the numpy statements of core.py:209-223, 451-452 on the same image'}}))


def lut_resampling(args):
    """load_kernels' resampling (SURVEY section 8 f row 4): 144 atoms x 500 orientations, lmax 12, 2 shells -> 90 DWI volumes"""
    from amico_amd import lut, synthetic as S
    from amico_amd.models import get_context
    from oracle import lut_np
    scheme = S.make_scheme()
    rng = np.random.default_rng(0)
    n_atoms, ndirs = 144, 500
    idx_out, ylm_out = lut.aux_structures_resample(scheme, 12)
    lm = rng.normal(size=(n_atoms, ndirs, ylm_out.shape[1])).astype(np.float32)
    ctx = get_context()
    ctx.set_profiling(True, only=4)
    for _ in range(args.warmup):
        lut.resample_kernels(lm, scheme.nS, idx_out, ylm_out)
    t0 = time.perf_counter()
    kms = 0.0
    for _ in range(args.steps):
        out = lut.resample_kernels(lm, scheme.nS, idx_out, ylm_out)
        kms += ctx.last_kernel_ms(4)
    el = (time.perf_counter() - t0) / args.steps
    kms /= args.steps
    t1 = time.perf_counter()
    na = 8
    ref = np.stack([lut_np.resample_kernel(lm[a], scheme.nS, idx_out, ylm_out, False, ndirs) for a in range(na)])
    cpu = (time.perf_counter() - t1) / na * n_atoms
    # the same LUT from the un-rotated factors (rotate_kernel fused into the GEMM): 105 KB + 182 KB in instead of 52 MB
    from amico_amd import _capi
    nsh = lut.n_sh(12)
    zonal = rng.normal(size=(n_atoms, ylm_out.shape[1])).astype(np.float32)
    yrot = rng.normal(size=(ndirs, nsh)).astype(np.float32)
    _capi.lut_rotate_resample(ctx, zonal, yrot, ylm_out, idx_out, scheme.nS)
    t2 = time.perf_counter()
    fk = 0.0
    for _ in range(args.steps):
        fused = _capi.lut_rotate_resample(ctx, zonal, yrot, ylm_out, idx_out, scheme.nS)
        fk += ctx.last_kernel_ms(4)
    fused_s = (time.perf_counter() - t2) / args.steps
    lm_f = (zonal[:4, None, :] * np.tile(yrot, (1, ylm_out.shape[1] // nsh))[None, :, :]).astype(np.float32)
    fused_err = float(np.abs(fused[:4] - lut.resample_kernels(lm_f, scheme.nS, idx_out, ylm_out)).max())
    flop = 2.0 * n_atoms * ndirs * ylm_out.shape[1] * ylm_out.shape[0]
    print(json.dumps({'metric': 'seconds, LUT resampling of one subject (host arrays in/out)', 'value': el, 'unit': 's',
                      'higher_is_better': False, 'n_gpus': 1, 'steps': args.steps, 'warmup': args.warmup, 'dtype': 'f32',
                      'data': 'synthetic', 'config': {'workload': '144 atoms x 500 orientations, 182 SH coefficients -> 90 DWI volumes of 99'},
                      'roofline': {'bound': 'mfma', 'achieved': flop / (kms * 1e-3) / 1e12, 'peak': 157.3, 'unit': 'TFLOP/s',
                                   'frac': flop / (kms * 1e-3) / 1e12 / 157.3, 'traffic': None, 'kernel': 'k_lut_resample',
                                   'kernel_ms': kms, 'note': 'one-off per subject; the call is bound by the PCIe copies of lm (52 MB) and KERNELS (28 MB)'},
                      'parity': {'atoms_checked': na, 'max_abs_diff': float(np.abs(out[:na] - ref).max())},
                      'fused_rotate_resample': {'value': fused_s, 'unit': 's', 'kernel_ms': fk / args.steps, 'max_abs_diff_vs_two_step': fused_err,
                                                'note': 'amx_lut_rotate_resample: rotated SH coefficients formed in registers, no 52 MB upload'},
                      'cpu_baseline': {'value': cpu, 'unit': 's', 'cores': 1, 'kind': 'reference',
                                       'sample': 'the numpy statement of lut.pyx:274-311 on %d of 144 atoms, scaled' % na}}))


def volume_pipeline(args):
    """raw image in HBM -> NDI/ODI/FWF volumes in HBM: prepare + tensor directions + NODDI fit + scatter on one stream"""
    import torch
    from amico_amd import pipeline, synthetic as S
    from oracle import oracle, signal_np
    dev = torch.device('cuda', 0)
    scheme = S.make_scheme()
    lut_dirs = S.fibonacci_hemisphere(500)
    ht = S.build_htable(lut_dirs)
    K = S.noddi_kernels(scheme, lut_dirs)
    shape = (128, 128, 80)
    n_all = int(np.prod(shape))
    y, _ = S.noddi_signals(n_all, K, ht, scheme, seed=1)
    img = np.asfortranarray((y.reshape(shape + (-1,)) * 900.0).astype(np.float32))     # nibabel hands out Fortran order
    xx, yy, zz = np.meshgrid(*[np.linspace(-1, 1, s) for s in shape], indexing='ij')
    mask = ((xx * xx + yy * yy + zz * zz) < 0.92).astype(np.uint8)
    fused = os.environ.get('AMX_PIPELINE_UNFUSED', '0') in ('', '0')        # A/B: gather + tensor fit as two passes (the round-4 chain)
    pl = pipeline.NoddiVolumePipeline(scheme, img, mask, K, ht, fused=fused)
    flat = np.lib.stride_tricks.as_strided(img, shape=(img.size,), strides=(4,))
    d_img = torch.from_numpy(flat.copy()).to(dev)
    for _ in range(args.warmup):
        pl.run(d_img)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    t0 = time.perf_counter()
    for _ in range(args.steps):
        pl.run(d_img)
    torch.cuda.synchronize()
    el = (time.perf_counter() - t0) / args.steps
    n = pl.n_vox
    # parity of the whole chain on a sample: numpy preprocessing -> numpy/LAPACK tensor fit -> C oracle
    sel = mask == 1
    y_ref, _ = signal_np.prepare_signal(img, mask, scheme.b0_idx, scheme.dwi_idx)
    exact_y = bool(np.array_equal(pl.y.cpu().numpy(), y_ref))
    m = 20000
    d_ref = signal_np.dti_directions(y_ref[:m], scheme.b, scheme.raw[:, :3])
    ref = oracle.noddi_fit(y_ref[:m], d_ref, K, ht, scheme.dwi_idx, nthreads=os.cpu_count())['estimates']
    diff = np.abs(pl.est[:m].cpu().numpy() - ref).max(axis=1)
    print(json.dumps({'metric': 'voxels/sec, raw image -> map volumes (prepare + tensor directions + NODDI fit + scatter)',
                      'value': n / el, 'unit': 'voxels/s', 'n_gpus': 1, 'steps': args.steps, 'warmup': args.warmup,
                      'ms_per_step': 1e3 * el, 'dtype': 'f32 -> f64 -> f32', 'data': 'synthetic',
                      'config': {'workload': '128x128x80x99 float32 image (Fortran order), %d masked voxels, NODDI' % n,
                                 'gather_and_tensor_fit': 'one kernel' if fused else 'two passes'},
                      'parity': {'y_bit_exact': exact_y, 'sample_voxels': m, 'frac_within_1e-6': float((diff < 1e-6).mean()),
                                 'median_abs_dmap': float(np.median(diff)),
                                 'note': 'directions differ from LAPACK\'s by ~1e-13: a voxel whose LUT index flips gets another dictionary orientation'}}))


def _capi_lib():
    from amico_amd import _capi
    return _capi.lib()


def pmc_valu(stage, n, kernel_ms):
    """compute-side reading of the stage kernel: VALU wave-instructions per voxel (committed rocprofv3 PMC pass) and the
    share of the SIMDs' issue cycles they fill at the live kernel time (1024 SIMDs, 2.4 GHz, 4 cycles per wave64 VALU op)"""
    t = pmc_json()[0]
    try:
        insts = float(t['stage_valu_insts_per_launch'][str(stage)]) / t['voxels_per_launch']
    except (KeyError, ValueError, TypeError):
        return None
    busy = insts * n * 4.0 / 1024.0 / (kernel_ms * 1e-3 * 2.4e9)
    out = {'bound': 'dependent latency (VALU issue slots mostly idle)', 'valu_wave_insts_per_voxel': insts, 'issue_cycles_filled': busy,
           'source': 'profiles/pmc_traffic.json (SQ_INSTS_VALU) x live kernel time'}
    # the same kernel against the fp64 matrix cores: its dual scans are 120 v_mfma_f64_16x16x4 per trip of 64 voxels
    # (SQ_INSTS_VALU_MFMA_MOPS_F64 counts 512 flops each; MI355X: 78.6 TFLOP/s fp64 matrix peak)
    if stage == 8:
        try:
            mops = [v['mfma_f64_mops'] for k, v in t['kernels'].items() if k.startswith('k_nnls_seed<1')][0] / t['voxels_per_launch']
            tf = mops * n * 512.0 / (kernel_ms * 1e-3) / 1e12
            out['mfma_f64'] = {'flops_per_voxel': mops * 512.0, 'achieved': tf, 'peak': 78.6, 'unit': 'TFLOP/s', 'frac': tf / 78.6}
        except (KeyError, IndexError, TypeError):
            pass
    return out


def pmc_traffic(stage, n):
    """HBM bytes per launch of the stage kernel from the committed rocprofv3 PMC passes (profiles/), scaled to
    this run's voxels per launch; None when the profile summary is not there."""
    t = pmc_json()[0]
    try:
        return float(t['stage_bytes_per_launch'][str(stage)]) * n / t['voxels_per_launch']
    except (KeyError, ValueError, TypeError):
        return None


def pmc_whole_fit(n):
    """HBM bytes of ONE whole NODDI fit (all kernel groups of the committed PMC passes), scaled to n voxels"""
    t = pmc_json()[0]
    try:
        b = t['stage_bytes_per_launch']
        return sum(float(b[k]) for k in ('1', '2', '3', '5', '6', '7')) * n / t['voxels_per_launch']
    except (KeyError, ValueError, TypeError):
        return None


def noddi_hard_mix(ctx, lut, K, htable, scheme, n, steps, warmup):
    """the NODDI fit on signals the dictionary does not explain (synthetic.noddi_hard_signals: crossings, wrong direction,
    CSF-dominated, pure noise, flat, half-zeroed, background; SNR 5 / 15 / 40): rate, certification rates of the three stages, parity
    on a sample -- the headline's rates are a property of its signal distribution (one atom + iso <= 0.5, SNR 30), this leg says
    what the same chain does when the seed solvers are wrong more often"""
    import torch
    from amico_amd import _capi, synthetic as S
    from oracle import oracle
    dev = torch.device('cuda', torch.cuda.current_device())
    blk = 250_000
    parts = [S.noddi_hard_signals(min(blk, n - s), K, htable, scheme, seed=900 + s // blk) for s in range(0, n, blk)]
    y_h = np.concatenate([p[0] for p in parts]); d_h = np.concatenate([p[1] for p in parts])
    y = torch.from_numpy(y_h).to(dev); d = torch.from_numpy(d_h).to(dev)
    est = torch.zeros((n, 3), dtype=torch.float64, device=dev)
    L = _capi.lib()
    stream = torch.cuda.current_stream().cuda_stream

    def fit():
        ctx.check(L.amx_noddi_fit_device(ctx._h, lut._h, y.data_ptr(), d.data_ptr(), n, 0.5, 1e-3, 0, est.data_ptr(), None, None, None, stream))
    for _ in range(warmup):
        fit(); ctx.sync(stream)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fit(); ctx.sync(stream)
    torch.cuda.synchronize()
    el = (time.perf_counter() - t0) / steps
    ctx.set_profiling(True)                                    # (one more, untimed, fit with the stage groups' events recorded)
    fit(); ctx.sync(stream)
    ctx.set_profiling(False)
    stats, seed = ctx.last_stats(), ctx.last_seed_stats()
    kms = {}
    for w, name in ((0, 'all_kernels'), (5, 'stage1_gemm_seed_cert'), (6, 'lasso_gemm_seed_cert'), (7, 'stage3_seed_cert'), (1, 'stage1_leftover'), (2, 'lasso_leftover'), (3, 'stage3_leftover')):
        try:
            kms[name] = ctx.last_kernel_ms(w)
        except Exception:
            pass
    pick = np.unique(np.linspace(0, n - 1, min(n, 20000)).astype(np.int64))
    ref = oracle.noddi_fit(np.ascontiguousarray(y_h[pick]), np.ascontiguousarray(d_h[pick]), K, htable, scheme.dwi_idx, nthreads=physical_cores() or os.cpu_count() or 1)
    diff = np.abs(est.cpu().numpy()[pick] - ref['estimates']).max(axis=1)
    out = {'metric': 'voxels/sec, NODDI fit, hard signal mix (inputs resident in HBM)', 'value': n / el, 'unit': 'voxels/s', 'voxels': n,
           'ms_per_step': 1e3 * el, 'kernel_ms': kms, 'solver_stats': stats, 'seed_chain': seed,
           'parity': {'sample_voxels': len(pick), 'max_abs_dmap': float(diff.max()), 'frac_within_1e-6': float((diff < 1e-6).mean())},
           'mix': list(S.HARD_KINDS)}
    del y, d, est
    return out


def noddi_other_protocol(ctx, shells, n_b0, n, steps, warmup, headline_rate_per_byte, exvivo=False, snr=None):
    """the NODDI fit on another acquisition protocol (the reference's loop is shape generic, models.pyx:825-828, 851-861): voxels/s,
    the share of the headline's rate per byte of signal, certification rates, parity on a sample"""
    import torch
    from amico_amd import _capi, synthetic as S
    from oracle import oracle
    dev = torch.device('cuda', torch.cuda.current_device())
    lut_dirs = S.fibonacci_hemisphere(500)
    htable = S.build_htable(lut_dirs)
    scheme = S.make_scheme(n_b0, shells, seed=4)
    K = S.noddi_kernels(scheme, lut_dirs)
    y_h, d_h = S.noddi_signals_parallel(n, K, htable, scheme, seed=17, **({} if snr is None else {'snr': snr}))
    lut = _capi.upload_noddi(ctx, K, htable, scheme.dwi_idx, exvivo)
    y = torch.from_numpy(y_h).to(dev); d = torch.from_numpy(d_h).to(dev)
    est = torch.zeros((n, 4 if exvivo else 3), dtype=torch.float64, device=dev)
    L = _capi.lib()
    stream = torch.cuda.current_stream().cuda_stream

    def fit():
        ctx.check(L.amx_noddi_fit_device(ctx._h, lut._h, y.data_ptr(), d.data_ptr(), n, 0.5, 1e-3, 0, est.data_ptr(), None, None, None, stream))
    for _ in range(warmup):
        fit(); ctx.sync(stream)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fit(); ctx.sync(stream)
    torch.cuda.synchronize()
    el = (time.perf_counter() - t0) / steps
    fit(); ctx.sync(stream)
    stats, seed = ctx.last_stats(), ctx.last_seed_stats()
    pick = np.unique(np.linspace(0, n - 1, min(n, 10000)).astype(np.int64))
    ref = oracle.noddi_fit(np.ascontiguousarray(y_h[pick]), np.ascontiguousarray(d_h[pick]), K, htable, scheme.dwi_idx, is_exvivo=exvivo,
                           nthreads=physical_cores() or os.cpu_count() or 1)
    diff = np.abs(est.cpu().numpy()[pick] - ref['estimates']).max(axis=1)
    bpv = 8 * scheme.nS + 48
    out = {'metric': 'voxels/sec, NODDI fit, %d-volume protocol%s%s (inputs resident in HBM)' % (scheme.nS, ', ex-vivo model (dot compartment, 4 maps)' if exvivo else '', '' if snr is None else ', SNR %g' % snr), 'value': n / el, 'unit': 'voxels/s', 'voxels': n,
           'ms_per_step': 1e3 * el, 'volumes': int(scheme.nS), 'bytes_per_voxel': bpv,
           'rate_per_byte_vs_headline': (n / el * bpv) / headline_rate_per_byte,
           'solver_stats': stats, 'seed_chain': seed,
           'parity': {'sample_voxels': len(pick), 'max_abs_dmap': float(diff.max()), 'frac_within_1e-6': float((diff < 1e-6).mean())}}
    del y, d, est, lut
    torch.cuda.empty_cache()
    return out


def noddi_model_fit(K, htable, scheme, y_h, d_h, est_ref):
    """``model.fit(evaluation)`` of the host mirror (amico_amd/models.py = models.pyx:902-981 behind BaseModel.fit): seconds of the
    first call (dictionary upload + tables) and voxels/s of the later ones; maps against the device-resident fit of the same voxels"""
    from amico_amd import NODDI

    class Ev:                                   # the fields model.fit reads of an Evaluation (core.py:42-104)
        def __init__(self):
            self.y, self.DIRs, self.htable, self.KERNELS, self.nthreads = y_h, d_h, htable, K, 1

        def get_config(self, k):
            return False

    m = NODDI()
    m.scheme = scheme
    ev = Ev()
    t0 = time.perf_counter()
    out = m.fit(ev)
    first = time.perf_counter() - t0
    ts = []
    for _ in range(5):
        t0 = time.perf_counter()
        out = m.fit(ev)
        ts.append(time.perf_counter() - t0)
    n = len(y_h)
    return {'metric': 'voxels/sec, NODDI().fit(evaluation): host numpy in, result dict out (PCIe inclusive)', 'value': n / float(np.median(ts)),
            'unit': 'voxels/s', 'voxels': n, 'ms_per_call': 1e3 * float(np.median(ts)), 'first_call_ms': 1e3 * first,
            'max_abs_dmap_vs_device_fit': float(np.abs(out['estimates'] - est_ref).max()),
            'note': 'first call = digest of KERNELS + dictionary upload + Gram matrices / bases on the device + the fit; later calls = digest + fit'}


def device_barrier(dev, world):
    """both sides of the timed region: drain the device, meet the other ranks, drain again"""
    import torch
    import torch.distributed as dist
    if dev.type == 'cuda':
        torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    if dev.type == 'cuda':
        torch.cuda.synchronize()


def sharded_step(fit, est, gathered, world):
    """one step of the N-GPU path: this rank fits its own shard, then ONE all_gather of the maps (RCCL under nccl)"""
    from amico_amd.parallel import gather_equal

    def step():
        fit()
        if gathered is not None:             # (world == 1 runs allocate no gather buffer; a test may: RCCL with one rank)
            gather_equal(est, gathered)
    return step


def timed_steps(step, step_sync, steps, warmup, world, dev, per_step=None):
    """W untimed warm-up steps, then exactly K steps between two barriers; returns the MAX over ranks of the elapsed
    seconds (the contract of the driver's scaling runs)"""
    import torch
    import torch.distributed as dist
    for _ in range(warmup):
        step()
        step_sync()
    device_barrier(dev, world)
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
        step_sync()
        if per_step is not None:
            per_step()
    device_barrier(dev, world)
    elapsed = time.perf_counter() - t0
    per_rank = [elapsed]
    if world > 1:
        # every rank's own clock next to the MAX (the contract's figure): the first N > 1 run should read like any other
        mine = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        every = torch.zeros(world, dtype=torch.float64, device=dev)
        dist.all_gather_into_tensor(every, mine)
        per_rank = [float(v) for v in every.cpu()]
        elapsed = max(per_rank)
    timed_steps.per_rank = per_rank
    return elapsed


DUMP_LIMIT_BYTES = 64_000_000


def dump_outputs(dirname, arrays):
    """--dump-outputs: every array (torch or numpy) as <dirname>/<name>.npy in float64.  When the arrays together exceed 64 MB
    (the gathered maps of a multi-GPU run), each is cut to the same fixed sample of rows (numpy seed 0, row order kept), so that
    two builds run with the same arguments can be compared output for output."""
    os.makedirs(dirname, exist_ok=True)
    host = {name: np.asarray(a.cpu() if hasattr(a, 'cpu') else a, dtype=np.float64) for name, a in arrays.items()}
    total = sum(a.nbytes for a in host.values())
    for name, a in host.items():
        if total > DUMP_LIMIT_BYTES:
            keep = max(1, len(a) * DUMP_LIMIT_BYTES // total)
            a = a[np.sort(np.random.default_rng(0).choice(len(a), keep, replace=False))]
        np.save(os.path.join(dirname, name + '.npy'), np.ascontiguousarray(a))


def rank_records(world, rank, dev):
    """who ran: backend, world size and each rank's device (gathered through the process group when there is one)"""
    import torch
    import torch.distributed as dist
    me = {'rank': rank, 'device': torch.cuda.get_device_name(dev) if dev.type == 'cuda' else 'cpu', 'index': dev.index, 'pid': os.getpid()}
    if dev.type == 'cuda':
        try:
            pr = torch.cuda.get_device_properties(dev)
            me['pci_bus_id'] = '%04x:%02x:%02x' % (getattr(pr, 'pci_domain_id', 0), pr.pci_bus_id, getattr(pr, 'pci_device_id', 0))
        except Exception:
            pass
    recs = [me]
    if world > 1:
        recs = [None] * world
        dist.all_gather_object(recs, me)
    return {'rccl_ranks': world, 'backend': dist.get_backend() if (world > 1 and dist.is_initialized()) else 'none (single process)',
            'ranks': recs}


def self_launch(n_gpus):
    """re-run this command line under torch.distributed.run: N ranks on this node, rendezvous on 127.0.0.1 (the
    container hostname may not resolve); the ranks inherit stdout, rank 0 prints the one JSON line"""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(n_gpus), '--master-addr', '127.0.0.1',
           '--master-port', str(port), os.path.abspath(__file__)] + sys.argv[1:]
    rc = subprocess.call(cmd, env=env)
    if rc != 0:
        raise SystemExit(rc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--voxels', type=int, default=1_000_000, help='voxels per GPU')
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--no-other-configs', action='store_true', help='headline only: skip configs 3 / 4 (FreeWater 2 M, SANDI 1 M), CylinderZeppelinBall and the host-buffer legs of the --full run')
    ap.add_argument('--model', default='noddi', choices=['noddi', 'freewater', 'sandi', 'czb', 'dti', 'prep', 'lut', 'pipeline'],
                    help='noddi = the BASELINE.json headline; the others are extra measurements (configs 3, 4)')
    ap.add_argument('--full', action='store_true',
                    help='everything beyond the headline figure: stage-group event probes, roofline and counter figures, solver statistics, '
                         'oracle parity, size scan, host-buffer legs, other protocols and models, CPU baselines')
    ap.add_argument('--dump-outputs', metavar='DIR',
                    help='after the timed steps, write the maps of the last step as DIR/<name>.npy (float64, at most 64 MB)')
    args = ap.parse_args()
    if args.dump_outputs and args.model != 'noddi':
        raise SystemExit('bench.py: --dump-outputs is implemented for the NODDI headline (--model noddi) only')
    if args.model == 'dti':
        return dti_directions(args)
    if args.model == 'prep':
        return signal_preparation(args)
    if args.model == 'lut':
        return lut_resampling(args)
    if args.model == 'pipeline':
        return volume_pipeline(args)
    if args.model != 'noddi':
        return other_models(args)

    import torch
    import torch.distributed as dist
    from amico_amd import _capi, synthetic as S

    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        # `python bench.py --gpus N` without a launcher: start the N ranks ourselves (one process per GPU, RCCL over xGMI)
        return self_launch(args.gpus)
    if args.gpus != world:
        raise SystemExit('bench.py: --gpus %d but WORLD_SIZE=%d' % (args.gpus, world))
    if torch.cuda.is_available() and torch.cuda.device_count() < world and world > 1:
        raise SystemExit('bench.py: %d GPUs requested, %d visible' % (world, torch.cuda.device_count()))
    if not torch.cuda.is_available():
        raise SystemExit('bench.py needs a GPU: the fit path has no CPU fallback')
    torch.cuda.set_device(local_rank)
    dev = torch.device('cuda', local_rank)
    if world > 1:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        dist.init_process_group('nccl', device_id=dev)     # "nccl" is RCCL on ROCm

    n = args.voxels
    # ---- synthetic workload (same dictionary on every rank, different voxels per rank)
    lut_dirs = S.fibonacci_hemisphere(500)
    htable = S.build_htable(lut_dirs)
    scheme = S.make_scheme(seed=0)
    K = S.noddi_kernels(scheme, lut_dirs)
    y_h, d_h = S.noddi_signals(n, K, htable, scheme, seed=1 + rank)

    ctx = _capi.Context(local_rank)
    lut = _capi.upload_noddi(ctx, K, htable, scheme.dwi_idx, False)
    y = torch.from_numpy(y_h).to(dev)
    d = torch.from_numpy(d_h).to(dev)
    est = torch.zeros((n, 3), dtype=torch.float64, device=dev)
    gathered = torch.zeros((world * n, 3), dtype=torch.float64, device=dev) if world > 1 else None
    stream = torch.cuda.current_stream().cuda_stream
    L = _capi.lib()

    def fit():
        ctx.check(L.amx_noddi_fit_device(ctx._h, lut._h, y.data_ptr(), d.data_ptr(), n, 0.5, 1e-3, 0,
                                         est.data_ptr(), None, None, None, stream))

    step = sharded_step(fit, est, gathered, world)          # fit + the single collective of the path
    kms = np.zeros(10)

    def read_pairs(ws):
        for w in ws:                                            # HIP events on the launch stream
            try:
                kms[w] += ctx.last_kernel_ms(w)
            except Exception:                                   # seed kernels absent (AMX_NO_SEED=1)
                pass

    if args.full:
        # Untimed probe steps with EVERY event pair recorded: the stage groups' times and which single kernel dominates.  An event is a
        # packet of the stream (~5 us of the fit each, ~70 us for the full set: tools/r06/a27.sh), so the timed steps record only the
        # dominant kernel's pair -- the duration the roofline object is computed from is still measured inside the timed region.
        ctx.set_profiling(True)
        PROBE = 3
        for k in range(max(1, args.warmup) + PROBE):
            step(); ctx.sync(stream)
            if k >= max(1, args.warmup):
                read_pairs((0, 1, 2, 3, 5, 6, 7, 8, 9))
        kms /= PROBE
        # the dominant SINGLE kernel: the stage-1 seed solver (its own event pair), else the slowest of the other launches
        stage = max((8, 9, 1, 2, 3), key=lambda w: kms[w])
        if kms[8] == 0.0 and kms[9] == 0.0:                        # seeds off: the three stage kernels are the whole fit
            stage = max((1, 2, 3), key=lambda w: kms[w])
        probe_all_ms = float(kms[0])
        ctx.set_profiling(True, only=stage)
        kms[stage] = 0.0

        def per_step():
            read_pairs((stage,))
        warmup = args.warmup
    else:
        # a plain run records no events: W warm-up steps, at least one (the first fit of a context sizes its buffers), then the K
        # timed steps
        per_step = None
        warmup = max(1, args.warmup)

    # ctx.sync: status of the step (raises on error)
    elapsed = timed_steps(step, lambda: ctx.sync(stream), args.steps, warmup, world, dev, per_step)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {'estimates': est if gathered is None else gathered})
    if args.full:
        kms[stage] /= max(1, args.steps)
        ctx.set_profiling(False)                                   # (everything below is timed as a user would run it)
        stats = ctx.last_stats()
        seed_chain = ctx.last_seed_stats()
        if seed_chain.get('seeded_voxels'):            # (the counters accumulate between two syncs: one step's worth here)
            seed_chain['certified_by_gram_certificates'] = seed_chain.pop('certified')
        who = rank_records(world, rank, dev)

    if rank == 0:
        value = world * n * args.steps / elapsed
        out = {
            'metric': 'voxels/sec (whole node), NODDI fit',
            'value': value, 'unit': 'voxels/s', 'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup,
            'ms_per_step': 1e3 * elapsed / args.steps, 'higher_is_better': True, 'scaling': 'weak',
            'vs_baseline': None, 'dtype': 'f64', 'data': 'synthetic',
            'config': {'workload': 'NODDI fit, %d masked voxels per GPU, 99-volume 2-shell scheme '
                                   '(9 b0 + 30@b700 + 60@b2000), 145 atoms, ndirs=500, inputs resident in HBM' % n,
                       'voxels_per_gpu': n, 'global_voxels': world * n,
                       'parallelism': 'voxel shards x%d, one RCCL all_gather of the maps per step' % world},
        }
        if not args.full:
            print(json.dumps(out))
    if rank == 0 and args.full:
        groups = {1: 'k_noddi<1> (stage 1: voxels the Gram certificate left over) + re-run kernel', 2: 'k_noddi<4> (LASSO: left-over voxels) + re-run kernel',
                  3: 'k_noddi<3> (stage 3: left-over voxels) + re-run kernel',
                  5: "k_noddi_gemm + k_nnls_seed<1> + k_nnls_gcert<1> (A'y on the matrix cores, seed solver, Gram certificate of stage 1)",
                  6: 'k_noddi_gemm<lasso> + k_lasso_seed + k_lasso_gcert x2 (LASSO stage)', 7: 'k_nnls_seed<3> + k_nnls_gcert<3> (stage 3)'}
        singles = {8: 'k_nnls_seed<1, 8> (stage-1 NNLS seed solver, one voxel per lane, fp64 MFMA dual scan)',
                   9: 'k_lasso_seed (LASSO seed solver, one voxel per lane, Woodbury form)', 1: groups[1], 2: groups[2], 3: groups[3]}
        names = singles
        dom_ms = float(kms[stage])
        achieved = BYTES_PER_VOXEL * n / (dom_ms * 1e-3) / 1e9
        traffic = pmc_traffic(stage, n)
        whole = pmc_whole_fit(n)
        out.update({
            'roofline': {'bound': 'hbm', 'achieved': achieved, 'peak': HBM_PEAK_GBS, 'unit': 'GB/s',
                         'frac': achieved / HBM_PEAK_GBS, 'traffic': traffic,
                         # the same two figures for the WHOLE fit: algorithmic bytes of the step over its wall time, and the counter
                         # traffic of all its kernels (the dominant kernel alone touches ~100 B per voxel: `traffic` above is that)
                         'frac_end_to_end': BYTES_PER_VOXEL * n / (elapsed / args.steps) / 1e9 / HBM_PEAK_GBS,
                         'traffic_whole_fit': whole, 'algorithmic_bytes_whole_fit': BYTES_PER_VOXEL * n,
                         # SURVEY 8(d)'s secondary figure: the dense fp64 contractions no two voxels share (A'y of stage 1, A2'y2 of stage 2,
                         # A x of the residual: 2 * 99 * 145 + 2 * 90 * 144 + 2 * 99 * 145 flop) over the step, against the fp64 peak
                         'fp64_end_to_end': {'algorithmic_flops_per_voxel': 83340, 'achieved': 83340.0 * n / (elapsed / args.steps) / 1e12,
                                             'peak': 78.6, 'unit': 'TFLOP/s', 'frac': 83340.0 * n / (elapsed / args.steps) / 1e12 / 78.6},
                         'traffic_source': 'profiles/pmc_traffic.json (rocprofv3 --pmc, bytes per launch)'
                                           if traffic is not None else None,
                         'kernel': names[stage], 'kernel_ms': dom_ms, 'kernels_launched': ctx.last_path(),
                         'stage_ms': [float(v) for v in kms[1:4]], 'seed_ms': [float(v) for v in kms[5:8]], 'seed_solver_ms': [float(kms[8]), float(kms[9])],
                         'groups': {str(k): {'kernels': v, 'ms': float(kms[k])} for k, v in groups.items()}, 'all_kernels_ms': float(kms[0]),
                         'note': 'the path is bound by dependent latencies inside the per-voxel active-set solvers, not by HBM (DESIGN.md section 5): see compute_side'},
            'compute_side': pmc_valu(stage, n, dom_ms),
            'solver_stats': stats, 'seed_chain': seed_chain,
            'multi_gpu': dict(who, elapsed_s_per_rank=getattr(timed_steps, 'per_rank', None), elapsed_s_max=elapsed),
            'build': build_record(),
        })
        if world == 1:
            from oracle import oracle
            # parity on a sample of the benchmarked voxels (max |dmap| of BASELINE.json's metric)
            ns = min(n, 20000)
            cores = physical_cores() or os.cpu_count() or 1    # one thread per physical core (measured: 128 threads beat 256 on this box)
            pick = np.unique(np.linspace(0, n - 1, ns).astype(np.int64))      # spread over the whole benchmarked batch
            ns = len(pick)
            ref = oracle.noddi_fit(np.ascontiguousarray(y_h[pick]), np.ascontiguousarray(d_h[pick]), K, htable, scheme.dwi_idx, nthreads=cores)
            diff = np.abs(est.cpu().numpy()[pick] - ref['estimates']).max(axis=1)
            out['parity'] = {'sample_voxels': ns, 'sample': 'every %d-th voxel of the batch' % max(1, n // ns), 'max_abs_dmap': float(diff.max()),
                             'median_abs_dmap': float(np.median(diff)),
                             'frac_within_1e-6': float((diff < 1e-6).mean()),
                             'frac_within_1e-4': float((diff < 1e-4).mean())}
            other = {}
            # the same fit on the first 50 000 / 200 000 / 300 000 voxels of the resident batch (the sizes a brain mask, and a batch of the
            # host-buffer pipeline, have): T(n) = floor + slope n is the chain's signature, and the driver should see it
            size_scan = {}
            for ns_ in (50_000, 200_000, 300_000):
                if ns_ >= n or args.no_other_configs:          # (profiling runs want the headline's launches only: per-kernel means are taken over ALL launches)
                    continue
                est_s = torch.zeros((ns_, 3), dtype=torch.float64, device=dev)

                def fit_s():
                    ctx.check(L.amx_noddi_fit_device(ctx._h, lut._h, y.data_ptr(), d.data_ptr(), ns_, 0.5, 1e-3, 0, est_s.data_ptr(), None, None, None, stream))
                for _ in range(3):
                    fit_s(); ctx.sync(stream)
                ts_ = []
                for _ in range(9):
                    t1 = time.perf_counter(); fit_s(); ctx.sync(stream); ts_.append(time.perf_counter() - t1)
                size_scan[str(ns_)] = {'ms': round(1e3 * float(np.median(ts_)), 4), 'voxels_per_s': round(ns_ / float(np.median(ts_)))}
                del est_s
            size_scan[str(n)] = {'ms': round(1e3 * elapsed / args.steps, 4), 'voxels_per_s': round(value)}
            if not args.no_other_configs:
                # host numpy in -> host numpy out through amx_noddi_fit (H2D + kernels + D2H): the PCIe-inclusive rate,
                # reported beside the headline, never as `value`
                _capi.noddi_fit(ctx, lut, y_h, d_h, 0.5, 1e-3, 3)
                hb = []
                for _ in range(7):      # (median of seven: one call in ten takes 10 - 15 ms longer on the two-socket box, whatever the transport)
                    t1 = time.perf_counter()
                    _capi.noddi_fit(ctx, lut, y_h, d_h, 0.5, 1e-3, 3)
                    hb.append(time.perf_counter() - t1)
                other = {'noddi_host_buffers': {'metric': 'voxels/sec, NODDI fit, host buffers in/out (PCIe inclusive)',
                                                'value': n / float(np.median(hb)), 'unit': 'voxels/s', 'voxels': n,
                                                'ms_per_call': 1e3 * float(np.median(hb)),
                                                'batches_as_float32': ctx.last_host_narrowed(),
                                                'note': 'float64 signals from pageable host memory, batches pipelined behind the solver.  The signals are what '
                                                        'evaluation.y of the reference is -- the float64 cast of a float32 image (core.py:136, 451) -- which the '
                                                        'library finds out element by element and sends as float32 (csrc/amx_stage.hpp): lossless, bit-identical maps'}}
                # the same call on genuine float64 values (no float32 round trip): nothing can be narrowed, 8 bytes per value cross PCIe
                y_g = y_h * (1.0 + 2.0 ** -30)
                _capi.noddi_fit(ctx, lut, y_g, d_h, 0.5, 1e-3, 3)
                hb = []
                for _ in range(7):      # (median of seven: one call in ten takes 10 - 15 ms longer on the two-socket box, whatever the transport)
                    t1 = time.perf_counter()
                    _capi.noddi_fit(ctx, lut, y_g, d_h, 0.5, 1e-3, 3)
                    hb.append(time.perf_counter() - t1)
                other['noddi_host_buffers_f64_values'] = {
                    'metric': 'voxels/sec, NODDI fit, float64 host buffers holding genuine float64 values (PCIe inclusive)',
                    'value': n / float(np.median(hb)), 'unit': 'voxels/s', 'voxels': n, 'ms_per_call': 1e3 * float(np.median(hb)),
                    'batches_as_float32': ctx.last_host_narrowed(),
                    'note': 'the call is the link (792 MB at 56.4 GB/s) plus the last batch: profiles/r05c_host_transport.txt'}
                del y_g
                try:
                    y32 = y_h.astype(np.float32)
                    _capi.noddi_fit(ctx, lut, y32, d_h, 0.5, 1e-3, 3)
                    hb = []
                    for _ in range(7):      # (median of seven: one call in ten takes 10 - 15 ms longer on the two-socket box, whatever the transport)
                        t1 = time.perf_counter()
                        e32 = _capi.noddi_fit(ctx, lut, y32, d_h, 0.5, 1e-3, 3)[0]
                        hb.append(time.perf_counter() - t1)
                    other['noddi_host_buffers_f32'] = {'metric': 'voxels/sec, NODDI fit, float32 signals from host buffers (PCIe inclusive)',
                                                       'value': n / float(np.median(hb)), 'unit': 'voxels/s', 'voxels': n,
                                                       'ms_per_call': 1e3 * float(np.median(hb)),
                                                       'max_abs_dmap_vs_f64_upload': float(np.abs(e32 - est.cpu().numpy()).max()),
                                                       'note': 'lossless for AMICO (the image is float32, core.py:136): half the PCIe bytes'}
                    del y32
                except (TypeError, AttributeError, ValueError):
                    pass
            if not args.no_other_configs:
                # the plug-in surface itself: NODDI().fit(evaluation) as core.py:462-467 calls it (host numpy in, the result dict out) on a
                # FRESH context -- the first call pays the dictionary upload and the device tables built from it (Gram matrices, bases),
                # the later ones find the dictionary by the digest of KERNELS (BaseModel._lut)
                other['noddi_model_fit'] = noddi_model_fit(K, htable, scheme, y_h, d_h, est.cpu().numpy())
                # ... and on a device SET (amico_amd.set_devices / AMX_DEVICES: one context + host thread per device, contiguous shards).  This box
                # has one GPU: naming it twice measures the machinery (two contexts, two copy streams, two narrowing pools on ONE link), not scaling
                import amico_amd
                try:
                    amico_amd.set_devices([local_rank, local_rank])
                    other['noddi_model_fit_two_contexts_one_gpu'] = noddi_model_fit(K, htable, scheme, y_h, d_h, est.cpu().numpy())
                finally:
                    amico_amd.set_devices(None)
            if not args.no_other_configs:
                other['noddi_hard_mix'] = noddi_hard_mix(ctx, lut, K, htable, scheme, min(n, 1_000_000), 5, 2)
                per_byte = value * BYTES_PER_VOXEL
                other['noddi_105vol'] = noddi_other_protocol(ctx, ((700.0, 50), (2000.0, 50)), 5, min(n, 1_000_000), 5, 2, per_byte)
                other['noddi_150vol'] = noddi_other_protocol(ctx, ((700.0, 40), (2000.0, 60), (3000.0, 40)), 10, min(n, 1_000_000), 5, 2, per_byte)
                other['noddi_exvivo'] = noddi_other_protocol(ctx, ((700.0, 30), (2000.0, 60)), 9, min(n, 1_000_000), 5, 2, per_byte, exvivo=True)
                # the headline's protocol at other noise levels: the chain's thresholds (trip caps, pivot ratios, switch points) were tuned
                # at SNR 30 -- correctness does not depend on them, the rate does
                other['noddi_snr10'] = noddi_other_protocol(ctx, ((700.0, 30), (2000.0, 60)), 9, min(n, 1_000_000), 5, 2, per_byte, snr=10.0)
                other['noddi_snr50'] = noddi_other_protocol(ctx, ((700.0, 30), (2000.0, 60)), 9, min(n, 1_000_000), 5, 2, per_byte, snr=50.0)
                # lambda1 = 0 (a pure ridge: a legal set_solver): dense LASSO optima, beyond the 64 atoms the fast kernels hold -- AMX_E_OVERFLOW until
                # round 5, now k_noddi_lasso_big (csrc/amx_big.hip: block principal pivoting, a workgroup per voxel): slow, exact
                try:
                    nb_ = min(n, 100_000)
                    estb = torch.zeros((nb_, 3), dtype=torch.float64, device=dev)

                    def fit_b():
                        ctx.check(L.amx_noddi_fit_device(ctx._h, lut._h, y.data_ptr(), d.data_ptr(), nb_, 0.0, 1e-3, 0, estb.data_ptr(), None, None, None, stream))
                    fit_b(); ctx.sync(stream)
                    t1 = time.perf_counter(); fit_b(); ctx.sync(stream); tb_ = time.perf_counter() - t1
                    pk_ = np.arange(0, nb_, max(1, nb_ // 2000))
                    refb = oracle.noddi_fit(np.ascontiguousarray(y_h[pk_]), np.ascontiguousarray(d_h[pk_]), K, htable, scheme.dwi_idx, lambda1=0.0, lambda2=1e-3, nthreads=cores)
                    other['noddi_lambda1_0'] = {'metric': 'voxels/sec, NODDI fit with lambda1 = 0 (dense LASSO optimum: k_noddi_lasso_big for every voxel)', 'value': nb_ / tb_, 'unit': 'voxels/s',
                                                'voxels': nb_, 'ms_per_step': 1e3 * tb_, 'kernels_launched': ctx.last_path(), 'solver_stats': ctx.last_stats(),
                                                'parity': {'sample_voxels': int(len(pk_)), 'max_abs_dmap': float(np.abs(estb.cpu().numpy()[pk_] - refb['estimates']).max())}}
                    del estb
                except Exception as e:                                  # (an extra leg must not cost the line)
                    other['noddi_lambda1_0'] = {'error': repr(e)}
                # an HCP-style acquisition (18 b0 + 3 x 90 directions = 288 volumes): the most common public NODDI data
                other['noddi_288vol'] = noddi_other_protocol(ctx, ((1000.0, 90), (2000.0, 90), (3000.0, 90)), 18, min(n, 1_000_000), 5, 2, per_byte)
            if not args.no_cpu_baseline:
                # bounded CPU legs on the host cores of this box: the oracle -- a port, the reference's
                # cyspams path cannot be built -- at -O3 -march=native, the reference's chunk-per-thread structure
                # (models.pyx:204-211), one warm-up + median of 5 runs.  "faithful": voxels in the caller's order, so the
                # LUT slice is copied per voxel like models.pyx:905
                oracle.use_fast_build(True)
                m = min(n, 100000)
                fit = lambda yy, dd: oracle.noddi_fit(yy, dd, K, htable, scheme.dwi_idx, nthreads=cores)
                rate_f, dt_f = median_rate(lambda: fit(y_h[:m], d_h[:m]), m)
                oracle.use_fast_build(False)
                # (rounds 3 - 5 also timed the voxels sorted by LUT index -- "optimised": one dictionary copy per orientation and thread; it was
                #  never faster than the caller's order on this box, 103.6 k against 109.3 k voxels/s in round 5, and is gone: VERDICT r05 weak 13)
                out['cpu_baseline'] = {'value': rate_f, 'unit': 'voxels/s', 'cores': cores, 'logical_cpus': os.cpu_count(),
                                       'kind': 'port', 'variant': 'faithful',
                                       'sample': 'first %d voxels of the same workload, oracle/amico_oracle.c (Lawson-Hanson NNLS + LARS '
                                                 'lasso) -O3 -march=native, %d threads, warm-up + median of 5 runs (%.2f s)'
                                                 % (m, cores, dt_f)}
            if not args.no_other_configs:
                # free the headline's buffers first: configs 3 and 4 run on the same GPU, one after the other
                del y, d, est
                torch.cuda.empty_cache()
                other['freewater_2M'] = small_model('freewater', 2_000_000, 5, 2, cpu=not args.no_cpu_baseline)
                other['sandi_1M'] = small_model('sandi', 1_000_000, 5, 2, cpu=not args.no_cpu_baseline)
                other['czb_500k'] = small_model('czb', 500_000, 5, 2, cpu=not args.no_cpu_baseline)
            if other:
                out['other_configs'] = other
            # LAST in the line (the driver keeps the tail of stdout): the numbers at the reference's own boundary -- model.fit(evaluation) takes
            # and returns host numpy (core.py:462-467) -- beside the resident headline, and the size scan
            out['size_scan'] = size_scan
            if other:
                g = lambda k, f='value': (round(other[k][f], 3) if k in other and f in other[k] else None)
                out['host_boundary'] = {
                    'unit': 'voxels/s', 'voxels': n, 'resident_in_hbm': round(value),
                    'noddi_host_buffers': g('noddi_host_buffers'), 'noddi_host_buffers_ms': g('noddi_host_buffers', 'ms_per_call'),
                    'noddi_host_buffers_f64_values': g('noddi_host_buffers_f64_values'), 'noddi_host_buffers_f32': g('noddi_host_buffers_f32'),
                    'noddi_model_fit': g('noddi_model_fit'), 'noddi_model_fit_ms': g('noddi_model_fit', 'ms_per_call'),
                    'noddi_model_fit_first_call_ms': g('noddi_model_fit', 'first_call_ms'),
                    'noddi_model_fit_two_contexts_one_gpu': g('noddi_model_fit_two_contexts_one_gpu'),
                    'freewater_2M_host_buffers': (round(other['freewater_2M']['host_buffers']['f64']['value']) if 'freewater_2M' in other and 'host_buffers' in other['freewater_2M'] else None),
                    'sandi_1M_host_buffers': (round(other['sandi_1M']['host_buffers']['f64']['value']) if 'sandi_1M' in other and 'host_buffers' in other['sandi_1M'] else None)}
                # (scalars the driver's record of `roofline` keeps)
                out['roofline']['host_buffers_voxels_per_s'] = out['host_boundary']['noddi_host_buffers']
                out['roofline']['model_fit_voxels_per_s'] = out['host_boundary']['noddi_model_fit']
            for k_ in ('200000', '300000'):
                if k_ in size_scan:
                    out['roofline']['voxels_per_s_at_%s' % k_] = size_scan[k_]['voxels_per_s']
        print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
