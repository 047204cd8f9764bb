#!/usr/bin/env python3
"""FreeWater, SANDI and CylinderZeppelinBall on dictionaries of more than 64 atoms (csrc/amx_enet_big.hip) against what a user could do
before that route existed: amx_lasso_batched_device on a dictionary marked dense (k_batched + k_batched_big), which holds the same
dictionaries, takes the same voxels and dict_idx, and gives x only -- no maps.  100 000 voxels resident in HBM (float64), hard-mix signals
(tests/small_np.hard_mix: every third voxel all-zero, one atom, pure noise ...) over three LUT orientations, the two legs ALTERNATING in one
process, device events, one warm-up pair, then --reps pairs: median and spread of each leg.  The oracle's loop (16 threads) on a sample of
the same voxels on the same box stands beside them.

  czb_40x130      CylinderZeppelinBall 40 volumes x 130 atoms, lambda2 = 4    (dense optimum: the batched call's 16- and 48-atom passes fail first)
  fw_33x101       FreeWater 33 x 101, lambda2 = 1e-3
  sandi_6x65      SANDI 6 x 65, lambda2 = 5e-3
  sandi_306x66    SANDI 306 x 66 (no directional average), lambda2 = 5e-3

    python tools/time_big_dictionaries.py [--voxels 100000] [--reps 5] [--case NAME]
Every line starts with the library's amx_build_id.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
CASES = ('czb_40x130', 'fw_33x101', 'sandi_6x65', 'sandi_306x66')
BASE = 6144          # voxels made on the host (2 048 per orientation), repeated on the device


def problem(name):
    """(model, upload(ctx) -> Lut, A [n_dicts, m, n], lams, y [BASE, m], idx [BASE] int32, dirs [BASE, 3] or None, oracle(y, d) -> None)"""
    import big_np as B
    import small_np as N
    from amico_amd import _capi, synthetic as S
    from oracle import oracle
    h = N._htable()
    rng = np.random.default_rng(7)
    if name.startswith('sandi'):
        if name == 'sandi_6x65':
            K, Rs, d_in, d_isos = B.dictionary('sandi_6x65')
        else:
            sch = S.make_sandi_scheme()
            K, Rs, d_in, d_isos = S.sandi_kernels(sch, Rs=np.linspace(1.0, 12.0, 22) * 1e-6, d_in=np.linspace(0.25, 3.0, 22) * 1e-3,
                                                  d_isos=np.linspace(0.25, 3.0, 22) * 1e-3)
        A = N.sandi_matrix(K)
        y, _ = N.hard_mix(A, N.easy_signals(A, BASE, rng, snr=50.0), 1)
        return ('sandi', lambda ctx: _capi.upload_sandi(ctx, K, Rs, d_in, d_isos), A[None], N.SANDI_DEFAULT, y, np.zeros(BASE, np.int32), None,
                lambda yy, dd: oracle.sandi_fit(yy, K, Rs, d_in, d_isos, *N.SANDI_DEFAULT, nthreads=16))
    D = B.dictionary(name)
    idx = rng.permutation(np.repeat(np.arange(3, dtype=np.int32), BASE // 3))
    dirs = np.ascontiguousarray(h['dirs'][B.ORI[idx]], dtype=np.float64)
    A = np.stack([B.matrix(name, lid) for lid in B.ORI])
    y = np.zeros((BASE, A.shape[1]))
    for k in range(3):
        rows = np.flatnonzero(idx == k)
        y[rows], _ = N.hard_mix(A[k], N.easy_signals(A[k], len(rows), rng), 11 + k)
    if name.startswith('fw'):
        return ('freewater', lambda ctx: _capi.upload_freewater(ctx, D[0], h['htable']), A, N.FW_DEFAULT, y, idx, dirs,
                lambda yy, dd: oracle.freewater_fit(yy, dd, D[0], h['htable'], *N.FW_DEFAULT, nthreads=16))
    return ('czb', lambda ctx: _capi.upload_czb(ctx, D[0], D[1], h['htable']), A, B.CZB_DEFAULT, y, idx, dirs,
            lambda yy, dd: oracle.czb_fit(yy, dd, D[0], D[1], h['htable'], *B.CZB_DEFAULT, nthreads=16))


def run(name, n, reps):
    import torch
    from amico_amd import _capi, get_context
    tag = _capi.build_id()
    model, upload, A, lam, y, idx, dirs, oracle_fit = problem(name)
    rep = -(-n // BASE)
    d_y = torch.from_numpy(y).cuda().repeat(rep, 1)[:n].contiguous()
    d_idx = torch.from_numpy(idx).cuda().repeat(rep)[:n].contiguous()
    d_dirs = None if dirs is None else torch.from_numpy(dirs).cuda().repeat(rep, 1)[:n].contiguous()
    d_x = torch.zeros((n, A.shape[2]), dtype=torch.float64, device='cuda')
    ctx = get_context()
    lut = upload(ctx)
    dic = _capi.Dict(ctx, A, dense=True)
    L = _capi.lib()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def fit_model():
        if model == 'sandi':
            return _capi.sandi_fit_device(ctx, lut, d_y, *lam)
        if model == 'freewater':
            return _capi.freewater_fit_device(ctx, lut, d_y, d_dirs, lam[0], lam[1], False)
        return _capi.czb_fit_device(ctx, lut, d_y, d_dirs, *lam)

    def fit_batched():
        ctx.check(L.amx_lasso_batched_device(ctx._h, dic._h, d_idx.data_ptr(), d_y.data_ptr(), n, lam[0], lam[1], d_x.data_ptr(), None))
    ms = {'model': [], 'batched': []}
    paths, stats = {}, {}
    for k in range(reps + 1):                                  # one warm-up pair (workspace, tables), then the timed pairs, alternating
        for leg, fn in (('model', fit_model), ('batched', fit_batched)):
            ev[0].record()
            fn()
            ev[1].record()
            torch.cuda.synchronize()
            ctx.sync()
            if k:
                ms[leg].append(ev[0].elapsed_time(ev[1]))
            paths[leg], stats[leg] = ctx.last_path(), ctx.last_stats()
    paths['batched'] = paths['batched'].replace(paths['model'] + ' -> ', '')      # (amx_last_path starts afresh with a model fit only)
    dense = ctx.last_dense()
    shape = f'{A.shape[1]} volumes x {A.shape[2]} atoms, lambda = ({lam[0]:g}, {lam[1]:g})'
    for leg in ('model', 'batched'):
        t, lo, hi = float(np.median(ms[leg])), min(ms[leg]), max(ms[leg])
        print(f'{tag} | {name} {leg:7s}: {n} voxels, {shape}: median {t:.1f} ms (min {lo:.1f}, max {hi:.1f}, {reps} fits), {n / t / 1e3:.3f} M voxels/s '
              f'[{paths[leg]}] itercap {stats[leg]["itercap_voxels"]} guard {stats[leg]["guard_trips"]}'
              + (f' dense voxels {dense["voxels"]} steps {dense["steps"]}' if leg == 'batched' else ''))
    tm, tb = float(np.median(ms['model'])), float(np.median(ms['batched']))
    print(f'{tag} | {name}: model fit / batched call = {tm / tb:.2f} (below 1: the model fit, maps included, is the faster)')
    m = min(2048, n)
    t0 = time.perf_counter()
    oracle_fit(y[:m], None if dirs is None else dirs[:m])
    dt = time.perf_counter() - t0
    print(f'{tag} | {name} oracle : {m} voxels, 16 threads: {dt * 1e3:.0f} ms, {m / dt / 1e6:.4f} M voxels/s', flush=True)
    lut.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--voxels', type=int, default=100000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--case', choices=CASES)
    a = ap.parse_args()
    for name in ([a.case] if a.case else CASES):
        run(name, a.voxels, a.reps)


if __name__ == '__main__':
    main()
