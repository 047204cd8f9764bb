"""The seeded NODDI chain at every shape edge its route has, on hard voxels, each voxel held to its own Kuhn-Tucker certificate and to
the CPU oracle.

The cases and the edge each is there for are the table noddi_np.CASES: dictionaries of 13 .. 226 atoms, protocols of 41 .. 512 volumes,
the repair / rescue / third / exact passes forced on and off, the QR solver at a weak ridge, a weak lambda1, and three calls of 600 000
voxels for what only a call's size selects.  The signals are noddi_np.hard_signals: synthetic.noddi_hard_signals on three orientations of
2 100, 835 and 65 voxels (with AMX_SEED_CHUNK=256: nine seed chunks with a ragged last one, four, a quarter of one), amplitudes 2^-8, 1
and 2^6 side by side (lambda1 is absolute: empty supports, supports of up to 26 atoms, and supports beyond the 64 atoms the re-run kernel
holds, which reach k_noddi_lasso_big through the overflow lists).  Every case first asserts its route from Context.last_path() and
last_seed_stats()['seeded_voxels'].  Then, with s = max|y| of the voxel, EVERY voxel is held to:

* finite results, min x >= 0 in all three stages; an all-zero voxel has x exactly 0 and the maps NDI 0, ODI 1, FWF 0;
* the certificate of the device x (kkt_certificates.noddi_certificates_per_voxel, long-double residuals): |g_P| < 1e-9 s and g_Z < 1e-9 s in
  each stage -- the project's W_P_TOL / W_Z_TOL, per voxel and relative --, stage-3 coefficients off the allowed set exactly zero;
* x_iso of stage 1 within 1e-7 s of the oracle's;
* stage-2 x within czb_np.x_bound(n_wm, lambda2) s of the oracle's; where that bound exceeds 1e-6 (every lambda2 used here), A2 x within
  1e-4 s instead; supports equal to the oracle's except on atoms the oracle marks degenerate (within 1e-7 s of zero);
* maps: noddi_np.noddi_maps of the DEVICE x to 1e-12 relative, and within 1e-6 of the oracle's on every voxel whose stage-2 support equals
  the oracle's.  A voxel whose support differs on degenerate atoms only is excused from that last comparison alone (at most 1 % of a
  case); a support that differs on any other atom is a failure;
* itercap_voxels == 0, guard_trips == 0, overflow_voxels == 0.  (overflow_voxels counts what the one-wavefront re-run kernels could not
  hold -- misc[12] / misc[13], k_fold_stats --; the voxels k_noddi_lasso_big settles come from a list of their own, misc[14], and are not
  in it: the counter is zero however many supports exceed 64 atoms, and anything else is an error of the fit);
* the table k_noddi_gemm made of the signals (small cases that run it): a_j'y of every atom, sum_b0 y, ||y||^2 and sum_b0 y^2 of every
  voxel against numpy in long double, within the bound of a float64 dot product (_check_table).  The certificates REFUSE a seed whose
  table entries are wrong and the left-over kernels then solve the voxel from the signal itself, so that a table kernel which skips a
  tile of atoms leaves every map right and every count below n: only the table itself shows it;
* non-vacuity: the left-over counts of last_seed_stats() the case names are non-zero and below n;
* two more voxels, one with a NaN sample and one with +Inf in the last sample, give NaN maps and change no other voxel's bits;
* error maps where the case asks: |rmse - rmse_ld(device x)| <= 1e-9 rmse + 3e-8 rms(y), NRMSE likewise -- the floor
  test_gpu_amplitude._compare_scaled documents for Gram-form residuals.

A large call tiles the 3 000 voxels of its small case to 600 000, every period rotated by one voxel; the first copy gets all of the
above, every other copy must have x equal to its first copy's within 1e-12 s elementwise (compared on the device), and a copy that does
not is certified on its own.  test_noddi_hard.py shows on the CPU that the oracle meets this standard with two digits to spare.

MEASURED on an MI355X (profiles/noddi_hard_kkt.txt): all 40 cases pass.  Worst gP / s 6.9e-13 (v512; the oracle reaches 1.3e-12 there), gZ / s 0
in every case (no clamped atom of any voxel has a positive dual value), A2 x at most 2.9e-6 of its bound (vLDS), maps within 3.3e-10 of
the oracle's, no voxel excused, no copy of a large call off its first copy; the table of k_noddi_gemm at most 0.64 of the dot-product
bound.  No kernel defect came out of it.  The mutation check (scratch build, not committed): the second window of the table kernel cut
by one K-step fails v161 and v512 on the table, the certificate (2 954 voxels, gP / s 2.1) and the maps; the last float32 tile's rows
left unwritten fails d144, d146x, v161 and v512 on the table ALONE -- certificate, maps and left-over counts stay clean, because the
certificates refuse what the table gets wrong -- and leaves d13 (no float32 tile) passing."""
import numpy as np
import pytest

import czb_np as Z
import noddi_np as N

pytestmark = pytest.mark.gpu

ZERO_MAPS = np.array([0.0, 1.0, 0.0, 0.0])


def _route(c, n, path, ss):
    p = path + ' ->'
    miss = [m for m in c['must'] if m not in p]
    has = [m for m in c['must_not'] if m in p]
    assert not miss and not has, ('route', 'missing', miss, 'has', has, path)
    assert ss['seeded_voxels'] == (n if c['seeded'] else 0), ss
    assert ('k_noddi_lasso_big' in path) == c['big_in_path'], path


def _stats(ctx, c, n, found, check_left):
    st, ss = ctx.last_stats(), ctx.last_seed_stats()
    if not (st['itercap_voxels'] == 0 and st['guard_trips'] == 0 and st['overflow_voxels'] == 0):
        found.append(('solver statistics', st))
    if check_left:
        for k in c['left']:
            if not 0 < ss[k] < n:
                found.append(('vacuous: ' + k, ss))
    return ss


def _same_bits(clean, dirty, n):
    """the run with the two bad voxels behind: NaN maps for them, every other voxel's results to the last bit what they were"""
    import torch
    found = []
    for k, (a, b) in enumerate(zip(clean, dirty)):
        if a is None:
            continue
        if k == 0 and not bool(torch.isnan(b[n:]).all()):
            found.append(('maps of the bad voxels', b[n:].cpu().numpy().tolist()))
        if not torch.equal(a, b[:n]):
            w = torch.nonzero((a != b[:n]).reshape(n, -1).any(dim=1)).flatten()
            found.append(('a bad voxel changed others', 'output', k, 'voxels', int(w.numel()), int(w[0])))
    return found


def _check(name, label, path, x, est, rmse, nrmse):
    """the first 3 000 voxels of a case against certificate and oracle; returns what it found wrong, one entry per property"""
    from amico_amd import synthetic as S
    c = N.CASES[name]
    sch, K, y, d, kind, amp = N.problem(name)
    ref = N.reference(name)
    xo, mo = ref['x'], ref['estimates']
    lam2 = c['lam'][1]
    n, n_wm, n_maps = len(y), K['wm'].shape[0], est.shape[1]
    s = N.scale_of(y)
    live = s > 0
    sc = np.where(live, s, 1.0)
    found = []
    if not (np.isfinite(x).all() and np.isfinite(est).all()):
        return ['non-finite results on %d finite voxels' % int((~np.isfinite(x).reshape(n, -1).all(axis=1) | ~np.isfinite(est).all(axis=1)).sum())]
    if x[~live].any() or not (np.abs(est[~live] - ZERO_MAPS[None, :n_maps]) <= 1e-12).all():
        found.append(('an all-zero voxel with a non-zero x or maps other than 0, 1, 0', est[~live].tolist()))
    # Kuhn-Tucker conditions of the device coefficients, per voxel
    cert = N.certificates(name, x)
    bad = N.kkt_failures(cert)
    gp = np.max([cert['gP%d' % k] for k in (1, 2, 3)], axis=0)
    gz = np.max([cert['gZ%d' % k] for k in (1, 2, 3)], axis=0)
    if bad.any():
        w = np.flatnonzero(bad)
        found.append(('certificate', 'voxels', len(w), 'first', int(w[0]), {k: float(cert[k][live].max()) for k in ('gP1', 'gZ1', 'gP2', 'gZ2', 'gP3', 'gZ3', 'off3')},
                      'min x', float(x.min()), 'kinds', sorted(set(S.HARD_KINDS[k] for k in kind[w])), 'amplitudes', sorted(set(N.AMPS[a] for a in amp[w]))))
    # stage 1 hands x_iso on
    diso = np.abs(x[:, 0, -1] - xo[:, 0, -1]) / sc
    if not (diso <= N.XISO_TOL).all():
        found.append(('x_iso of stage 1', 'voxels', int((diso > N.XISO_TOL).sum()), 'worst', float(diso.max()), int(diso.argmax())))
    # stage-2 x (or A2 x) against the oracle
    unit = Z.x_bound(n_wm, lam2)
    x2, xo2 = x[:, 1, :n_wm], xo[:, 1, :n_wm]
    if unit <= 1e-6:
        ratio, what = np.abs(x2 - xo2).max(axis=1) / (unit * sc), '|dx|/bound'
    else:
        ratio, what = np.abs(N.stage2_product(K, sch, d, x2 - xo2, c['exvivo'])).max(axis=1) / (N.AX_TOL * sc), '|A dx|/bound'
    if not (ratio <= 1.0).all():
        w = np.flatnonzero(ratio > 1.0)
        found.append(('stage-2 x against the oracle', 'voxels', len(w), 'worst', float(ratio.max()), int(ratio.argmax()), sorted(set(S.HARD_KINDS[k] for k in kind[w]))))
    # supports
    mism = (x2 > 0) != (xo2 > 0)
    deg = N.degenerate(xo2, N.reference_certificates(name)['g2'], N.DEGENERATE * s)
    wrong = (mism & ~deg).any(axis=1)
    excused = mism.any(axis=1) & ~wrong
    if wrong.any():
        w = np.flatnonzero(wrong)
        found.append(('support differs on a non-degenerate atom', 'voxels', len(w), int(w[0]), sorted(set(S.HARD_KINDS[k] for k in kind[w])),
                      'amplitudes', sorted(set(N.AMPS[a] for a in amp[w]))))
    if excused.mean() > N.MAX_SHARE:
        found.append(('too many voxels excused', int(excused.sum())))
    # maps: the arithmetic alone, then against the oracle
    mine = N.noddi_maps(x[:, 2], K, c['exvivo'])
    err = np.abs(est - mine) - (1e-12 * np.abs(mine) + 1e-300)
    if not (err <= 0.0).all():
        w = int(err.max(axis=1).argmax())
        found.append(('maps of the device x', 'voxels', int((err > 0).any(axis=1).sum()), w, est[w].tolist(), mine[w].tolist()))
    dm = np.abs(est - mo).max(axis=1)
    miss = ~(dm < N.MAP_TOL) & ~mism.any(axis=1)
    if miss.any():
        w = np.flatnonzero(miss)
        found.append(('maps against the oracle', 'voxels', len(w), 'worst', float(dm[w].max()), int(w[dm[w].argmax()]), sorted(set(S.HARD_KINDS[k] for k in kind[w])),
                      'amplitudes', sorted(set(N.AMPS[a] for a in amp[w]))))
    # error maps
    if rmse is not None:
        g = N.groups_of(K, d, c['exvivo'])
        rms = np.sqrt((y * y).mean(axis=1))
        r = N.rmse_ld(g, y, x[:, 2])
        b = ~(np.abs(rmse - r) <= 1e-9 * r + 3e-8 * rms)
        if b.any():
            found.append(('rmse', 'voxels', int(b.sum()), int(np.flatnonzero(b)[0]), float(rmse[b][0]), float(r[b][0]), float(rms[b][0])))
        r = N.nrmse_ld(g, y, x[:, 2])
        b = ~(np.abs(nrmse - r) <= 1e-9 * r + 3e-8)
        if b.any():
            found.append(('nrmse', 'voxels', int(b.sum()), int(np.flatnonzero(b)[0]), float(nrmse[b][0]), float(r[b][0])))
    w = int(np.argmax(np.where(live, np.maximum(np.maximum(gp, gz) / N.KKT, ratio), 0.0)))
    print('NODDIHARD %-14s gP/s %.2e  gZ/s %.2e  %s %.2e  dmap %.2e  excused %d  worst: %s x %g  | %s' %
          (label, gp[live].max(), gz[live].max(), what, ratio.max(), dm[~mism.any(axis=1)].max(), int(excused.sum()), S.HARD_KINDS[kind[w]], N.AMPS[amp[w]], path))
    return found


def _check_table(ctx, name, n):
    """the A'y table k_noddi_gemm left in the workspace (amx_debug_fetch: 7 misc -- word 1 is the number of seed chunks --, 6 the chunks
    {orientation, start, count, first block}, 0 the voxel permutation, 5 the table f64 [block][rows][64]; voxel k of a chunk sits in
    block pad + k / 64, column k % 64) against numpy in long double: the rows a_j'y of every atom, sum_b0 y, ||y||^2 and sum_b0 y^2 of
    EVERY voxel, each within the bound of a float64 dot product of nS terms, nS 2^-53 |a_j|'|y| -- whatever the left-over kernels mend
    afterwards, a row the kernel did not write, or wrote from too few samples, shows here"""
    from amico_amd import _capi
    c = N.CASES[name]
    sch, K, y, d, _, _ = N.problem(name)
    nS, n_atoms = sch.nS, K['wm'].shape[0] + (2 if c['exvivo'] else 1)
    rows = ((n_atoms + 28 + 15) // 16) * 16
    n_sch = int(_capi.debug_fetch(ctx, None, 'misc', (2,), np.int32)[1])
    ch = _capi.debug_fetch(ctx, None, 'schunks', (n_sch, 4), np.int32)
    perm = _capi.debug_fetch(ctx, None, 'perm', (n,), np.int32)
    ch = ch[ch[:, 2] > 0]
    if sorted(perm.tolist()) != list(range(n)) or ch[:, 2].sum() != n:
        return [('table: the chunks do not cover the voxels once', int(ch[:, 2].sum()))]
    n_blocks = int((ch[:, 3] + (ch[:, 2] + 63) // 64).max())
    C = _capi.debug_fetch(ctx, None, 'cgemm', (n_blocks, rows, 64), np.float64)
    b0 = np.zeros(nS)
    b0[np.asarray(sch.b0_idx)] = 1.0
    iso = K['iso'].astype(np.float64)
    fixed = ([np.ones(nS)] if c['exvivo'] else []) + [iso]
    worst, bad = 0.0, 0
    for dr, start, count, pad in ch:
        vox = perm[start:start + count]
        A = np.concatenate([K['wm'][:, dr, :].astype(np.float64)] + [f[None, :] for f in fixed] + [b0[None, :]], axis=0).T      # nS x (n_atoms + 1)
        Y = y[vox]
        ref = np.concatenate([(Y.astype(N.LD) @ A.astype(N.LD)), (Y.astype(N.LD) ** 2).sum(axis=1)[:, None], ((Y * b0).astype(N.LD) ** 2).sum(axis=1)[:, None]],
                             axis=1).astype(np.float64)
        tol = nS * 2.0 ** -53 * np.concatenate([np.abs(Y) @ np.abs(A), (Y ** 2).sum(axis=1)[:, None], ((Y * b0) ** 2).sum(axis=1)[:, None]], axis=1)
        k = np.arange(count)
        got = C[pad + k // 64, :, k % 64]                                                                                      # count x rows
        got = np.concatenate([got[:, :n_atoms], got[:, [n_atoms + 24, n_atoms + 25, n_atoms + 26]]], axis=1)
        err = np.abs(got - ref)
        bad += int((~(err <= tol)).any(axis=1).sum())
        worst = max(worst, float((err / np.maximum(tol, 1e-300)).max()))
    print('NODDIHARD %-14s table of k_noddi_gemm: worst error %.2f of the dot-product bound' % (name, worst))
    return [('table of k_noddi_gemm', 'voxels', bad, 'worst error / bound', worst)] if bad else []


def _check_copies(name, xd, est_t, yb, db, n):
    """a large call: every copy of a voxel has the x of its first copy within 1e-12 s elementwise (and maps within 1e-9); a copy that
    has not is certified on its own.  Compared on the device: nothing but the odd voxels' rows comes to the host"""
    import torch
    c = N.CASES[name]
    sch, K, y, _, _, _ = N.problem(c['signals'])
    m = N.N_SMALL
    dev = xd.device
    s_t = torch.from_numpy(N.scale_of(y)).to(dev)
    base = torch.arange(m, device=dev)
    odd = []
    for p in range(1, n // m):
        idx = (base + p) % m
        blk = slice(p * m, (p + 1) * m)
        dx = (xd[blk] - xd[:m][idx]).abs().amax(dim=(1, 2))
        dmap = (est_t[blk] - est_t[:m][idx]).abs().amax(dim=1)
        b = ~(dx <= 1e-12 * s_t[idx]) | ~(dmap <= 1e-9)
        if bool(b.any()):
            odd.append(torch.nonzero(b).flatten() + p * m)
    if not odd:
        return [], 0
    rows = torch.cat(odd)
    r = rows.cpu().numpy()
    cert = N.noddi_certificates_per_voxel(K, sch, N._htable()['htable'], yb[r].astype(np.float64), db[r], xd[rows].cpu().numpy(), c['lam'][0], c['lam'][1],
                                          exvivo=c['exvivo'])
    bad = N.kkt_failures(cert)
    mine = N.noddi_maps(xd[rows][:, 2].cpu().numpy(), K, c['exvivo'])
    bad |= ~(np.abs(est_t[rows].cpu().numpy() - mine) <= 1e-12 * np.abs(mine) + 1e-300).all(axis=1)
    return ([('copies that differ from their first copy and miss the certificate', int(bad.sum()), 'of', len(r), int(r[bad][0]))] if bad.any() else []), len(r)


@pytest.mark.parametrize('name', list(N.CASES))
def test_noddi_route_on_hard_voxels(name, amx_env):
    import torch
    from amico_amd import _capi, get_context
    c = N.CASES[name]
    amx_env(**N.case_env(name))
    src = c['signals'] or name
    sch, K, y, d, _, _ = N.problem(src)
    n, big = c['n'], c['n'] != N.N_SMALL
    dev = torch.device('cuda', 0)
    yb, db = (N.tiled(y.astype(np.float32), n), N.tiled(d, n)) if big else (y, d)
    ctx = get_context()
    lut = _capi.upload_noddi(ctx, K, N._htable()['htable'], sch.dwi_idx, is_exvivo=c['exvivo'])
    found, paths = [], []

    def fit(yy, dd, first):
        out = _capi.noddi_fit_device(ctx, lut, torch.from_numpy(np.array(yy)).to(dev), torch.from_numpy(np.array(dd)).to(dev), c['lam'][0], c['lam'][1],
                                     4 if c['exvivo'] else 3, rmse=c['errors'], nrmse=c['errors'], return_x=True)
        ctx.sync()
        paths.append(ctx.last_path())
        ss = _stats(ctx, c, len(yy), found, first)
        _route(c, len(yy), paths[-1], ss)
        return [out[k] for k in (0, 1, 2, 4)]
    clean = fit(yb, db, True)
    if not big and 'k_noddi_gemm' in paths[0]:
        found += _check_table(ctx, name, n)
    dirty = fit(*N.with_bad_voxels(yb, db), False)
    lut.close()
    found += _same_bits(clean, dirty, n)
    del dirty
    est_t, rmse_t, nrmse_t, xd = clean
    m = N.N_SMALL
    est, rmse, nrmse, x = [None if t is None else t[:m].cpu().numpy() for t in (est_t, rmse_t, nrmse_t, xd)]
    found += _check_first_copy(name, paths[0], x, est, rmse, nrmse) if big else _check(name, name, paths[0], x, est, rmse, nrmse)
    if big:
        more, odd = _check_copies(name, xd, est_t, yb, db, n)
        print('NODDIHARD %-14s %d voxels: %d copies differ from their first copy by more than 1e-12 s and were certified on their own' % (name, n, odd))
        found += more
    assert not found, (name, found)


def _check_first_copy(name, path, x, est, rmse, nrmse):
    """the first 3 000 voxels of a large call are the small case's problem at the large call's lambdas and dictionary"""
    c, src = N.CASES[name], N.CASES[N.CASES[name]['signals']]
    assert (c['lam'], c['exvivo'], c['grid'], N.case_protocol(name)) == (src['lam'], src['exvivo'], src['grid'], N.case_protocol(c['signals']))
    found = _check(c['signals'], name, path, x, est, rmse, nrmse)
    return [('first copy',) + (f if isinstance(f, tuple) else (f,)) for f in found]
