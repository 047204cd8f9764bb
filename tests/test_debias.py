"""Rician debias (doDebiasSignal / DWI-SNR, core.py:201-206 -> preproc.py:23-36), the parts that need no GPU: the fixture's
premise, the errors `set_data` raises before a context exists, and the C ABI's declarations."""
import os
import re

import numpy as np
import pytest

import debias_np as D
from conftest import ROOT, load_npz
from amico_amd import synthetic as S


def fixture_rows():
    f = load_npz('debias_fixture.npz')
    sel = f['mask'] != 0
    rows = f['img'][sel]
    lvl = f['region'][sel]
    sigma = D.sigma_of(rows, f['b0_idx'], 1.0) / f['snr_levels'][lvl]
    return f, rows, lvl, sigma


def test_fixture_is_self_consistent():
    """the exact minimiser is one (zero at or below the floor, a root of mu(e) = S above it) and the reference's output never has a
    lower objective: the premise of the GPU test against the reference"""
    f, rows, lvl, sigma = fixture_rows()
    assert set(np.unique(f['mask'])) == {0, 1, 2} and (rows == 0).any() and len(f['b0_idx']) == 9
    assert np.array_equal(np.argwhere(f['mask'] != 0), f['vox']) and rows.shape == f['exact_E'].shape == f['ref_E'].shape
    fl = D.floor_of(sigma)[:, None]
    below = rows <= fl
    assert below.any() and not f['exact_E'][below].any()
    res = np.abs(D.mu(f['exact_E'], sigma[:, None]) - rows)
    assert (res[~below] <= 1e-14 * rows[~below]).all()
    F_exact, F_ref = D.objective(f['exact_E'], rows, sigma), D.objective(f['ref_E'], rows, sigma)
    assert np.array_equal(F_ref, f['ref_F'])
    assert (F_exact <= F_ref).all()
    b0 = (sigma * f['snr_levels'][lvl])[:, None]
    gap = np.array([np.max(np.abs(f['ref_E'] - f['exact_E'])[lvl == k] / b0[lvl == k]) for k in range(len(f['snr_levels']))])
    assert np.array_equal(gap, f['gap']) and (gap > 1e-5).all()          # the reference stops well short of its minimum


def test_mu_helper_branches_agree_and_bound():
    e = np.geomspace(1e-3, 1e7, 400)
    m = D.mu(e, 1.0)
    assert (m > e).all() and (np.diff(m) > 0).all() and D.mu(0.0, 2.0) == 2.0 * D.SQRT_HALF_PI
    x_edge = np.sqrt(2.0 * D.X_ASYMPTOTIC)
    # across the switch: 2e-12 from the step in e itself + 3 / (128 x^3) = 2.4e-14, the first term the series drops
    assert abs(D.mu(x_edge * (1 + 1e-12), 1.0) / D.mu(x_edge * (1 - 1e-12), 1.0) - 1.0) < 2e-12 + 1e-13
    assert np.isfinite(D.mu(1e5, 1.0)) and abs(D.mu(1e5, 1.0) - (1e5 + 0.5e-5)) < 1e-9


def test_set_data_refuses_debias_without_snr_or_b0():
    """both before a context is created (this test runs without a GPU); the first with the reference's message (core.py:205)"""
    import amico_amd
    sch = S.make_scheme(seed=0)
    img = np.ones((2, 2, 2, sch.nS), dtype=np.float32)
    ae = amico_amd.Evaluation()
    ae.set_config('doDebiasSignal', True)
    with pytest.raises(RuntimeError, match='Set noise variance for debiasing'):
        ae.set_data(img, sch)
    raw = np.asarray(sch.raw)
    nob0 = S.SimpleScheme(raw[np.asarray(sch.dwi_idx)])
    assert nob0.b0_count == 0
    ae = amico_amd.Evaluation()
    ae.set_config('doDebiasSignal', True)
    ae.set_config('DWI-SNR', 30.0)
    ae.set_config('doNormalizeSignal', False)
    with pytest.raises(RuntimeError, match='No b0 volume to estimate the noise level'):
        ae.set_data(np.ones((2, 2, 2, nob0.nS), dtype=np.float32), nob0)


def test_debias_symbols_declared_and_bound():
    from amico_amd import _capi
    hdr = open(os.path.join(ROOT, 'include', 'amico_amd.h')).read()
    declared = set(re.findall(r'\b(amx_[a-z0-9_]+)\s*\(', hdr))
    names = ['amx_debias_rows', 'amx_debias_rows_f32', 'amx_debias_rows_device', 'amx_debias_rows_device_f32',
             'amx_prep_set_debias_mask', 'amx_prep_debias', 'amx_prep_debias_device', 'amx_debias_last_unconverged']
    L = _capi.lib()
    for n in names:
        assert n in declared and n in _capi.SYMBOLS and getattr(L, n).argtypes is not None, n
    assert 'preproc.py:23-36' in hdr and 'core.py:201-206' in hdr


def load_generator():
    import importlib.util
    spec = importlib.util.spec_from_file_location('gen_debias_cheb', os.path.join(ROOT, 'tools', 'gen_debias_cheb.py'))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def kernel_tables():
    src = open(os.path.join(ROOT, 'amico_amd', 'csrc', 'amx_debias.hip')).read()
    out = {}
    for name in ('kA0', 'kA1', 'kB0', 'kB1'):
        body = re.search(r'__constant__ double ' + name + r'\[\d+\] = \{([^}]*)\}', src).group(1)
        out[name] = [float(v) for v in body.replace('\n', ' ').split(',') if v.strip()]
    return src, out


def test_chebyshev_tables_of_the_kernel_meet_scipy():
    """the tables amx_debias.hip holds, evaluated in float64 by the kernel's recurrence, against scipy's ive (numpy + scipy only)"""
    from scipy.special import ive
    gen = load_generator()
    _, t = kernel_tables()
    assert [len(t[k]) for k in ('kA0', 'kA1', 'kB0', 'kB1')] == [30, 30, 25, 25]
    z = np.concatenate([np.linspace(1e-6, 8.0, 3000), np.geomspace(8.0, 1e8, 3000)])
    i0, i1 = gen.ive_f64(z, t)
    assert np.max(np.abs(i0 / ive(0, z) - 1.0)) < 3e-15 and np.max(np.abs(i1 / ive(1, z) - 1.0)) < 3e-15


def test_chebyshev_tables_in_the_kernel_are_the_generated_ones():
    """amx_debias.hip carries, verbatim, the text tools/gen_debias_cheb.py prints.  The generator needs mpmath (50-digit Bessel
    functions; a dependency of sympy, which torch requires) and a few seconds: the one test of the CPU suite that does."""
    gen = load_generator()
    src, t = kernel_tables()
    assert t == gen.tables()
    assert gen.source_text() in src


def test_set_data_refuses_more_b0_volumes_than_the_kernel_sums():
    """before a context is created, next to the other debias checks (the kernel follows numpy's summation order up to its block size)"""
    import amico_amd
    tab = np.zeros((140, 4))
    tab[130:, 0], tab[130:, 3] = 1.0, 1000.0
    sch = S.SimpleScheme(tab)
    assert sch.b0_count == 130
    ae = amico_amd.Evaluation()
    ae.set_config('doDebiasSignal', True)
    ae.set_config('DWI-SNR', 30.0)
    with pytest.raises(RuntimeError, match='more than 128 b0 volumes'):
        ae.set_data(np.ones((2, 2, 2, 140), dtype=np.float32), sch)
