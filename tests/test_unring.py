"""Gibbs unringing by local sub-voxel shifts (doUnring; include/amico_amd.h "(f0+++)"): what can be checked without a device --
the numpy oracle's own properties and its effect on a truncated phantom, the independent restatement by circulant and DFT matrices against
it, the launch arithmetic (amx_unring_route) and the configuration rules of Evaluation.set_data.

The constant.  Two float64 evaluations of the definition differ by rounding alone; measured as max|delta| / (n_max eps64 max|slice|) between
the oracle (FFT) and the restatement (matrices) over every slice of every input of tests/test_gpu_unring.py (unring_np.CASES, seeds
fixed), the worst ratio was C_U = 0.2314 (the 8 x 8 slices; 0.07 to 0.17 on the larger ones).  The GPU tests allow four times that.  On the
same inputs no pixel of the restatement needed the near-tie clause (unring_np.compare): the noise keeps the minima apart."""
import os
import re

import numpy as np
import pytest

import unring_np as U
from test_mppca import one_b0_image, stop_at_the_plan, Reached

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
C_U = 0.2314


def noisy_slice(n_a, n_b, seed=3):
    return U.noisy_image((n_a, n_b, 1, 1), seed)[:, :, 0, 0].astype(np.float64)


# ------------------------------------------------------------------ the oracle's own properties
def test_a_zero_slice_stays_zero():
    assert not U.unring_slice(np.zeros((12, 9))).any()


@pytest.mark.parametrize('shape', [(8, 8), (9, 17), (32, 15)])
def test_a_constant_slice_stays_constant(shape):
    out = U.unring_slice(np.full(shape, 750.0))
    assert np.abs(out - 750.0).max() <= 16 * max(shape) * U.EPS * 750.0


@pytest.mark.parametrize('shape', [(8, 8), (9, 16), (16, 9), (31, 33), (64, 64)])
def test_the_two_filters_sum_to_one(shape):
    gx, gy = U.filter_x(*shape), U.filter_x(*shape[::-1]).T
    assert np.abs(gx + gy - 1.0).max() <= 4 * U.EPS and gx.min() >= 0.0 and gx.max() <= 1.0
    if shape[0] % 2 == 0 and shape[1] % 2 == 0:
        assert gx[shape[0] // 2, shape[1] // 2] == 0.5


def test_a_cyclic_translation_commutes():
    I = noisy_slice(24, 17)
    ref = U.unring_slice(I)
    for da, db in [(1, 0), (0, 5), (7, 11)]:
        out = U.unring_slice(np.roll(np.roll(I, da, axis=0), db, axis=1))
        d = np.abs(out - np.roll(np.roll(ref, da, axis=0), db, axis=1))
        assert d.max() <= 4 * 24 * U.EPS * np.abs(I).max()


def test_transposing_the_slice_transposes_the_result():
    # the operator with the axes swapped: U along b of the part that rings along b, U along a of the other
    img = U.noisy_image((20, 13, 2, 1), 5)
    a = U.unring64(img, (0, 1))
    b = U.unring64(np.ascontiguousarray(img.transpose(1, 0, 2, 3)), (1, 0))
    assert np.array_equal(a, b.transpose(1, 0, 2, 3))
    # ... and the plain transpose agrees to rounding: Iy = I - Ix is not Gy's own product, bit for bit
    I = img[:, :, 0, 0].astype(np.float64)
    d = np.abs(U.unring_slice(I.T).T - U.unring_slice(I))
    assert np.median(d) <= 4 * 20 * U.EPS * np.abs(I).max()


def test_a_nan_passes_its_slice_through_and_no_other():
    img = U.noisy_image((10, 12, 2, 3), 7)
    clean = U.unring(img)
    bad = img.copy()
    bad[3, 4, 1, 2] = np.nan
    bad[0, 0, 0, 1] = np.inf
    res = U.unring(bad)
    assert res['slices'] == 6 and res['passed_through'] == 2 and clean['passed_through'] == 0
    assert np.array_equal(res['image'][:, :, 1, 2], bad[:, :, 1, 2], equal_nan=True)
    assert np.array_equal(res['image'][:, :, 0, 1], bad[:, :, 0, 1])
    keep = np.ones((2, 3), dtype=bool)
    keep[1, 2] = keep[0, 1] = False
    assert np.array_equal(res['image'][:, :, keep], clean['image'][:, :, keep])
    assert not np.array_equal(clean['image'], img)


def test_three_dimensional_input_and_every_axis_pair():
    img = U.noisy_image((9, 10, 11, 1), 11)[..., 0]
    for axes in [(0, 1), (0, 2), (1, 2), (2, 0)]:
        res = U.unring(img, axes)
        assert res['image'].shape == img.shape and res['image'].dtype == np.float32
        c = 3 - sum(axes)
        assert res['slices'] == img.shape[c]
        sl = [slice(None)] * 3
        sl[c] = 4
        I = img[tuple(sl)] if axes[0] < axes[1] else img[tuple(sl)].T
        got = res['image'][tuple(sl)] if axes[0] < axes[1] else res['image'][tuple(sl)].T
        assert np.array_equal(got, U.unring_slice(I).astype(np.float32))


# ------------------------------------------------------------------ the effect
@pytest.mark.parametrize('n', [64, 97])
def test_ringing_beside_edges_falls_threefold(n):
    low, truth = U.phantom(n, n)
    band = U.edge_band(truth, 6)
    out = U.unring_slice(low)
    before = np.sqrt(np.mean((low - truth)[band] ** 2))
    after = np.sqrt(np.mean((out - truth)[band] ** 2))
    print(f'n = {n}: rms error over {band.sum()} flat pixels within 6 of an edge {before:.2f} -> {after:.2f} (factor {before / after:.2f})')
    assert band.sum() > 1000 and before > 10.0 and after * 3.0 <= before


# ------------------------------------------------------------------ the restatement against the oracle, on every input of the GPU tests
@pytest.mark.parametrize('case', U.CASES)
def test_restatement_against_the_oracle(case):
    img = U.case_image(case)
    ref = U.unring64(img)
    got = U.unring64(img, one_slice=U.restated_slice)
    w, _ = U.slices_of(img)
    r, _ = U.slices_of(ref)
    g, _ = U.slices_of(got)
    ratio = max(np.abs(r[:, :, z, s] - g[:, :, z, s]).max() / (max(case[:2]) * U.EPS * np.abs(w[:, :, z, s]).max())
                for z in range(case[2]) for s in range(case[3]))
    worst, ties, out = U.compare(got, img, (0, 1), C_U, ref)
    print(f'{case}: max|delta| / (n_max eps64 max|slice|) = {ratio:.4f}; near-tie pixels {ties}, outside {out}')
    assert ratio <= C_U * 1.0001          # C_U is the recorded worst of these ratios
    assert ties == 0 and out == 0


def test_shift_table_is_the_fourier_shift():
    for n in (8, 9, 16, 31):
        f = np.random.default_rng(n).standard_normal((3, n))
        g = U.shifted_lines(f)
        d = U.shift_table(n)
        for j in (1, 7, 20, 21, 40):
            assert np.abs(f @ U.circulant(d[j]).T - g[j]).max() <= 8 * n * U.EPS * np.abs(f).max()
    assert U.SHIFTS[0] == 0.0 and U.SHIFTS[20] == 0.5 and U.SHIFTS[21] == -0.025 and U.SHIFTS[40] == -0.5 and len(U.SHIFTS) == 41


# ------------------------------------------------------------------ the launch arithmetic
def test_route_every_extent_pair():
    from amico_amd import _capi
    cap = None
    for n_a in range(8, 257):
        for n_b in range(8, 257):
            rt = _capi.unring_route(n_a, n_b)
            cap = rt['cap']
            assert rt['tile'] == (16, 16, 4)
            assert rt['lds_dft'] <= 160 * 1024 and rt['lds_shift'] <= 160 * 1024, (n_a, n_b)
            pa, pb = rt['pad']
            assert n_a <= pa < n_a + 16 and n_b <= pb < n_b + 16 and pa % 16 == 0 and pb % 16 == 0
            # a workgroup holds two tiles of max(pad) x (16 lines + 1) doubles, the shift kernel a row of the table more
            assert rt['lds_dft'] == 2 * max(pa, pb) * 17 * 8 and rt['lds_shift'] == rt['lds_dft'] + 8 * max(n_a, n_b)
            ga, gb = rt['groups']
            assert ga * 16 >= n_b > (ga - 1) * 16 and gb * 16 >= n_a > (gb - 1) * 16
            assert rt['slice_bytes'] >= 5 * 8 * n_a * n_b and rt['table_bytes'] >= 8 * (2 * n_a * n_a + 2 * n_b * n_b + 41 * (n_a + n_b))
            assert rt['chunk'] >= 1
            need = rt['table_bytes'] + rt['chunk'] * rt['slice_bytes']
            assert need + need // 8 + 256 <= cap, (n_a, n_b)               # as the grow-only workspace rounds it up
    assert cap == 128 << 20
    for bad in [(7, 8), (8, 7), (257, 8), (8, 257), (0, 0), (-1, 64)]:
        with pytest.raises(ValueError, match='8 to 256'):
            _capi.unring_route(*bad)


def test_bindings_are_declared():
    from amico_amd import _capi, unring
    hdr = open(os.path.join(ROOT, 'include', 'amico_amd.h')).read()
    declared = set(re.findall(r'\b(amx_[a-z0-9_]+)\s*\(', hdr))
    L = _capi.lib()
    for n in ['amx_prep_unring_device', 'amx_unring_route']:
        assert n in declared and n in _capi.SYMBOLS and getattr(L, n).argtypes is not None, n
    assert callable(_capi.Prep.unring_device) and callable(_capi.unring_route)
    assert callable(unring.unring_device) and callable(unring.unring)
    assert unring.is_unring('Kellner') and unring.is_unring(True) and not unring.is_unring(False) and not unring.is_unring(None)
    assert (unring.MIN_EXTENT, unring.MAX_EXTENT) == (U.MIN_EXTENT, U.MAX_EXTENT) == (8, 256)


# ------------------------------------------------------------------ configuration rules: all act in set_data, before anything is uploaded
@pytest.mark.parametrize('value', ['kellner', 'KELLNER', 'Kellner', True])
def test_set_data_accepts_the_key(value, monkeypatch):
    import amico_amd
    stop_at_the_plan(monkeypatch)
    img, sch = one_b0_image((8, 9, 3))
    ae = amico_amd.Evaluation()
    assert ae.get_config('doUnring') is False and ae.get_config('doSaveUnringedDWI') is False and ae.get_config('unring_axes') == (0, 1)
    ae.set_config('doUnring', value)
    with pytest.raises(Reached):
        ae.set_data(img, sch)


@pytest.mark.parametrize('value', ['gibbs', 'yes', 1, 2.0])
def test_any_other_value_is_a_value_error(value, monkeypatch):
    import amico_amd
    stop_at_the_plan(monkeypatch)
    img, sch = one_b0_image((8, 9, 3))
    ae = amico_amd.Evaluation()
    ae.set_config('doUnring', value)
    with pytest.raises(ValueError, match='doUnring'):
        ae.set_data(img, sch)


@pytest.mark.parametrize('axes', [(0, 0), (0, 3), (1,), (0, 1, 2), 'xy', (0.0, 1.0), (True, 2), None])
def test_bad_axes_are_a_value_error(axes, monkeypatch):
    import amico_amd
    stop_at_the_plan(monkeypatch)
    img, sch = one_b0_image((8, 9, 3))
    ae = amico_amd.Evaluation()
    ae.set_config('doUnring', True)
    ae.set_config('unring_axes', axes)
    with pytest.raises(ValueError, match='unring_axes'):
        ae.set_data(img, sch)


def test_extents_outside_the_limit_are_refused_at_set_data(monkeypatch):
    import amico_amd
    stop_at_the_plan(monkeypatch)
    ae = amico_amd.Evaluation()
    ae.set_config('doUnring', True)
    img, sch = one_b0_image((7, 9, 12))
    with pytest.raises(RuntimeError, match='doUnring.*8 to 256.*7 x 9'):
        ae.set_data(img, sch)
    ae.set_config('unring_axes', (1, 2))              # the short axis is the slices'
    with pytest.raises(Reached):
        ae.set_data(img, sch)
    img, sch = one_b0_image((8, 257, 1))
    ae.set_config('unring_axes', [0, 1])
    with pytest.raises(RuntimeError, match='doUnring.*8 to 256.*8 x 257'):
        ae.set_data(img, sch)
    ae.set_config('doUnring', False)                  # without the key nothing is asked of the extents
    with pytest.raises(Reached):
        ae.set_data(img, sch)


def test_check_functions():
    from amico_amd import unring
    assert unring.check_axes([1, 2]) == (1, 2) and unring.check_axes((np.int64(2), 0)) == (2, 0)
    unring.check_extents((8, 256, 3), (0, 1))
    with pytest.raises(RuntimeError, match='8 to 256'):
        unring.check_extents((8, 256, 3), (0, 2))
