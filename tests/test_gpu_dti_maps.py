"""Tensor maps from the direction fit on the GPU (amx_dti_fit*, TensorDirections.fit_maps, doSaveTensorMaps, tensor_maps=True)
against the numpy restatement of dipy's route (tests/dti_maps_np.py, pinned in tests/test_dti_maps.py).

Bounds.  Eigenvalues of a symmetric matrix move by at most ||dD||_F <= 3 max|dd|, so for OLS and WLS they are held to
EV_TOL = 3 x the 1e-10 the project holds WLS parameters to (test_dti_methods.py::test_restatement_vs_golden), relative to the
voxel's largest |tensor entry|.  FA moves by about 2.5 ||de|| / ||e||: held to FA_TOL = 1e-8 absolute; MD, AD, RD to the eigenvalue
bound.  The scalar bounds apply where the largest clipped eigenvalue is >= 1e-3 of the largest |tensor entry| (below that the
clip turns a relative 1e-10 into anything); at most 1e-3 of the voxels may be left out, the share is asserted, and the CPU test
shows that the scenes used here leave out none.  Voxels left out must still be finite with FA in [0, 1].
NLLS is defined to MINPACK's stopping rule only, so it is held as test_nlls_vs_minpack_synthetic holds directions: no farther
from MINPACK run to 1e-15 than MINPACK at dipy's tolerances is -- but no tighter than the direct solves' bounds above, which is
what an exact fit (the 7-volume scheme: both MINPACK runs stop at rounding, 2e-15 apart) would otherwise ask for.
"""
import numpy as np
import pytest

import dti_maps_np as T
from test_dti_maps import CLOSED_FORM, check_closed_form, closed_form_rows

pytestmark = pytest.mark.gpu

EV_TOL = 3e-10
FA_TOL = 1e-8
METHODS = ('OLS', 'WLS', 'NLLS')
COUNTS = (1, 7, 65, T.N_VOX)        # tails of the eight-lanes-per-voxel groups (1, 7), of a 64-voxel tile (65) and of a workgroup's tiles


def _estimator(name, method, **kw):
    from amico_amd import dti
    sc, merge = T.scene(name)
    return dti.TensorDirections.from_scheme(sc, do_merge_b0=merge, fit_method=method, **kw)


def _fit_device(est, y, f32, want=(True, True, True)):
    """the device entry points on rows of either type -> dict like fit_maps (None for an output that was not asked for)"""
    import torch
    dev = torch.device('cuda', torch.cuda.current_device())
    d_y = torch.from_numpy(np.array(y, dtype=np.float32 if f32 else np.float64, order='C')).to(dev)
    n = y.shape[0]
    bufs = [torch.full((n, k), -7.0, dtype=torch.float64, device=dev) if w else None for k, w in zip((3, 3, 4), want)]
    ptr = [None if b is None else b.data_ptr() for b in bufs]
    est.fit_device(d_y.data_ptr(), n, ptr[0], f32=f32, d_evals=ptr[1], d_scalars=ptr[2])
    est.ctx.sync()
    return dict(zip(('directions', 'evals', 'scalars'), (None if b is None else b.cpu().numpy() for b in bufs)))


def _fit(est, y, f32):
    return _fit_device(est, y, True) if f32 else est.fit_maps(y)


def _check(got, ref, method, label, rows=slice(None), assert_share=True):
    """the bounds of the module docstring; every figure is printed before anything is asserted"""
    ev, sc, scale = ref['evals'][rows], ref['scalars'][rows], ref['scale'][rows]
    ev_bound, fa_bound = EV_TOL, FA_TOL
    held = T.held(ref)[rows]
    if method == 'NLLS':
        ev_bound = max(EV_TOL, (np.abs(ref['evals_default'][rows] - ev) / scale[:, None]).max())
        fa_bound = max(FA_TOL, np.abs(ref['scalars_default'][rows][held, 0] - sc[held, 0]).max())
    e_ev = (np.abs(got['evals'] - ev) / scale[:, None]).max()
    e_fa = np.abs(got['scalars'][held, 0] - sc[held, 0]).max() if held.any() else 0.0
    e_md = (np.abs(got['scalars'][held, 1:] - sc[held, 1:]) / scale[held, None]).max() if held.any() else 0.0
    print('%s: %d voxels, eigenvalues %.3g (bound %.3g), FA %.3g (bound %.3g), MD/AD/RD %.3g, left out %d'
          % (label, len(scale), e_ev, ev_bound, e_fa, fa_bound, e_md, int((~held).sum())))
    assert np.isfinite(got['evals']).all() and np.isfinite(got['scalars']).all()
    assert (got['scalars'][:, 0] >= 0).all() and (got['scalars'][:, 0] <= 1).all()
    assert (np.diff(got['evals'], axis=1) <= 0).all()
    if assert_share:
        assert (~held).mean() <= 1e-3
    assert e_ev <= ev_bound
    assert e_fa <= fa_bound and e_md <= ev_bound


# ----------------------------------------------------------------------------- 1. shapes x schemes x row types x methods
@pytest.mark.parametrize('f32', [False, True])
@pytest.mark.parametrize('method', METHODS)
@pytest.mark.parametrize('name', T.SCENES)
def test_maps_vs_restatement(htable500, name, method, f32):
    b, g, y = T.scene_signals(name, htable500)
    ref = T.scene_reference(name, method, htable500)
    est = _estimator(name, method)
    assert est.min_diffusivity == T.min_diffusivity(T.M.design(b, g))
    full = _fit(est, y, f32)
    assert est.last_unconverged() == 0
    assert (full['evals'] >= est.min_diffusivity).all()
    assert np.array_equal(full['scalars'][:, 2], full['evals'][:, 0])                                  # AD = e1
    assert np.array_equal(full['directions'], est.fit(y))                                              # the directions of always
    _check(full, ref, method, '%s %s f32=%s' % (name, method, f32))
    for n in COUNTS[:-1]:
        part = _fit(est, y[:n], f32)
        for key in ('directions', 'evals', 'scalars'):
            # ragged tiles: a voxel's fit does not depend on its tile, so these are the head of the full call, bit for bit ...
            assert np.array_equal(part[key], full[key][:n]), (n, key)
        if method != 'NLLS':
            # ... and held to the bounds on their own (NLLS' bound is a maximum over the voxels of both MINPACK runs: it says
            # nothing about a handful, which the equality above ties to the full call)
            _check(part, ref, method, '%s %s f32=%s n=%d' % (name, method, f32, n), rows=slice(0, n), assert_share=False)


def test_host_call_with_some_outputs(htable500):
    b, g, y = T.scene_signals('std', htable500)
    est = _estimator('std', 'OLS')
    full = est.fit_maps(y[:65])
    for want in (['evals'], ['scalars'], ['directions', 'scalars'], ['directions']):
        got = est._dti.fit(y[:65], est.min_diffusivity, want)
        assert sorted(got) == sorted(want)
        for key in want:
            assert np.array_equal(got[key], full[key])
    assert est.fit_maps(y[:0])['scalars'].shape == (0, 4)
    with pytest.raises(ValueError, match='min_diffusivity'):
        est._dti.fit(y[:5], -1.0)
    with pytest.raises(ValueError, match='min_diffusivity'):
        est._dti.fit(y[:5], float('nan'))


# ----------------------------------------------------------------------------- 2. closed forms
@pytest.mark.parametrize('method', METHODS)
def test_closed_form_tensors(method):
    """signals S0 exp(-b g^T D g) are linear in the parameters after the logarithm: every method gives D back, so the eigenvalues
    and FA are known exactly (stick, prolate, oblate, ball, rotated general tensor: tests/test_dti_maps.py)"""
    b, g = T.table(T.scene('std')[0])
    y, ev = closed_form_rows(b, g)
    est = _estimator('std', method)
    for got in (est.fit_maps(y), _fit_device(est, y, False)):
        check_closed_form(got, ev, est.min_diffusivity, EV_TOL)
        for i, (name, (e, q)) in enumerate(CLOSED_FORM.items()):
            if e[0] > e[1]:
                assert np.linalg.norm(np.cross(got['directions'][i], q[:, 0])) < 1e-10, name
    assert est.last_unconverged() == 0


# ----------------------------------------------------------------------------- 3. degenerate voxels
@pytest.mark.parametrize('f32', [False, True])
@pytest.mark.parametrize('method', METHODS)
def test_degenerate_voxels(htable500, method, f32):
    """the outcomes include/amico_amd.h documents: all-zero / constant / all-below-min_signal voxels give min_diffusivity three times and
    FA = 0; a NaN sample counts as min_signal; a +Inf sample gives NaN maps; the other voxels of the tiles are untouched"""
    b, g, y = T.scene_signals('std', htable500)
    y = y[:192]
    est = _estimator('std', method)
    clean = _fit(est, y, f32)
    bad = y.copy()
    bad[5] = 0.0
    bad[70] = 0.37
    bad[71] = 1e-6
    bad[131, 17] = np.nan
    bad[150, 3] = np.inf
    got = _fit(est, bad, f32)
    md = est.min_diffusivity
    for i in (5, 70, 71):
        assert np.array_equal(got['evals'][i], [md, md, md]), i
        assert np.array_equal(got['scalars'][i], [0.0, md, md, md]), i
        assert np.isfinite(got['directions'][i]).all()
    # the NaN sample: what the voxel gives with min_signal in its place, bit for bit, and so the restatement's answer for that
    as_clipped = y[131:132].copy()
    as_clipped[0, 17] = est.min_signal
    one = _fit(est, as_clipped, f32)
    for key in ('directions', 'evals', 'scalars'):
        assert np.isfinite(got[key][131]).all() and np.array_equal(got[key][131], one[key][0]), key
    if method != 'NLLS':
        ref = T.fit_maps(as_clipped, b, g, method)
        assert (np.abs(one['evals'] - ref['evals']) / ref['scale'][:, None]).max() <= EV_TOL
    # the +Inf sample: not hidden by the clip
    assert np.isnan(got['evals'][150]).all() and np.isnan(got['scalars'][150]).all()
    rest = np.ones(len(y), dtype=bool)
    rest[[5, 70, 71, 131, 150]] = False
    for key in ('directions', 'evals', 'scalars'):
        assert np.array_equal(got[key][rest], clean[key][rest]), key
    # directions: those of amx_dti_directions* on the same rows (of the same type), degenerate voxels included
    assert np.array_equal(got['directions'], _fit_device(est, bad, f32, (True, False, False))['directions'], equal_nan=True)


# ----------------------------------------------------------------------------- 4. amplitudes
@pytest.mark.parametrize('f32', [False, True])
@pytest.mark.parametrize('method', METHODS)
def test_amplitude(htable500, method, f32):
    """a scale only moves ln S0 (min_signal is scaled along, as in test_dti_methods.py::test_amplitude; the scene clips no sample):
    eigenvalues, FA, MD, AD, RD against the reference of the unscaled signals, to the same bounds"""
    b, g, y = T.scene_signals('std', htable500)
    ref = T.scene_reference('std', method, htable500)
    for k in (-10, 14):
        est = _estimator('std', method, min_signal=1e-4 * 2.0 ** k)
        got = _fit(est, y * 2.0 ** k, f32)
        assert est.last_unconverged() == 0
        _check(got, ref, method, 'scale 2^%d %s f32=%s' % (k, method, f32))


# ----------------------------------------------------------------------------- 5. outputs all null
@pytest.mark.parametrize('f32', [False, True])
@pytest.mark.parametrize('method', METHODS)
def test_no_map_outputs_is_the_direction_call(htable500, method, f32):
    import torch
    b, g, y = T.scene_signals('std', htable500)
    est = _estimator('std', method)
    ctx = est.ctx
    dev = torch.device('cuda', torch.cuda.current_device())
    d_y = torch.from_numpy(np.array(y, dtype=np.float32 if f32 else np.float64, order='C')).to(dev)
    n = len(y)
    d_a, d_b = (torch.zeros((n, 3), dtype=torch.float64, device=dev) for _ in range(2))
    path0 = ctx.last_path()
    est._dti.directions_device(d_y.data_ptr(), n, d_a.data_ptr(), f32=f32)
    ctx.sync()
    path_a = ctx.last_path()
    est._dti.fit_device(d_y.data_ptr(), n, est.min_diffusivity, d_b.data_ptr(), None, None, f32=f32)       # amx_dti_fit_device[_f32]
    ctx.sync()
    assert ctx.last_path() == path_a == path0            # (a tensor pass is no model fit: neither call touches the fit's launch list)
    assert torch.equal(d_a, d_b) and torch.isfinite(d_a).all()
    # its checks are the direction call's: the direction buffer is needed then, and refused by the same words
    with pytest.raises(ValueError, match='amx_dti_directions: null buffer'):
        est._dti.fit_device(d_y.data_ptr(), n, est.min_diffusivity, None, None, None, f32=f32)
    # with map outputs: another kernel, the same directions bit for bit, whichever outputs are taken
    for want in ((True, True, True), (True, False, True), (True, True, False)):
        got = _fit_device(est, y, f32, want)
        assert np.array_equal(got['directions'], d_a.cpu().numpy()), want
    full = _fit_device(est, y, f32)
    only = _fit_device(est, y, f32, (False, True, True))
    assert only['directions'] is None and np.array_equal(only['evals'], full['evals']) and np.array_equal(only['scalars'], full['scalars'])


# ----------------------------------------------------------------------------- 6. Evaluation end to end
def _scatter(values, sel):
    vol = np.zeros(sel.shape + (values.shape[1],), dtype=np.float32)
    vol[sel] = values.astype(np.float32)
    return vol


def _volume_scene(htable500, model):
    import amico_amd.synthetic as S
    ht = htable500['htable']
    shape = (11, 9, 6)
    n = int(np.prod(shape))
    if model == 'NODDI':
        sch = S.make_scheme(seed=0)
        K = S.noddi_kernels(sch, htable500['dirs'])
        y, d = S.noddi_signals(n, K, ht, sch, seed=4)
    else:
        sch = S.make_scheme(5, ((1000.0, 60),), seed=3)
        K = S.freewater_kernels(sch, htable500['dirs'])
        y, d = S.freewater_signals(n, K, ht, sch, seed=2, snr=20.0)
    img = np.asfortranarray((y.reshape(shape + (-1,)) * 900.0).astype(np.float32))
    mask = (np.random.default_rng(2).uniform(size=shape) < 0.7).astype(np.uint8)
    return sch, K, ht, img, mask, d.reshape(shape + (3,)).astype(np.float32)


def _evaluate(scene, model, method='OLS', maps=None, directions=None, merge=False):
    import amico_amd
    sch, K, ht, img, mask, _ = scene
    ae = amico_amd.Evaluation()
    ae.set_config('DTI_fit_method', method)
    ae.set_config('doMergeB0', merge)
    if maps is None:
        del ae.CONFIG['doSaveTensorMaps']               # a configuration that has never heard of the key
    else:
        ae.set_config('doSaveTensorMaps', maps)
    ae.set_data(img, sch, mask, directions=directions)
    ae.set_model(model)
    if merge:                                           # (Free-Water only: the dictionary of [one b0] + the DWI volumes)
        cols = np.hstack((sch.b0_idx[0], sch.dwi_idx))
        K = {'model': 'FreeWater', 'D': np.ascontiguousarray(K['D'][..., cols]), 'CSF': np.ascontiguousarray(K['CSF'][..., cols])}
    ae.set_kernels(K, ht)
    res = ae.fit()
    return ae, res


@pytest.mark.parametrize('model,method,merge', [('NODDI', 'OLS', False), ('NODDI', 'WLS', False), ('FreeWater', 'OLS', False),
                                                ('FreeWater', 'NLLS', False), ('FreeWater', 'OLS', True)])
def test_evaluation_end_to_end(htable500, model, method, merge):
    from amico_amd import dti
    scene = _volume_scene(htable500, model)
    sch, K, ht, img, mask, d_true = scene
    sel = mask == 1
    off_a, _ = _evaluate(scene, model, method, maps=None, merge=merge)
    off_b, _ = _evaluate(scene, model, method, maps=False, merge=merge)
    assert sorted(off_a.RESULTS) == sorted(off_b.RESULTS) == ['DIRs', 'MAPs']
    for key in off_a.RESULTS:
        assert off_a.RESULTS[key].tobytes() == off_b.RESULTS[key].tobytes()
    on, res = _evaluate(scene, model, method, maps=True, merge=merge)
    new = ['DTI_MAPs', 'DTI_evals'] + (['DTI_MAPs_corrected', 'DTI_evals_corrected'] if model == 'FreeWater' else [])
    assert sorted(on.RESULTS) == sorted(['DIRs', 'MAPs'] + new)
    for key in ('DIRs', 'MAPs'):                         # the switch moves nothing else
        assert on.RESULTS[key].tobytes() == off_a.RESULTS[key].tobytes()
    est = dti.TensorDirections.from_scheme(sch, do_merge_b0=merge, fit_method=method)
    same = _fit_device(est, on.y, True)                  # the call fit() makes: float32 rows in HBM
    host = est.fit_maps(on.y)
    for key, k, name in (('DTI_MAPs', 4, 'scalars'), ('DTI_evals', 3, 'evals')):
        vol = on.RESULTS[key]
        assert vol.dtype == np.float32 and vol.shape == mask.shape + (k,) and not vol[~sel].any() and vol[sel].all()
        assert np.array_equal(vol, _scatter(same[name], sel))
        assert np.allclose(vol[sel], host[name], rtol=1e-6, atol=0)
    assert np.array_equal(on.RESULTS['DIRs'], _scatter(same['directions'], sel))
    # the tensor pass itself, on these rows, against the restatement
    b, g = T.table(sch, merge)
    if method != 'NLLS':
        ref = T.fit_maps(on.y, b, g, method)
        _check(host, ref, method, 'Evaluation %s %s' % (model, method), assert_share=model == 'NODDI')
    # caller-supplied directions: the tensor pass runs for the maps only
    given, _ = _evaluate(scene, model, method, maps=True, directions=d_true, merge=merge)
    assert np.array_equal(given.RESULTS['DIRs'][sel], d_true[sel]) and not given.RESULTS['DIRs'][~sel].any()
    for key in new[:2]:
        assert given.RESULTS[key].tobytes() == on.RESULTS[key].tobytes()
    if model == 'FreeWater':
        assert 'y_corrected' in res
        yc = res['y_corrected']
        again = est.fit_maps(yc)                         # the same float64 rows, through the host call
        for key, name in (('DTI_MAPs_corrected', 'scalars'), ('DTI_evals_corrected', 'evals')):
            vol = on.RESULTS[key]
            assert vol.dtype == np.float32 and not vol[~sel].any() and np.isfinite(vol).all()
            assert np.array_equal(vol, _scatter(again[name], sel))


def test_tensor_maps_refusals(htable500):
    import amico_amd
    scene = _volume_scene(htable500, 'NODDI')
    sch, K, ht, img, mask, _ = scene
    for method in ('RT', 'RESTORE'):
        ae = amico_amd.Evaluation()
        ae.set_config('DTI_fit_method', method)
        ae.set_config('doSaveTensorMaps', True)
        ae.set_data(img, sch, mask, directions=scene[5])            # (given directions: without the switch no tensor fit would run)
        ae.set_model('NODDI')
        ae.set_kernels(K, ht)
        with pytest.raises(NotImplementedError, match='sigma'):
            ae.fit()


def test_free_water_correction_raises_fa(htable500):
    """two compartments, a zeppelin of the dictionary and free water, no noise: the tensor of the mixture is rounder than the
    tissue's; the fit on the corrected rows gets the tissue's anisotropy back"""
    import amico_amd
    import amico_amd.synthetic as S
    ht = htable500['htable']
    sch = S.make_scheme(5, ((1000.0, 60),), seed=3)
    K = S.freewater_kernels(sch, htable500['dirs'])
    shape = (8, 6, 5)
    n = int(np.prod(shape))
    rng = np.random.default_rng(7)
    lut = rng.integers(0, 500, n)
    k = rng.integers(0, 6, n)                            # d_perp 0.1 .. 0.6e-3 beside d_par 1e-3: anisotropic tissue
    f = rng.uniform(0.2, 0.5, n)[:, None]
    y = (1.0 - f) * K['D'][k, lut].astype(np.float64) + f * K['CSF'][0].astype(np.float64)[None, :]
    img = (y.reshape(shape + (-1,)) * 700.0).astype(np.float32)
    ae = amico_amd.Evaluation()
    ae.set_config('doSaveTensorMaps', True)
    ae.set_data(img, sch, None, directions=htable500['dirs'][lut].reshape(shape + (3,)))
    ae.set_model('FreeWater')
    ae.set_kernels(K, ht)
    ae.fit()
    fa, fa_c = ae.RESULTS['DTI_MAPs'][..., 0], ae.RESULTS['DTI_MAPs_corrected'][..., 0]
    print('FA of the mixture %.3f .. %.3f, corrected %.3f .. %.3f, smallest gain %.3f' % (fa.min(), fa.max(), fa_c.min(), fa_c.max(), (fa_c - fa).min()))
    assert (fa_c > fa).all()
    assert 'DWI_corrected' not in ae.RESULTS             # doSaveCorrectedDWI was not needed, and is not implied


# ----------------------------------------------------------------------------- 7. pipelines
@pytest.mark.parametrize('model', ['NODDI', 'FreeWater'])
def test_pipeline_tensor_maps(htable500, model):
    import torch
    from amico_amd import pipeline
    scene = _volume_scene(htable500, model)
    sch, K, ht, img, mask, _ = scene
    flat = np.lib.stride_tricks.as_strided(img, shape=(img.size,), strides=(4,))
    cls = pipeline.NoddiVolumePipeline if model == 'NODDI' else pipeline.FreeWaterVolumePipeline
    ae, _ = _evaluate(scene, model, maps=True)
    pl = cls(sch, img, mask, K, ht, tensor_maps=True)
    maps, dirs = pl.run(torch.from_numpy(flat.copy()).to('cuda:0'))
    path_on = pl.ctx.last_path()
    assert np.array_equal(maps.cpu().numpy(), ae.RESULTS['MAPs']) and np.array_equal(dirs.cpu().numpy(), ae.RESULTS['DIRs'])
    assert np.array_equal(pl.dti_maps.cpu().numpy(), ae.RESULTS['DTI_MAPs'])
    assert np.array_equal(pl.dti_evals.cpu().numpy(), ae.RESULTS['DTI_evals'])
    if model == 'FreeWater':
        assert np.array_equal(pl.dti_maps_corrected.cpu().numpy(), ae.RESULTS['DTI_MAPs_corrected'])
        assert np.array_equal(pl.dti_evals_corrected.cpu().numpy(), ae.RESULTS['DTI_evals_corrected'])
        assert pl.corrected is None
    # the default: nothing of it is made, and the chain is the one fused=False has always been, volume for volume
    for fused in (True, False):
        plain = cls(sch, img, mask, K, ht, fused=fused)
        m0, d0 = plain.run(torch.from_numpy(flat.copy()).to('cuda:0'))
        assert plain.dti_maps is None and plain.dti_evals is None
        if model == 'FreeWater':
            assert plain.dti_maps_corrected is None and plain.x_iso is None
        if not fused:
            assert plain.ctx.last_path() == path_on          # the model fit's launch list
            assert np.array_equal(m0.cpu().numpy(), maps.cpu().numpy()) and np.array_equal(d0.cpu().numpy(), dirs.cpu().numpy())
