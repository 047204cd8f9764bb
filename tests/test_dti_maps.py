"""Tensor maps (eigenvalues, FA, MD, AD, RD): the numpy restatement of dipy's route (tests/dti_maps_np.py) pinned on tensors
whose answers are known in closed form, the scenes of the GPU tests (tests/test_gpu_dti_maps.py) checked for what those tests
assume of them, and the host-side rules of the new switch.  No GPU is needed here."""
import numpy as np
import pytest

import amico_amd.synthetic as S
import dti_maps_np as T


def rotation(seed):
    q, _ = np.linalg.qr(np.random.default_rng(seed).normal(size=(3, 3)))
    return q


def tensor_signal(evals, q, bvals, bvecs, s0=1.0):
    """S0 exp(-b g^T D g), D = q diag(evals) q^T"""
    D = (q * np.asarray(evals, dtype=float)) @ q.T
    return s0 * np.exp(-bvals * np.einsum('ij,jk,ik->i', bvecs, D, bvecs))


# name: (eigenvalues, rotation)
CLOSED_FORM = {
    'stick': ((1.7e-3, 0.0, 0.0), rotation(1)),
    'prolate': ((1.7e-3, 0.3e-3, 0.3e-3), rotation(2)),
    'oblate': ((1.2e-3, 1.2e-3, 0.2e-3), rotation(3)),
    'ball': ((0.9e-3, 0.9e-3, 0.9e-3), np.eye(3)),
    'general': ((1.5e-3, 0.7e-3, 0.2e-3), rotation(4)),
}


def exact_fa(e):
    e1, e2, e3 = e
    return np.sqrt(0.5 * ((e1 - e2) ** 2 + (e2 - e3) ** 2 + (e3 - e1) ** 2) / (e1 * e1 + e2 * e2 + e3 * e3))


def closed_form_rows(bvals, bvecs):
    """one voxel per tensor of CLOSED_FORM, in its order -> (y [5, nS], eigenvalues [5, 3])"""
    y = np.stack([tensor_signal(e, q, bvals, bvecs, s0=1.0 + 0.25 * i) for i, (e, q) in enumerate(CLOSED_FORM.values())])
    return y, np.array([e for e, _ in CLOSED_FORM.values()])


def check_closed_form(got, evals_true, min_d, rtol):
    """eigenvalues to rtol of the largest one; FA, MD, AD, RD against the formulas on the exactly known clipped eigenvalues"""
    want = np.maximum(evals_true, min_d)
    scale = want[:, :1]
    assert (np.abs(got['evals'] - want) / scale).max() < rtol
    fa = np.array([exact_fa(e) for e in want])
    assert np.abs(got['scalars'][:, 0] - fa).max() < 1e-8
    assert (np.abs(got['scalars'][:, 1] - want.mean(axis=1)) / scale[:, 0]).max() < rtol
    assert (np.abs(got['scalars'][:, 2] - want[:, 0]) / scale[:, 0]).max() < rtol
    assert (np.abs(got['scalars'][:, 3] - want[:, 1:].mean(axis=1)) / scale[:, 0]).max() < rtol
    names = list(CLOSED_FORM)
    ball, stick = names.index('ball'), names.index('stick')
    assert got['scalars'][ball, 0] < 1e-8 and abs(got['scalars'][ball, 1] - 0.9e-3) < rtol * 0.9e-3
    # (d, 0, 0): the two zero eigenvalues are clipped to min_diffusivity, so FA is 1 to within min_diffusivity / d
    assert 1.0 - min_d / 1.7e-3 * 2.0 < got['scalars'][stick, 0] <= 1.0
    assert np.array_equal(got['evals'][stick, 1:], [min_d, min_d])


def test_restatement_closed_form_tensors():
    sc = S.make_scheme()
    b, g = T.table(sc)
    y, ev = closed_form_rows(b, g)
    min_d = T.min_diffusivity(T.M.design(b, g))
    cross = 2.0 * np.abs(np.stack([g[:, 0] * g[:, 1], g[:, 0] * g[:, 2], g[:, 1] * g[:, 2]], axis=1))
    assert min_d == 1e-6 / max(1.0, (b[:, None] * g * g).max(), (b[:, None] * cross).max())      # 1e-6 / -min(design matrix)
    got = T.fit_maps(y, b, g, 'OLS')
    check_closed_form(got, ev, min_d, 1e-10)
    # the principal axis where it is defined (stick, prolate, general)
    for i, (name, (e, q)) in enumerate(CLOSED_FORM.items()):
        if e[0] > e[1]:
            assert np.linalg.norm(np.cross(got['directions'][i], q[:, 0])) < 1e-10, name


def test_restatement_degenerate_voxels():
    sc = S.make_scheme()
    b, g = T.table(sc)
    min_d = T.min_diffusivity(T.M.design(b, g))
    y = np.zeros((3, sc.nS))
    y[1] = 0.37                                     # constant
    y[2] = 1e-6                                     # all below min_signal
    for method in ('OLS', 'WLS', 'NLLS'):
        got = T.fit_maps(y, b, g, method)
        assert np.array_equal(got['evals'], np.full((3, 3), min_d)), method
        assert np.array_equal(got['scalars'], np.tile([0.0, min_d, min_d, min_d], (3, 1))), method


def test_scalar_formulas():
    ev = np.array([[3.0, 2.0, 1.0], [2.0, 2.0, 2.0], [1.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
    s = T.scalars(ev)
    assert np.allclose(s[0], [np.sqrt(0.5 * 6.0 / 14.0), 2.0, 3.0, 1.5], rtol=1e-15, atol=0)
    assert np.array_equal(s[1], [0.0, 2.0, 2.0, 2.0])
    assert np.array_equal(s[2], [1.0, 1.0 / 3.0, 1.0, 0.0])
    assert np.array_equal(s[3], [0.0, 0.0, 0.0, 0.0])           # FA = 0 where the denominator is 0


@pytest.mark.parametrize('name', T.SCENES)
def test_scenes_leave_no_voxel_out_of_the_scalar_bounds(htable500, name):
    """what the GPU tests may leave out of the scalar bounds (voxels the clip has taken over) is nothing at all on their signals;
    and no sample is clipped by min_signal, so the amplitude test's scaled min_signal clips none either"""
    b, g, y = T.scene_signals(name, htable500)
    assert y.shape[0] == T.N_VOX and y.min() > T.M.MIN_POSITIVE_SIGNAL
    assert np.array_equal(y, y.astype(np.float32).astype(np.float64))
    for method in ('OLS', 'WLS', 'NLLS'):
        ref = T.scene_reference(name, method, htable500)
        assert T.held(ref).all(), (name, method)
        fa = ref['scalars'][:, 0]
        assert np.isfinite(ref['scalars']).all() and (fa >= 0).all() and (fa <= 1).all()
        assert (np.diff(ref['evals'], axis=1) <= 0).all() and (ref['evals'] >= T.min_diffusivity(T.M.design(b, g))).all()


def test_tensor_maps_with_directional_average_is_refused_before_a_context_is_made(monkeypatch):
    import amico_amd
    from amico_amd import models

    def no_context(*a, **k):
        raise AssertionError('a context was asked for')
    monkeypatch.setattr(models, 'get_context', no_context)
    monkeypatch.setattr(models, 'get_contexts', no_context)
    ae = amico_amd.Evaluation()
    assert ae.get_config('doSaveTensorMaps') is False
    ae.set_config('doSaveTensorMaps', True)
    ae.set_config('doDirectionalAverage', True)
    with pytest.raises(ValueError, match='doSaveTensorMaps'):
        ae.fit()


def test_bindings_are_declared():
    from amico_amd import _capi, dti
    assert [name for name, _ in _capi.Dti.OUTPUTS] == ['directions', 'evals', 'scalars']
    assert {'amx_dti_fit', 'amx_dti_fit_device', 'amx_dti_fit_device_f32'} <= set(_capi.SYMBOLS)
    assert dti.SCALAR_NAMES == ('FA', 'MD', 'AD', 'RD') and dti.MIN_DIFFUSIVITY_TOL == T.MIN_DIFFUSIVITY_TOL
