"""The FreeWater, SANDI and CylinderZeppelinBall launchers follow the route: for every recorded case of tests/golden/small_routes.json, at
2 048 voxels on the synthetic dictionaries of tests/small_route_np.py, Context.last_path() of the fit, _capi.small_route of the same shape
and the path recorded before the route existed are the same string, and the fit returns the recorded status (two shapes are refused)."""
import json
import os

import numpy as np
import pytest

import small_route_np as R

pytestmark = pytest.mark.gpu


def _cases():
    with open(os.path.join(os.path.dirname(__file__), 'golden', 'small_routes.json')) as fh:
        return json.load(fh)


@pytest.mark.parametrize('model', sorted(R.MODELS), ids=[R.MODELS[m] for m in sorted(R.MODELS)])
def test_fit_launches_what_the_route_names(model):
    import torch
    from amico_amd import _capi
    cases = [c for c in _cases() if c['model'] == model]
    assert [{k: c[k] for k in R.CASES[0]} for c in cases] == [c for c in R.CASES if c['model'] == model]
    dev = torch.device('cuda', 0)
    ctx = _capi.Context(-1)
    try:
        for c in cases:
            upload, A = R.dictionary(c['model'], c['n_atoms'], c['nS'], c['mouse'])
            y, d = R.signals(A, c['n'])
            lut = upload(ctx)
            try:
                status, error = R.fit(ctx, lut, c, torch.from_numpy(y.astype(np.float32) if c['f32'] else y).to(dev), torch.from_numpy(d).to(dev))
                rt = _capi.small_route(c['model'], c['nS'], c['n_atoms'], c['ndirs'], c['n'], c['lam1'], c['lam2'], c['flags'], c['f32'])
                assert ctx.last_path() == rt['path'] == c['path'], c
                assert (status, error) == (rt['status'], rt['error']) == (c['status'], c['error']), c
            finally:
                lut.close()
    finally:
        ctx.close()
