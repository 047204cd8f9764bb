"""The NODDI launchers follow the route: for the recorded cases of tests/golden/noddi_routes.json that are small enough to fit here (every
host-buffer call of 22 535 voxels or fewer, and the device call of 150 000 voxels) Context.last_path() of the fit, _capi.noddi_route of
the same shape and sizes, and the path recorded before the route existed are the same string."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _cases():
    with open(os.path.join(os.path.dirname(__file__), 'golden', 'noddi_routes.json')) as fh:
        return [c for c in json.load(fh) if c['n'] <= 22535 or c['n'] == 150000]


def _tiled(a, n):
    return np.ascontiguousarray(np.tile(a, ((n + len(a) - 1) // len(a), 1))[:n])


@pytest.mark.parametrize('shape', sorted({c['shape'] for c in _cases()}))
def test_fit_launches_what_the_route_names(shape):
    import torch
    from amico_amd import _capi, synthetic as S
    cases = [c for c in _cases() if c['shape'] == shape]
    c0 = cases[0]
    dirs = S.fibonacci_hemisphere(c0['ndirs'])
    ht = S.build_htable(dirs)
    sch = S.make_scheme(n_b0=c0['n_b0'], shells=tuple(tuple(s) for s in c0['shells']), seed=0)
    K = S.noddi_kernels(sch, dirs, IC_VFs=np.linspace(0.1, 0.99, c0['n_vf']))
    y0, d0 = S.noddi_signals(256, K, ht, sch, seed=3)
    ctx = _capi.Context(-1)
    lut = _capi.upload_noddi(ctx, K, ht, sch.dwi_idx, is_exvivo=c0['exvivo'])
    n_maps = 4 if c0['exvivo'] else 3
    y, d = _tiled(y0, 22535), _tiled(d0, 22535)
    try:
        for c in cases:
            n = c['n']
            if c['entry'] == 'host':
                ctx.set_call_voxels(c['set_call_voxels'])
                try:
                    _capi.noddi_fit(ctx, lut, y[:n], d[:n], c['lam1'], c['lam2'], n_maps)
                finally:
                    ctx.set_call_voxels(0)
            else:
                yt = torch.from_numpy(_tiled(y0.astype(np.float32), n)).cuda()
                dt = torch.from_numpy(_tiled(d0, n)).cuda()
                _capi.noddi_fit_device(ctx, lut, yt, dt, c['lam1'], c['lam2'], n_maps)
                ctx.sync()
            rt = _capi.noddi_route(c['nS'], c['n_wm'], c['n_dwi'], c['ndirs'], c['exvivo'], n, c['call_vox'], c['lam1'], c['lam2'])
            assert ctx.last_path() == rt['path'] == c['path'], (c['lambdas'], n, c['call_vox'])
    finally:
        lut.close()
        ctx.close()
