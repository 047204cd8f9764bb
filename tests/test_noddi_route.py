"""The arithmetic that routes a NODDI fit (amx_noddi_route, csrc/amx_noddi_route.hpp), walked without a GPU.

tests/golden/noddi_routes.json holds Context.last_path() of fits recorded on the commit before the route existed (six dictionary shapes,
three lambda settings, call sizes on both sides of every threshold): the function names exactly those launches in that order.

Two sizes key the thresholds, and the walk pins which is which:
* call_vox (the whole call) keys the seeded chain (22 528), both occ2 builds (65 536), the third LASSO certificate pass (600 000, protocols
  of 96 .. 128 stage-2 rows) and the rescue pass (2 000 000; ex vivo 500 000): a batch takes what its whole call takes;
* n (this batch) keys the small-call builds of the stage-1 / stage-3 left-over kernels (150 000 / 600 000), the seed chunk and the
  wavefronts of the seed solvers: they size work to the voxels at hand and change no result."""
import json
import os

import pytest

LDS_MAX = 160 * 1024
HOST_BATCH = 393216
# (threshold, what flips there): keyed on call_vox ...
CALL_KEYS = ('seeds', 'seed_occ2', 'seed2_occ2', 'third', 'rescue', 'seeds2', 'gcert', 'gcert2', 'wide', 'repair', 'seed2_max_atoms', 'min_items',
             'left2_second_half', 'left2_count')
N_ATOMS = (17, 64, 145, 160, 161, 192, 193, 256)
SIZES = (22527, 22528, 65535, 65536, 149999, 150000, 499999, 500000, 599999, 600000, 1999999, 2000000)
SEED_KERNELS = ('k_nnls_seed', 'k_lasso_seed', 'k_nnls_gcert', 'k_lasso_gcert', 'k_noddi_gemm', 'k_s2_prep')


def _fixture():
    with open(os.path.join(os.path.dirname(__file__), 'golden', 'noddi_routes.json')) as fh:
        return json.load(fh)


def _route(c, **kw):
    from amico_amd import _capi
    a = dict(nS=c['nS'], n_wm=c['n_wm'], n_dwi=c['n_dwi'], ndirs=c['ndirs'], is_exvivo=c['exvivo'], n_vox=c['n'], call_vox=c['call_vox'],
             lambda1=c['lam1'], lambda2=c['lam2'])
    a.update(kw)
    return _capi.noddi_route(**a)


def test_route_names_the_recorded_launches():
    cases = _fixture()
    assert len(cases) == 184
    for c in cases:
        assert 'error' not in c
        assert _route(c)['path'] == c['path'], (c['shape'], c['lambdas'], c['n'], c['call_vox'])


def _global_tile(nS, n_atoms):
    """the predicate restated from the kernels' layout: the LDS builds hold <= 256 rows and <= 192 atoms and need the float32 tile (odd
    leading dimension, padded by a wavefront's 3 atoms per lane) beside two wavefronts of the LASSO stage's Gram solver with 32 passive
    atoms and the screening table, or one wavefront of its re-run kernel with 64"""
    if nS > 256 or n_atoms > 192:
        return True
    tile = (((nS * (n_atoms | 1) + 64 * 3 + 3) & ~3) * 4 + 15) & ~15
    wave = lambda maxp: (2 if nS <= 128 else 4) * 64 * 8 + (maxp + 1) * (maxp + 2) * 8 + 32
    return tile + 2 * wave(32) + 16 + 12 * 192 * 4 > LDS_MAX or tile + wave(64) + 16 > LDS_MAX


def _shape(nS, n_atoms):
    n_b0 = min(9, nS - 1)
    return dict(nS=nS, n_wm=n_atoms - 1, n_dwi=nS - n_b0, ndirs=500, is_exvivo=0)


@pytest.mark.parametrize('n_atoms', N_ATOMS)
def test_walk_every_protocol_length(n_atoms):
    from amico_amd import _capi
    for nS in range(7, 513):
        sh = _shape(nS, n_atoms)
        per_call = {}
        for call in SIZES:
            for n in sorted({call, min(call, HOST_BATCH)}):
                rt = _capi.noddi_route(n_vox=n, call_vox=call, **sh)
                tag = (nS, n_atoms, n, call)
                # every launch fits a CU's LDS
                assert rt['n_launch'] == len(rt['launches']) >= 3, tag
                for name, waves, lds, lds_list in rt['launches']:
                    assert waves >= 1 and lds <= LDS_MAX and lds_list <= LDS_MAX, (tag, name, waves, lds, lds_list)
                # no basis: no seed or certificate kernel
                if n_atoms > 160:
                    assert not rt['seeds'] and not any(k in rt['path'] for k in SEED_KERNELS), (tag, rt['path'])
                # the global tile: all three stages or none
                assert [rt[s] == 'global' for s in ('s1', 's2', 's3')] == [rt['global']] * 3, (tag, rt['s1'], rt['s2'], rt['s3'])
                assert rt['global'] == _global_tile(nS, n_atoms), tag
                assert (not rt['third'] or rt['wide']) and (not rt['wide'] or rt['gcert2']), tag
                assert (rt['seed2_max_atoms'] == 26) == rt['third'] and rt['seed2_max_atoms'] in (20, 26), tag
                # what the whole call keys is the same for a batch and for its call; what n keys follows n
                if call in per_call:
                    assert {k: rt[k] for k in CALL_KEYS} == per_call[call], tag
                per_call[call] = {k: rt[k] for k in CALL_KEYS}
                alone = _capi.noddi_route(n_vox=n, call_vox=n, **sh)
                if rt['seeds'] == alone['seeds']:
                    assert (rt['s1'], rt['s3'], rt['seed_chunk']) == (alone['s1'], alone['s3'], alone['seed_chunk']), tag


THRESHOLDS = (22528, 65536, 150000, 500000, 600000, 2000000)
# both sides of every threshold, and a grid of sizes between them: a flip anywhere but at a threshold shows too
PROBES = sorted({t + d for t in THRESHOLDS for d in (-1, 0, 1)} | set(range(20000, 2100000, 7919)))


def _flips(key, **kw):
    """[(a, b)]: neighbours of PROBES between which rt[key] changes, walking n == call_vox"""
    from amico_amd import _capi
    vals = [_capi.noddi_route(n_vox=v, **kw)[key] for v in PROBES]
    return [(PROBES[i - 1], PROBES[i]) for i in range(1, len(PROBES)) if vals[i] != vals[i - 1]]


def _at(*ts):
    return [(t - 1, t) for t in ts]


@pytest.mark.parametrize('lambdas', [(0.5, 1e-3), (0.0, 1e-3), (0.5, 1e-6)])
def test_every_threshold_flips_exactly_at_its_number(lambdas):
    from amico_amd import _capi
    lam = dict(lambda1=lambdas[0], lambda2=lambdas[1])
    default = dict(nS=99, n_wm=144, n_dwi=90, ndirs=500, is_exvivo=0, **lam)
    v105 = dict(nS=105, n_wm=144, n_dwi=100, ndirs=500, is_exvivo=0, **lam)
    assert _flips('seeds', **default) == _at(22528)
    assert _flips('seed_occ2', **default) == _at(65536) and _flips('seed2_occ2', **default) == _at(65536)
    assert _flips('s1', **default) == _at(22528, 150000)          # (unseeded -> small-call build -> 12 wavefronts on the fp64 tile)
    assert _flips('s3', **default) == _at(22528, 600000)
    assert _flips('rescue', **default) == _at(2000000)
    assert _flips('rescue', **dict(default, is_exvivo=1)) == _at(500000)
    seeded2 = lambdas == (0.5, 1e-3)      # (lambda1 = 0 goes straight to k_noddi_lasso_big, lambda2 < 1e-5 to the QR stage: no LASSO seeds)
    assert _flips('third', **default) == [] and _flips('third', **v105) == (_at(600000) if seeded2 else [])
    assert _flips('seeds2', **default) == (_at(22528) if seeded2 else [])
    assert _capi.noddi_route(n_vox=100000, **default)['s2'] == {(0.5, 1e-3): 'gram_left', (0.0, 1e-3): 'big_all', (0.5, 1e-6): 'qr'}[lambdas]
    # the small-call builds follow the batch, the rest the call
    batch = _capi.noddi_route(n_vox=149999, call_vox=2000000, **default)
    assert batch['s1'] == 'small' and batch['s3'] == 'small' and batch['rescue'] and batch['seed_occ2']
    batch = _capi.noddi_route(n_vox=HOST_BATCH, call_vox=2000000, **v105)
    assert batch['s1'] == 'f64_12' and batch['s3'] == 'small' and batch['third'] == seeded2 and batch['rescue']
    batch = _capi.noddi_route(n_vox=22527, call_vox=22528, **default)
    assert batch['seeds'] and batch['s1'] == 'small'


def test_a_wrong_argument_raises():
    from amico_amd import _capi
    for bad in (dict(nS=0), dict(nS=513), dict(n_wm=0), dict(n_wm=256), dict(n_dwi=100), dict(n_vox=0), dict(lambda1=-1.0), dict(ndirs=0)):
        with pytest.raises(ValueError):
            _capi.noddi_route(**dict(dict(nS=99, n_wm=144, n_dwi=90, ndirs=500, is_exvivo=0, n_vox=1000), **bad))
