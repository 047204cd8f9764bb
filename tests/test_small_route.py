"""The arithmetic that routes a FreeWater, SANDI or CylinderZeppelinBall fit (amx_small_route, csrc/amx_small_route.hpp), walked without a GPU.

tests/golden/small_routes.json holds Context.last_path() and the status of 62 fits of 2 048 voxels recorded on the commit before the route
existed, on both sides of every branch (the cases: tests/small_route_np.py): the function names exactly those launches in that order, and
the two refusals.

The walk compares every route with _expect(), which restates each predicate from the kernels' own limits: what a lane holds (16 atoms), what
reads float32 signals (every wavefront-per-voxel kernel's load_rows, FreeWater's matrix-core projection and fused kernel up to 4 x 24 K-steps
= 96 volumes, k_sandi_project, every CylinderZeppelinBall kernel, k_enet_big), where the ridge allows the warm start (1e-5), a Gram-space
lane solver (1e-9), CylinderZeppelinBall's Gram form (1e-6) and its complementary form (1e-2).  All 511 protocol lengths are walked on the
product path (switches_mask 0); the fifteen other masks on the lengths beside every threshold (NS_EDGES) -- the route is piecewise constant in
nS, and the full product (19 M routes) would take minutes."""
import ctypes as C
import json
import os

import pytest

LDS_MAX = 160 * 1024
F_RMSE, F_CORRECTED = 1, 8
N_ATOMS = (3, 11, 12, 13, 15, 16, 17, 26, 32, 33, 64, 65, 256)
LAM2 = (0.0, 9.9e-10, 1e-9, 9.9e-7, 1e-6, 9.9e-6, 1e-5, 9.9e-3, 1e-2, 4.0)
NS_EDGES = (2, 5, 6, 7, 63, 64, 65, 96, 97, 100, 101, 128, 129, 160, 161, 227, 228, 256, 257, 511, 512)
WAVE, NO_REFILL, ATOM_SPACE, NO_FUSE = 1, 2, 4, 8
LANE_NOTE = 'lane-per-voxel solver (k_freewater_lane / k_sandi_lane)'
LANE_KERNELS = ('lane', 'refill', 'fused', 'k_sandi_rows', 'k_fw_project', 'k_czb_project')
BIG = {2: 'k_enet_big<FreeWater> (65 .. 256 atoms)', 3: 'k_enet_big<SANDI> (65 .. 256 atoms)', 4: 'k_enet_big<CylinderZeppelinBall> (65 .. 256 atoms)'}
PAIR_TILE = 'dictionary tile does not fit the 160 KB LDS of a CU (nS x n_atoms too large)'
LONG_RIDGE = 'amx_sandi_fit: protocols of more than 128 volumes need lambda2 >= 1e-9 (Gram-space solver)'


def _fixture():
    with open(os.path.join(os.path.dirname(__file__), 'golden', 'small_routes.json')) as fh:
        return json.load(fh)


def test_route_names_the_recorded_launches():
    from amico_amd import _capi
    cases = _fixture()
    assert len(cases) == 62 and sum(c['status'] != 0 for c in cases) == 2
    for c in cases:
        rt = _capi.small_route(c['model'], c['nS'], c['n_atoms'], c['ndirs'], c['n'], c['lam1'], c['lam2'], c['flags'], c['f32'])
        assert (rt['path'], rt['status'], rt['error']) == (c['path'], c['status'], c['error']), c


# ------------------------------------------------------------------------------------------------ the predicates, restated
def _pair_lds(elem, nS, n_atoms, NR, waves, maxp, gram, extra=0):
    """dynamic LDS of a wavefront-per-voxel kernel: the tile (odd leading dimension, padded by a wavefront's one atom per lane), then per
    wavefront NR signal rows per lane, the solver's block (Gram: two packed triangles; QR: R and the ridge rows) and four mask words"""
    tile = (((nS * (n_atoms | 1) + 64 + 3) & ~3) * elem + 15) & ~15
    block = (maxp + 1) * (maxp + 2) if gram else 2 * (maxp + 1) ** 2
    return tile + waves * (NR * 64 * 8 + block * 8 + 32) + 16 + extra


def _pair(elem, nS, n_atoms, NR, full, maxp, gram, extra=0):
    """(refused, wavefronts, LDS, LDS of the re-run pass): `full` wavefronts halved until the main pass fits; the re-run pass holds 64 atoms"""
    w = full
    while w > 1 and _pair_lds(elem, nS, n_atoms, NR, w, maxp, gram, extra) > LDS_MAX:
        w >>= 1
    lds, lds_list = _pair_lds(elem, nS, n_atoms, NR, w, maxp, gram, extra), _pair_lds(elem, nS, n_atoms, NR, 1, 64, gram)
    return lds > LDS_MAX or lds_list > LDS_MAX, w, lds, lds_list


def _expect(model, nS, na, lam2, flags, f32, mask):
    """-> (path, error, family, widen, tables, in_order, chunk is the refill chunk)"""
    wave = bool(mask & WAVE)
    lane = na <= 16 and lam2 >= 1e-9 and not wave
    warm = lam2 >= 1e-5
    errors = bool(flags & 3)
    rows8 = 2 if nS <= 128 else (4 if nS <= 256 else 8)
    if model == 3 and nS > 128 and lam2 < 1e-9:
        return '', LONG_RIDGE, 'none', False, 'none', False, False
    if na > 64:
        return BIG[model], '', 'enet_big', False, 'none', model == 3, False
    if model == 3 and nS > 128:
        n = 12 if na <= 12 else (15 if na <= 15 else 16)
        return ('k_sandi_project<%s> -> %s' % ('float' if f32 else 'double', 'k_sandi_gram_lane<%d>' % n if lane else 'k_sandi_gram_wave'), '',
                'sandi_long_lane' if lane else 'sandi_long_wave', False, 'sandi_long', True, False)
    if model == 4:
        if na <= 32 and lam2 >= 1e-2 and not errors and not wave and nS <= 160:
            return 'k_czb_project<%d> -> k_czb_lane' % (25 if nS <= 100 else 40), '', 'czb_fast', False, 'czb', False, False
        if lam2 < 1e-6:
            refused = _pair(4, nS, na, rows8, 4, 32, False)[0]
            return 'k_czb_qr<%d>' % rows8, PAIR_TILE if refused else '', 'czb_qr', False, 'none', False, False
        refused = _pair(4, nS, na, rows8, 8, 32, True, (na * 64 + 33 * 34 + 33) * 8 + 16)[0]
        return 'k_czb<%d>' % rows8, PAIR_TILE if refused else '', 'czb_gram', False, 'none', False, False
    if not lane:
        refused = _pair(4, nS, na, rows8, 8, 16, False)[0] if model == 2 else _pair(8, nS, na, 1 if nS <= 64 else 2, 8, 16, False)[0]
        return ('k_freewater (wavefront per voxel)' if model == 2 else 'k_sandi (wavefront per voxel)', PAIR_TILE if refused else '', 'wave', False,
                'none', False, False)
    if model == 3:
        if nS == 6 and na == 15 and warm and not mask & ATOM_SPACE:
            return 'k_sandi_rows<6,15>', '', 'sandi_rows', f32, 'sandi', True, False
        return LANE_NOTE, '', 'lane', f32, 'none', False, False
    # FreeWater: k_fw_project's LDS at 12 atoms, beside the 12 x 64 block per wavefront the gate counts, within half a CU's
    if warm and not mask & NO_REFILL and na <= 12 and not errors and not flags & F_CORRECTED and (12 * nS + 144 + 4 * (16 * 65 + 12 * 64 + 32)) * 8 + 16 <= LDS_MAX // 2:
        n = 11 if na <= 11 else 12
        if 64 <= nS <= 96 and not mask & NO_FUSE:
            return 'k_freewater_fused<%d>' % n, '', 'fw_fused', False, 'fw', False, True
        return ('k_fw_project_mfma' if nS <= 96 else 'k_fw_project') + ' -> k_freewater_refill', '', 'fw_refill', f32 and nS > 96, 'fw', False, True
    return LANE_NOTE, '', 'lane', f32, 'none', False, False


def _walk(model, lengths, masks):
    from amico_amd import _capi
    route, out, buf = _capi.lib().amx_small_route, (C.c_int64 * len(_capi.SMALL_ROUTE_WORDS))(), C.create_string_buffer(1024)
    W = {k: i for i, k in enumerate(_capi.SMALL_ROUTE_WORDS)}
    ndirs, n = (1 if model == 3 else 500), 2048
    extra = F_CORRECTED if model == 2 else 2          # (SANDI, CylinderZeppelinBall: AMX_F_NRMSE, the other error map)
    for nS in lengths:
        for na in N_ATOMS:
            for lam2 in LAM2:
                for flags in (0, F_RMSE, extra):
                    for f32 in (0, 1):
                        for mask in masks:
                            tag = (model, nS, na, lam2, flags, f32, mask)
                            assert route(model, nS, na, ndirs, n, 0.0, lam2, flags, f32, mask, buf, 1024, out) == 0, tag
                            path, _, error = buf.value.decode().partition('\n')
                            want = _expect(model, nS, na, lam2, flags, f32, mask)
                            got = (path, error, _capi.SMALL_FAMILIES[out[W['family']]], bool(out[W['widen']]), _capi.SMALL_TABLES[out[W['tables']]],
                                   bool(out[W['in_order']]), out[W['chunk']] == 512 and model == 2)
                            assert got == want, (tag, got, want)
                            # every LDS size fits a CU, or the fit is refused; a refusal is a status and a text
                            assert (out[W['lds']] <= LDS_MAX and out[W['lds_list']] <= LDS_MAX) or out[W['refusal']], tag
                            assert bool(out[W['refusal']]) == bool(error), tag
                            # (the old "float32 signals need the matrix-core projection" state: float32, not widened, on k_fw_project)
                            assert not (f32 and not got[3] and 'k_fw_project ->' in path), tag
                            if mask & WAVE:
                                assert not any(k in path for k in LANE_KERNELS), (tag, path)
                            if na > 64 and not error:
                                assert path == BIG[model], (tag, path)
                            if mask & NO_REFILL:
                                assert 'refill' not in path and 'fused' not in path, (tag, path)
                            if mask & NO_FUSE:
                                assert 'fused' not in path, (tag, path)
                            if mask & ATOM_SPACE:
                                assert 'k_sandi_rows' not in path, (tag, path)
                            # tables are named exactly when the route's kernels read them
                            assert (got[4] == 'fw') == ('refill' in path or 'fused' in path), tag
                            assert (got[4] == 'sandi') == ('k_sandi_rows' in path) and (got[4] == 'sandi_long') == ('k_sandi_project' in path), tag
                            assert (got[4] == 'czb') == ('k_czb_lane' in path) == (out[W['blocks_chunk']] == 2048), tag


@pytest.mark.parametrize('model', (2, 3, 4))
def test_walk_every_protocol_length(model):
    _walk(model, range(2, 513), (0,))


@pytest.mark.parametrize('model', (2, 3, 4))
def test_walk_every_switch(model):
    _walk(model, NS_EDGES, range(1, 16))


def test_a_switch_removes_exactly_its_kernel():
    """... and a switch of another model, or of a kernel the shape does not take, changes nothing"""
    from amico_amd import _capi
    for model, ndirs in ((2, 500), (3, 1), (4, 500)):
        for nS in NS_EDGES:
            for na in N_ATOMS:
                for lam2 in LAM2:
                    base = _capi.small_route(model, nS, na, ndirs, 2048, 0.0, lam2)
                    for bit, kernels in ((NO_REFILL, ('refill', 'fused')), (NO_FUSE, ('fused',)), (ATOM_SPACE, ('k_sandi_rows',))):
                        rt = _capi.small_route(model, nS, na, ndirs, 2048, 0.0, lam2, switches_mask=bit)
                        if any(k in base['path'] for k in kernels):
                            assert not any(k in rt['path'] for k in kernels), (model, nS, na, lam2, bit)
                        else:
                            assert rt == base, (model, nS, na, lam2, bit)


def _flips(key, values, call):
    """[(a, b)]: neighbours of `values` between which call(v)[key] changes"""
    got = [call(v)[key] for v in values]
    return [(values[i - 1], values[i]) for i in range(1, len(values)) if got[i] != got[i - 1]]


def _at(*ts):
    return [(t - 1, t) for t in ts]


def test_every_threshold_flips_exactly_at_its_number():
    from amico_amd import _capi
    R = _capi.small_route
    NS = list(range(2, 513))
    fw = lambda **kw: (lambda nS: R(2, nS, 11, 500, 2048, **kw))
    assert _flips('path', NS, fw()) == _at(64, 97, 228)                       # refill (mfma) | fused | refill | lane
    assert _flips('family', NS, fw()) == _at(64, 97, 228)
    assert _flips('mfma', NS, fw(switches_mask=NO_FUSE)) == _at(97)           # k_fw_project_mfma | k_fw_project (a lane route has no projection)
    assert _flips('widen', NS, fw(f32=True)) == _at(97)                       # float32 in place up to 96 volumes, widened beyond (refill and lane)
    assert _flips('widen', NS, fw()) == []
    assert _flips('NR', NS, lambda nS: R(2, nS, 17, 500, 2048)) == _at(129, 257)
    assert _flips('NR', NS, lambda nS: R(4, nS, 26, 500, 2048)) == _at(129, 257)
    assert _flips('NR', NS, lambda nS: R(4, nS, 26, 500, 2048, lambda2=0.0)) == _at(129, 257)
    assert _flips('path', NS, lambda nS: R(3, nS, 17, 1, 2048)) == _at(129) and _flips('NR', NS[:127], lambda nS: R(3, nS, 17, 1, 2048)) == _at(65)
    assert _flips('path', NS, lambda nS: R(3, nS, 15, 1, 2048)) == _at(6, 7, 129)
    assert _flips('path', NS, lambda nS: R(4, nS, 26, 500, 2048, lambda2=4.0)) == _at(101, 161, 257)      # project<25> | <40> | k_czb<4> | <8>
    assert _flips('nSp', NS[:159], lambda nS: R(4, nS, 26, 500, 2048, lambda2=4.0)) == _at(101)
    lam = sorted(set(LAM2) | {float('1e-%d' % k) for k in range(12)})
    near = lambda t: [v for v in lam if v < t][-1]
    paths = lambda model, na, nS, ndirs: [(a, b) for a, b in _flips('path', lam, lambda l: R(model, nS, na, ndirs, 2048, lambda2=l))]
    assert paths(2, 11, 65, 500) == [(near(1e-9), 1e-9), (near(1e-5), 1e-5)]                             # wave | lane | fused
    assert paths(3, 15, 6, 1) == [(near(1e-9), 1e-9), (near(1e-5), 1e-5)]                                # wave | lane | rows
    assert paths(4, 26, 100, 500) == [(near(1e-6), 1e-6), (near(1e-2), 1e-2)]                            # qr | gram | fast
    assert _flips('status', lam, lambda l: R(3, 129, 15, 1, 2048, lambda2=l)) == [(near(1e-9), 1e-9)]    # refused | long
    atoms = list(range(1, 257))
    assert _flips('family', atoms, lambda na: R(2, 300, na, 500, 2048)) == _at(17, 65)                   # lane | wave | enet_big
    assert _flips('family', atoms, lambda na: R(4, 100, na, 500, 2048, lambda2=4.0)) == _at(33, 65)      # fast | gram | enet_big
    assert _flips('N', atoms[:16], lambda na: R(2, 300, na, 500, 2048)) == _at(12, 13)                   # k_freewater_lane<11 | 12 | 16>
    assert _flips('N', atoms[:16], lambda na: R(3, 129, na, 1, 2048)) == _at(13, 16)                     # k_sandi_gram_lane<12 | 15 | 16>


def test_the_refill_chunk():
    from amico_amd import _capi
    chunk = lambda n, **kw: _capi.small_route(2, 65, 11, 500, n, **kw)['chunk']
    for n in (1, 2048, 786432, 786432 + 1535):
        assert chunk(n) == 512, n
    assert chunk(786432 + 1536) == 513
    for n in (1000000, 2000000, 3145727):
        assert chunk(n) == n // 1536, n
    for n in (3145728, 4000000, 2 ** 29 - 1):
        assert chunk(n) == 2048, n
    # every other route buckets by kChunk; SANDI has nothing to bucket
    assert chunk(4000000, flags=F_RMSE) == 256 and _capi.small_route(4, 100, 26, 500, 4000000)['chunk'] == 256
    assert _capi.small_route(3, 6, 15, 1, 4000000)['chunk'] == 0


def test_a_wrong_argument_raises():
    from amico_amd import _capi
    good = dict(model=2, nS=65, n_atoms=11, ndirs=500, n_vox=2048)
    for bad in (dict(model=1), dict(model=5), dict(nS=0), dict(nS=513), dict(n_atoms=0), dict(n_atoms=257), dict(ndirs=0), dict(model=3, ndirs=2),
                dict(n_vox=0), dict(n_vox=2 ** 29), dict(lambda1=-1.0), dict(lambda2=-1.0), dict(lambda2=float('nan')), dict(switches_mask=16)):
        with pytest.raises(ValueError):
            _capi.small_route(**dict(good, **bad))
