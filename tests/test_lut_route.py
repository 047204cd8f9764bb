"""The arithmetic that picks the LUT resampling GEMM's kernel (amx_lut_route, csrc/amx_lut_route.hpp), walked without a GPU over
K = 1 .. 300 reduction indices x N = 1 .. 512 volumes x plain / fused input: where each of the three kernels is reached, what LDS it
asks for, and the boundaries the dispatch has always had."""
import pytest

TILE_KS = {88, 90, 92, 180, 182, 184, 252, 254, 256}       # even K at most 4 floats below 4 * {23, 46, 64}


@pytest.fixture(scope='module')
def walk():
    from amico_amd import _capi
    return {(k, n, f): _capi.lut_route(k, n, f) for k in range(1, 301) for n in range(1, 513) for f in (0, 1)}


def test_every_shape_has_a_route_within_its_lds(walk):
    for (k, n, fused), rt in walk.items():
        assert rt['route'] in ('tile', 'lds', 'generic', 'refused'), (k, n, fused, rt)
        assert rt['kh2'] == (23 if k <= 92 else 46 if k <= 184 else 64), (k, n, fused, rt)
        if rt['route'] == 'tile':
            assert not fused and k in TILE_KS and 0 < rt['lds'] <= 160 * 1024, (k, n, rt)
            # operator zone (whole KB + 2 KB of zeros) + four row tiles of whole KB
            assert rt['lds'] == -(-n * k * 4 // 1024) * 1024 + 2048 + 4 * (-(-32 * k * 4 // 1024) * 1024), (k, n, rt)
        elif rt['route'] == 'lds':
            assert k <= 256 and 0 < rt['lds'] <= 80 * 1024, (k, n, fused, rt)
            assert rt['lds'] == -(-n // 32) * 32 * (4 * rt['kh2'] + 2) * 4, (k, n, fused, rt)
        else:
            assert rt['lds'] == 0, (k, n, fused, rt)
        if fused:
            assert rt['route'] in ('lds', 'refused'), (k, n, rt)       # a fused call is never generic (nor tile)
        else:
            assert rt['route'] != 'refused', (k, n, rt)                # no plain call is refused
        # what is not tile is lds exactly while K <= 256 and the padded operator fits 80 KB
        if rt['route'] != 'tile':
            fits = k <= 256 and -(-n // 32) * 32 * (4 * rt['kh2'] + 2) * 4 <= 80 * 1024
            assert (rt['route'] == 'lds') == fits, (k, n, fused, rt)


def _ranges(walk, k):
    """-> {route: (first N, last N)} of the plain call at this K, and a check that each route's N are one run"""
    out = {}
    for n in range(1, 513):
        r = walk[(k, n, 0)]['route']
        lo, hi = out.get(r, (n, n - 1))
        assert hi == n - 1, (k, n, r)
        out[r] = (lo, n)
    return out


def test_boundaries_of_todays_arithmetic(walk):
    assert _ranges(walk, 182) == {'tile': (1, 92), 'lds': (93, 96), 'generic': (97, 512)}
    assert _ranges(walk, 256) == {'tile': (1, 30), 'lds': (31, 64), 'generic': (65, 512)}
    assert _ranges(walk, 90) == {'tile': (1, 312), 'generic': (313, 512)}
    assert _ranges(walk, 257) == {'generic': (1, 512)}
    # NODDI's shape (two shells of lmax 12, 90 volumes) stays on the tile kernel
    assert walk[(182, 90, 0)] == {'route': 'tile', 'kh2': 46, 'lds': 161792}


def test_bad_sizes():
    from amico_amd import _capi
    for k, n in ((0, 1), (1, 0), (-3, 5)):
        with pytest.raises(ValueError):
            _capi.lut_route(k, n)
