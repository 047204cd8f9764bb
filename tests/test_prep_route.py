"""The arithmetic that picks the gather's tile kernel (amx_prep_route, csrc/amx_prep_route.hpp), walked without a GPU: every protocol
of 7 .. 512 volumes gets a route whose LDS fits a workgroup's 160 KB, the two-tile route is kept exactly where its size check lets it
through, and 513 volumes are refused."""
import pytest

LDS_MAX = 160 * 1024

# the four rows of the tile's size: (identity, direct, inplace) -> words of one wavefront's tile on the two-tile route
ROWS = {'identity, planar (direct)': ((1, 1, 1), lambda n: n * 65),
        'identity, interleaved or strided': ((1, 0, 1), lambda n: 64 * (n | 1)),
        'grouped, in place': ((0, 0, 1), lambda n: 64 * (n | 1)),
        'grouped, not in place': ((0, 0, 0), lambda n: 2 * 64 * (n | 1))}


def _lists(nS, identity, n_b0):
    """-> (n_out, n_gidx) of identity groups | the b0 merge"""
    return (nS, nS) if identity else (nS - n_b0 + 1, nS)


@pytest.mark.parametrize('row', list(ROWS))
def test_every_protocol_up_to_512_volumes_has_a_route_that_fits(row):
    from amico_amd import _capi
    (identity, direct, inplace), per_wave = ROWS[row]
    first_long = None
    for nS in range(7, 513):
        for n_b0 in (1, min(9, nS - 1), nS - 1):                       # few b0 volumes, the usual nine, nearly all
            n_out, n_gidx = _lists(nS, identity, n_b0)
            legacy = (2 * per_wave(nS) + n_b0 + n_out + 1 + n_gidx) * 4
            rt = _capi.prep_route(nS, n_out, n_b0, n_gidx, identity, direct, inplace)
            assert rt['route'] in ('tile', 'long') and rt['lds'] <= LDS_MAX, (nS, n_b0, rt)
            # what fits two tiles keeps them, with the LDS it asked for before the long route existed
            assert (rt['route'] == 'tile') == (legacy <= LDS_MAX), (nS, n_b0, rt)
            if rt['route'] == 'tile':
                assert rt['waves'] == 2 and rt['lds'] == legacy and rt['per_wave'] == per_wave(nS)
            else:
                assert rt['waves'] == 1 and rt['per_wave'] >= per_wave(nS) // (1 if inplace or identity else 2)
                if n_b0 == min(9, nS - 1) and first_long is None:
                    first_long = nS
    lo, hi = (150, 170) if not (identity or inplace) else (300, 320)
    assert lo <= first_long <= hi, first_long


@pytest.mark.parametrize('row', list(ROWS))
def test_513_volumes_have_no_route(row):
    from amico_amd import _capi
    (identity, direct, inplace), _ = ROWS[row]
    n_out, n_gidx = _lists(513, identity, 9)
    assert _capi.prep_route(513, n_out, 9, n_gidx, identity, direct, inplace)['route'] == 'refused'
    with pytest.raises(ValueError):
        _capi.prep_route(0, 1, 0, 1, 1, 1, 1)
