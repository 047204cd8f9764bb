"""The LDS of the wide LASSO certificate passes (k_lasso_gcert<18, wide>, <24, wide, 18>), walked without a GPU.

They hold the packed lower triangle of the orientation's white-matter Gram block -- n_wm (n_wm + 1) / 2 doubles -- beside what the first
pass holds, at one workgroup per CU.  A seeded LASSO stage has at most 144 white-matter atoms, so the sum never exceeds a CU's LDS
and the route has no second path: there is no fall-back field to flip."""
import pytest

LDS_MAX = 160 * 1024                      # kLdsPerCU
N_ATOMS = (17, 64, 145, 160, 161, 192, 193, 256)      # what tests/test_noddi_route.py walks
SIZES = (22527, 22528, 65535, 65536, 149999, 150000, 499999, 500000, 599999, 600000, 1999999, 2000000)
WIDE_NOTES = ('k_lasso_gcert<18,wide>', 'k_lasso_gcert<24,wide,18>')


def _first_pass_lds(n_wm):
    """S rows (stride 14) + ticket, column scales and G[.][iso] (even counts), S in MFMA operand order (9 tiles x 3 K-steps x 64),
    a [64][16] block for each of four wavefronts; doubles"""
    return (n_wm * 14 + 2 + 2 * ((n_wm + 1) & ~1) + 9 * 3 * 64 + 4 * 64 * 16) * 8


def _triangle(n_wm):
    return n_wm * (n_wm + 1) // 2 * 8


def test_default_shape_reports_the_wide_lds():
    from amico_amd import _capi
    rt = _capi.noddi_route(nS=99, n_wm=144, n_dwi=90, ndirs=500, is_exvivo=0, n_vox=1000000)
    assert rt['wide'] and not rt['third']
    assert _first_pass_lds(144) == 65040 and _triangle(144) == 83520
    assert rt['gcert2_wide_lds'] == 65040 + 83520
    lds = {name: b for name, _, b, _ in rt['launches']}
    assert lds['k_lasso_gcert<11>'] == 65040                     # the first pass keeps its own size: two workgroups per CU
    assert lds['k_lasso_gcert<18,wide>'] == 65040 + 83520


def test_the_largest_seeded_dictionary_leaves_room():
    """144 atoms is the most a seeded LASSO stage holds; the formula alone would cross a CU's LDS between 155 and 156 atoms"""
    first_over = next(n for n in range(1, 257) if _first_pass_lds(n) + _triangle(n) > LDS_MAX)
    assert first_over > 144 + 1, first_over
    assert _first_pass_lds(first_over - 1) + _triangle(first_over - 1) <= LDS_MAX


@pytest.mark.parametrize('exvivo', [0, 1])
@pytest.mark.parametrize('n_atoms', N_ATOMS)
def test_wide_lds_fits_wherever_the_route_turns_the_pass_on(n_atoms, exvivo):
    from amico_amd import _capi
    n_wm = n_atoms - 1 - exvivo
    seen = set()
    for nS in range(7, 513):
        n_b0 = min(9, nS - 1)
        for call in SIZES:
            rt = _capi.noddi_route(nS=nS, n_wm=n_wm, n_dwi=nS - n_b0, ndirs=500, is_exvivo=exvivo, n_vox=call)
            tag = (nS, n_atoms, exvivo, call)
            seen.add(rt['wide'])
            if not rt['wide']:
                assert rt['gcert2_wide_lds'] == 0 and not any(w in rt['path'] for w in WIDE_NOTES), tag
                continue
            assert n_wm <= 144, tag
            assert rt['gcert2_wide_lds'] == _first_pass_lds(n_wm) + _triangle(n_wm) <= LDS_MAX, (tag, rt['gcert2_wide_lds'])
            lds = {name: b for name, _, b, _ in rt['launches']}
            assert lds[WIDE_NOTES[0]] == rt['gcert2_wide_lds'] and lds['k_lasso_gcert<11>'] == _first_pass_lds(n_wm), tag
            assert (WIDE_NOTES[1] in lds) == rt['third'], tag
            if rt['third']:
                assert lds[WIDE_NOTES[1]] == rt['gcert2_wide_lds'], tag
    assert seen == ({True, False} if n_wm <= 144 else {False}), (n_atoms, seen)      # (small calls run no seeded chain)
