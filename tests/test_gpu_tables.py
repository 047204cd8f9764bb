"""Every table the library builds on the device from an uploaded dictionary, fetched with amx_debug_fetch and held to a long-double
reference of the same expression (tables_np.py) within a rounding bound that follows from how the table is summed -- none of the bounds
was measured.  test_tables_np.py checks on the CPU what the bounds rely on (numpy's own float64 inverse meets the inverse bound on
every matrix chosen here; the NODDI shapes take the branches they are named for).

A fit reads these tables but hides their errors: a wrong basis only makes seeds worse and the certificates hand the voxel on.  The one
exception is the screening bound kappa of the NODDI certificates (amx_solver.hpp, NNSolver::certify_seed): with a kappa that is too
small, or a basis that is not orthonormal, a violated Kuhn-Tucker condition is accepted.  test_noddi_upload_tables restates that
inequality on the fetched tables, also for dictionaries of rank below kSeedKD = 12.

Every test prints `TABLES <case> <quantity> <largest value> <bound>` lines (pytest -s)."""
import numpy as np
import pytest

import tables_np as T

pytestmark = pytest.mark.gpu

LD = T.LD
F32, F64 = np.float32, np.float64
N_VOX = 64


def _report(case, what, value, bound):
    print('TABLES %-28s %-28s %.3e  bound %.3e' % (case, what, value, bound))


def _within(case, what, err, bound):
    """elementwise err <= bound; the line printed holds the entry that uses the largest share of its bound"""
    err, bound = np.asarray(err, dtype=F64), np.broadcast_to(np.asarray(bound, dtype=F64), np.shape(err))
    with np.errstate(divide='ignore', invalid='ignore'):
        share = np.where(bound > 0.0, err / bound, np.where(err > 0.0, np.inf, 0.0))
    k = np.unravel_index(np.argmax(share), err.shape) if err.ndim else ()
    _report(case, what, float(err[k]), float(bound[k]))
    assert np.isfinite(err).all() and (err <= bound).all(), (case, what, float(err[k]), float(bound[k]), k)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == F32 else np.uint64)


def _fetch(ctx, lut, name, shape, dtype=F64):
    from amico_amd import _capi
    return _capi.debug_fetch(ctx, lut, name, shape, dtype)


def _signals(atoms_of, n_atoms, seed):
    """N_VOX voxels spread over the orientations: mixtures of three atoms with a little noise; (y float64, dirs)"""
    rng = np.random.default_rng(seed)
    dirs = T.orientations()[0]
    ori = np.arange(N_VOX) % T.N_ORI
    y = []
    for v in range(N_VOX):
        A = atoms_of(ori[v]).astype(F64)
        w = np.zeros(n_atoms)
        w[rng.choice(n_atoms, 3, replace=False)] = rng.dirichlet(np.ones(3))
        y.append(np.abs(A @ w + 0.02 * rng.standard_normal(A.shape[0])))
    return np.ascontiguousarray(y), np.ascontiguousarray(dirs[ori])


# ================================================================================================ NODDI: the tables of an upload
FULL_RANK = ('bench', 'v150', 'v288', 'exvivo', 'single_b0', 'nonunit_b0')


def _check_gram(case, what, G, A, rows, n, ldG, n_terms):
    assert (G[:, n:] == 0.0).all(), (case, what, 'padding')
    assert np.array_equal(_bits(G[:, :n]), _bits(np.ascontiguousarray(G[:, :n].T))), (case, what, 'symmetry')
    Gref, S = T.gram(A, rows)
    _within(case, what, np.abs(G[:, :n].astype(LD) - Gref), T.gram_bound(S, n_terms))


def _check_basis(case, stage, U, S, Sf, kap, kap0, Acols, nS, rows, rng, full_rank):
    """one orientation: U [nS][12], S [n][12], Sf [12][192], the columns Acols [nS][n] (long double) the basis was built from"""
    n = Acols.shape[1]
    tag = 'stage %d ' % stage
    assert np.isfinite(U).all() and np.isfinite(S).all() and np.isfinite(Sf).all() and np.isfinite([kap, kap0]).all(), (case, stage)
    if rows is not None:
        assert (U[~rows] == 0.0).all(), (case, 'rows of U2 outside the stage-2 rows')
    diag, off = T.basis_defect(U)
    bound = 8 * nS * T.U52
    dead = diag == 0.0
    assert (U[:, dead] == 0.0).all()
    _within(case, tag + "U'U off-diagonal", off, bound)
    _within(case, tag + "U'U diagonal - 1", np.abs(diag[~dead] - 1.0).max(initial=0.0), bound)
    if full_rank:
        assert not dead.any(), (case, stage, 'a full-rank dictionary lost a direction', diag)
    # S = U'A from the fetched U
    _within(case, tag + "S - U'A", np.abs(S.T.astype(LD) - T.matmul(U.T, Acols)), T.product_bound(U.T, Acols.astype(F64), nS))
    assert np.array_equal(_bits(Sf[:, :n]), _bits(np.ascontiguousarray(S.T).astype(F32))), (case, stage, 'screen_S is not (float)S')
    assert (Sf[:, n:] == 0.0).all(), (case, stage, 'screen_S padding')
    # kappa0 = max ||a_j - U U'a_j||, kappa = kappa0 + 2e-6 max ||a_j||
    E = T.residual_columns(U, Acols)
    en, an = T.column_norms(E), T.column_norms(Acols)
    e, amax = float(en.max()), float(an.max())
    _within(case, tag + 'kappa0 - e', abs(kap0 - e), 64 * nS * T.U52 * amax)
    _within(case, tag + 'kappa rel', abs(kap - (kap0 + 2e-6 * amax)) / kap, 1e-12)
    # the screening inequality on the vectors a certificate could meet
    A64 = Acols.astype(F64)
    jw = int(np.argmax(en))
    R = [A64]
    if en[jw] > 0.0:
        R.append((E[:, jw] / LD(en[jw])).astype(F64)[:, None])
    rnd = rng.standard_normal((nS, 32))
    if rows is not None:
        rnd[~rows] = 0.0
    rnd /= np.linalg.norm(rnd, axis=0, keepdims=True)
    R += [rnd, A64[:, np.arange(32) % n] + amax * rnd]
    slack = T.screen_slack(A64, U, Sf[:, :n], kap, np.hstack(R))
    _report(case, tag + 'screen slack (>= 0)', slack, 0.0)
    assert slack >= 0.0, (case, stage, 'the screen would skip an atom whose dual value it underestimates', slack)
    return e, amax


@pytest.mark.parametrize('name', T.NODDI_SHAPES)
def test_noddi_upload_tables(name):
    from amico_amd import _capi, get_context
    K, sch, exvivo = T.noddi_case(name)
    ht = T.orientations()[1]
    ctx = get_context()
    lut = _capi.upload_noddi(ctx, K, ht, sch.dwi_idx, is_exvivo=exvivo)
    n_wm, nd, nS = K['wm'].shape
    n = n_wm + 1 + int(exvivo)
    ldA, ts, ldG = T.lda_of(n), T.tile_stride_of(nS, n), 192
    branches = T.noddi_branches(nS, n)
    rng = np.random.default_rng(7)
    # ---- host-side: rows of stage 2 (single-b0 rule: j + 1), column scales, s2_derive
    rows = np.zeros(nS, dtype=bool)
    rows[(np.arange(sch.dwi_count) + 1) if nS == 1 + sch.dwi_count else np.asarray(sch.dwi_idx)] = True
    assert np.array_equal(_fetch(ctx, lut, 'rowdwi', (nS,), np.uint8), rows.astype(np.uint8))
    colscale = np.ones(n)
    colscale[:n_wm] = K['norms'][0]
    assert np.array_equal(_bits(_fetch(ctx, lut, 'colscale', (n,))), _bits(colscale))
    assert int(_fetch(ctx, lut, 's2_derive', (1,), np.int32)[0]) == (0 if name in ('exvivo', 'nonunit_b0') else 1)
    # ---- tiles (k_build_lut): bit-equal, padding 0
    tiles = _fetch(ctx, lut, 'tiles', (nd, ts), F32)
    atoms = [T.noddi_atoms(K, d, exvivo) for d in range(nd)]
    if exvivo:
        assert (atoms[0][:, n_wm] == 1.0).all()
    for d in range(nd):
        assert np.array_equal(_bits(tiles[d]), _bits(T.tile_layout(atoms[d], ldA, ts))), (name, d, 'tile')
    # ---- Gram matrices (k_build_gram, LDS / global branch)
    G1, G2 = _fetch(ctx, lut, 'gram', (nd, n, ldG)), _fetch(ctx, lut, 'gram_dwi', (nd, n, ldG))
    for d in range(nd):
        _check_gram(name, 'gram', G1[d], atoms[d], None, n, ldG, nS)
        _check_gram(name, 'gram_dwi', G2[d], atoms[d], rows, n, ldG, nS)
    # ---- bases, screening tables, kappa, u2iso (k_build_basis in LDS / on a global scratch block, k_u2iso)
    if not branches['seeds']:
        for which in ('basis_U', 'basis_S', 'basis2_U', 'basis2_S', 'screen_S', 'screen2_S', 'screen_kappa', 'screen2_kappa0', 'u2iso'):
            with pytest.raises(ValueError, match='no seeds for more than 160 atoms'):
                _fetch(ctx, lut, which, (1,))
        return
    U1, S1 = _fetch(ctx, lut, 'basis_U', (nd, nS, 12)), _fetch(ctx, lut, 'basis_S', (nd, n, 12))
    U2, S2 = _fetch(ctx, lut, 'basis2_U', (nd, nS, 12)), _fetch(ctx, lut, 'basis2_S', (nd, n_wm, 12))
    Sf1, Sf2 = _fetch(ctx, lut, 'screen_S', (nd, 12, 192), F32), _fetch(ctx, lut, 'screen2_S', (nd, 12, 192), F32)
    k1, k10 = _fetch(ctx, lut, 'screen_kappa', (nd,)), _fetch(ctx, lut, 'screen_kappa0', (nd,))
    k2, k20 = _fetch(ctx, lut, 'screen2_kappa', (nd,)), _fetch(ctx, lut, 'screen2_kappa0', (nd,))
    u2iso = _fetch(ctx, lut, 'u2iso', (nd, 12))
    for d in range(nd):
        A1 = atoms[d].astype(LD)
        e1, a1 = _check_basis(name, 1, U1[d], S1[d], Sf1[d], k1[d], k10[d], A1, nS, None, rng, name in FULL_RANK)
        A2 = (A1[:, :n_wm] * colscale[:n_wm].astype(LD)[None, :]) * rows[:, None]
        e2, a2 = _check_basis(name, 2, U2[d], S2[d], Sf2[d], k2[d], k20[d], A2, nS, rows, rng, name in FULL_RANK)
        iso = atoms[d][:, n - 1].astype(F64)[:, None]
        _within(name, "u2iso - U2'iso", np.abs(u2iso[d].astype(LD) - T.matmul(U2[d].T, iso)[:, 0]), T.product_bound(U2[d].T, iso, nS)[:, 0])
        if d == 0:
            print('TABLES %-28s kappa0 / max||a||: stage 1 %.3e / %.3e, stage 2 %.3e / %.3e' % (name, e1, a1, e2, a2))


# ================================================================================================ refusals of amx_debug_fetch
def test_fetch_refuses_what_it_cannot_copy():
    from amico_amd import _capi, get_context
    ctx = get_context()
    ht = T.orientations()[1]
    K, sch, _ = T.noddi_case('atoms5')
    noddi = _capi.upload_noddi(ctx, K, ht, sch.dwi_idx)
    fw = _capi.upload_freewater(ctx, T.fw_kernels(10), ht)
    nS, nd = sch.nS, T.N_ORI
    assert _fetch(ctx, noddi, 'basis_U', (nd, nS, 12)).shape == (nd, nS, 12)                    # the whole table, and less, are fine
    assert _fetch(ctx, noddi, 'basis_U', (1, nS, 12)).shape == (1, nS, 12)
    with pytest.raises(ValueError, match='bytes asked of a table of %d' % (nd * nS * 12 * 8)):
        _fetch(ctx, noddi, 'basis_U', (nd, nS, 13))
    with pytest.raises(ValueError, match='bytes asked of a table of 4'):
        _fetch(ctx, noddi, 's2_derive', (2,), np.int32)
    with pytest.raises(ValueError, match='no fit has built that table'):
        _fetch(ctx, fw, 'fw_prep', (1,))
    for lut, which in ((fw, 'basis_U'), (fw, 'gram_dwi'), (noddi, 'fw_prep'), (noddi, 'czb_prep'), (fw, 'sandi_prep'), (noddi, 'sandi_long_prep')):
        with pytest.raises(ValueError, match="model has no such table"):
            _fetch(ctx, lut, which, (1,))
    with pytest.raises(ValueError, match='has no such table'):                                  # 11 atoms: no Gram tables
        _fetch(ctx, fw, 'gram', (1,))
    with pytest.raises(ValueError, match='needs a dictionary handle'):
        _fetch(ctx, None, 'basis_U', (1,))
    with pytest.raises(ValueError, match='no such'):
        _fetch(ctx, noddi, 27, (1,))
    with pytest.raises(ValueError, match='no such buffer'):
        _fetch(ctx, noddi, 99, (1,))
    dic = _capi.Dict(ctx, np.eye(4))
    with pytest.raises(ValueError, match='not dense'):
        _fetch(ctx, dic, 'dict_gram', (1,))
    with pytest.raises(ValueError, match='not an amx_lut handle'):
        _fetch(ctx, dic, 'basis_U', (1,))
    with pytest.raises(ValueError, match='reads an amx_dict handle'):
        _fetch(ctx, noddi, 'dict_gram', (1,))
    other = _capi.Context(-1)
    try:
        with pytest.raises(ValueError, match='belongs to another context'):
            _fetch(other, noddi, 'basis_U', (1,))
        with pytest.raises(ValueError, match='no fit on this context'):
            _fetch(other, None, 'perm', (1,), np.int32)
    finally:
        other.close()


# ================================================================================================ FreeWater: A | H^-1 | H per lambda2
def _check_fw(case, tab, K, n, nS, lam2):
    N = 11 if n <= 11 else 12
    for d in range(T.N_ORI):
        A, Hi, H = T.fw_split(tab[d], nS, N)
        A32 = T.fw_atoms(K, d)
        assert np.array_equal(_bits(A[:, :n]), _bits(A32.astype(F64))) and (A[:, n:] == 0.0).all(), (case, 'A')
        G, S = T.gram(A32)
        Href, SH = T.ridge(G, S, lam2)
        _within(case, 'H', np.abs(H[:n, :n].astype(LD) - Href), T.gram_bound(SH, nS + 1))
        assert np.array_equal(_bits(H), _bits(np.ascontiguousarray(H.T))), (case, 'H symmetric')
        pad = np.eye(N)
        pad[:n, :n] = H[:n, :n]
        assert np.array_equal(H, pad), (case, 'identity on the padding atoms of H')
        assert (Hi[:, N:] == 0.0).all()
        X = Hi[:, :N]
        padx = np.eye(N)
        padx[:n, :n] = X[:n, :n]
        assert np.array_equal(X, padx), (case, 'identity on the padding atoms of H^-1')
        _within(case, 'H H^-1 - I', T.inverse_residual(Href, X[:n, :n]), T.inverse_bound(Href))


@pytest.mark.parametrize('n_atoms', T.FW_ATOMS)
def test_freewater_tables_and_their_cache(n_atoms):
    from amico_amd import _capi, get_context
    ctx = get_context()
    K, ht, nS = T.fw_kernels(n_atoms), T.orientations()[1], T.fw_scheme().nS
    N = 11 if n_atoms <= 11 else 12
    used = nS * 12 + N * 12 + N * N                    # (rounded up to even for the next orientation's alignment: that word is never written)
    words = (used + 1) & ~1
    y, dirs = _signals(lambda d: T.fw_atoms(K, d), n_atoms, 11)
    a, b = T.FW_LAM2

    def run(lut, lam2):
        _capi.freewater_fit(ctx, lut, y, dirs, 0.0, lam2, False)
        path = ctx.last_path()
        assert ('k_freewater_fused<%d>' % N) in path or ('k_fw_project' in path and 'k_freewater_refill' in path), path
        return _fetch(ctx, lut, 'fw_prep', (T.N_ORI, words))

    lut = _capi.upload_freewater(ctx, K, ht)
    with pytest.raises(ValueError, match='no fit has built that table'):
        _fetch(ctx, lut, 'fw_prep', (T.N_ORI, words))
    ta, tb, ta2 = run(lut, a), run(lut, b), run(lut, a)
    with pytest.raises(ValueError, match='bytes asked'):
        _fetch(ctx, lut, 'fw_prep', (T.N_ORI, words + 2))
    _check_fw('FreeWater %d atoms, %g' % (n_atoms, a), ta, K, n_atoms, nS, a)
    _check_fw('FreeWater %d atoms, %g' % (n_atoms, b), tb, K, n_atoms, nS, b)
    assert np.array_equal(_bits(ta[:, :used]), _bits(ta2[:, :used])), 'lambda2 a, b, a: the third tables are not the first'
    fresh = run(_capi.upload_freewater(ctx, K, ht), b)
    assert np.array_equal(_bits(tb[:, :used]), _bits(fresh[:, :used])), 'tables at b differ from a fresh handle'


# ================================================================================================ CylinderZeppelinBall: M | H | M 1 | M A' | A'
def _check_czb(case, tab, K, n, nS, nSp, lam2):
    for d in range(T.N_ORI):
        M, H, m1, B, At = T.czb_split(tab[d], nSp)
        A32 = T.czb_atoms(K, d)
        A = A32.astype(F64)
        want = np.zeros((32, nSp))
        want[:n, :nS] = A.T
        assert np.array_equal(_bits(At), _bits(want)), (case, "A'")
        G, S = T.gram(A32)
        Href, SH = T.ridge(G, S, lam2)
        _within(case, 'H', np.abs(H[:n, :n].astype(LD) - Href), T.gram_bound(SH, nS + 1))
        outside = np.ones((32, 33), dtype=bool)
        outside[:n, :n] = False
        assert (H[outside] == 0.0).all() and (M[outside] == 0.0).all(), (case, 'zero outside the dictionary')
        assert np.array_equal(_bits(M[:, :32]), _bits(np.ascontiguousarray(M[:, :32].T))), (case, 'M symmetric')
        Mn = M[:n, :n]
        _within(case, 'H M - I', T.inverse_residual(Href, Mn), T.inverse_bound(Href))
        # products of the inverse, against the long-double products of the FETCHED M
        ones = np.ones((n, 1))
        _within(case, 'M 1', np.abs(m1[:n].astype(LD) - T.matmul(Mn, ones)[:, 0]), T.product_bound(Mn, ones)[:, 0])
        _within(case, "M A'", np.abs(B[:n, :nS].astype(LD) - T.matmul(Mn, A.T)), T.product_bound(Mn, A.T))
        assert (m1[n:] == 0.0).all() and (B[n:] == 0.0).all() and (B[:, nS:] == 0.0).all(), (case, 'padding of M 1, M A\'')


@pytest.mark.parametrize('n_atoms,nS', T.CZB_SHAPES)
def test_czb_tables_and_their_cache(n_atoms, nS):
    from amico_amd import _capi, get_context
    ctx = get_context()
    (K, Rs), ht = T.czb_kernels(n_atoms, nS), T.orientations()[1]
    nSp = 100 if nS <= 100 else 160
    stride = 2 * 32 * 33 + 32 + 2 * 32 * nSp
    y, dirs = _signals(lambda d: T.czb_atoms(K, d), n_atoms, 12)
    a, b = T.CZB_LAM2

    def run(lut, lam2):
        _capi.czb_fit(ctx, lut, y, dirs, 0.0, lam2)
        path = ctx.last_path()
        assert ('k_czb_project<25>' if nS <= 100 else 'k_czb_project<40>') in path and 'k_czb_lane' in path, path
        return _fetch(ctx, lut, 'czb_prep', (T.N_ORI, stride))

    lut = _capi.upload_czb(ctx, K, Rs, ht)
    ta, tb, ta2 = run(lut, a), run(lut, b), run(lut, a)
    with pytest.raises(ValueError, match='bytes asked'):
        _fetch(ctx, lut, 'czb_prep', (T.N_ORI, stride + 1))
    case = 'CZB %d atoms %d volumes' % (n_atoms, nS)
    _check_czb(case + ', %g' % a, ta, K, n_atoms, nS, nSp, a)
    _check_czb(case + ', %g' % b, tb, K, n_atoms, nS, nSp, b)
    assert np.array_equal(_bits(ta), _bits(ta2)), 'lambda2 a, b, a: the third tables are not the first'
    assert np.array_equal(_bits(tb), _bits(run(_capi.upload_czb(ctx, K, Rs, ht), b))), 'tables at b differ from a fresh handle'
    # the Gram table the H above is made from (k_build_gram, ldG = 64)
    G = _fetch(ctx, lut, 'gram', (T.N_ORI, n_atoms, 64))
    for d in range(T.N_ORI):
        _check_gram(case, 'gram', G[d], T.czb_atoms(K, d), None, n_atoms, 64, nS)


# ================================================================================================ SANDI 6 x 15: T | G | g0 | A
def _check_sandi_rows(case, tab, A, lam1, lam2):
    M, N = A.shape
    Tt, G, g0, Ap = tab[:N * 22].reshape(N, 22), tab[N * 22:N * 22 + N * M].reshape(N, M), tab[N * 28:N * 28 + 16], tab[N * 28 + 16:N * 28 + 16 + M * 16].reshape(M, 16)
    ref = T.sandi_row_tables(A, lam1, lam2)
    assert np.array_equal(_bits(Tt[:, :21]), _bits(ref['T'])) and (Tt[:, 21] == 0.0).all(), (case, 'T')
    assert np.array_equal(_bits(Ap[:, :N]), _bits(A)) and (Ap[:, N:] == 0.0).all(), (case, 'A')
    # G = A'W with W = B^-1 the kernel's own (not kept): G B - A' = A'(W B - I), and W B - I is held to the inverse bound; the two
    # products (M terms each) to the product bound
    B, W = ref['B'], ref['W']
    res = np.abs(T.matmul(G, B) - A.T.astype(LD))
    bound = np.abs(A.T).sum(axis=1, keepdims=True) * T.inverse_bound(B) + 2 * M * T.U52 * T.absmul(T.absmul(A.T, W), B)
    _within(case, "G B - A'", res, bound)
    # g0 = -(lambda1 / lambda2) (1 - a_j'W A 1), from the FETCHED G: a_j'W A 1 = (G A 1)_j up to the rounding of the sums
    A1 = A.sum(axis=1, keepdims=True)
    want = -(LD(lam1) / LD(lam2)) * (1 - T.matmul(G, A1)[:, 0])
    gb = (lam1 / lam2) * ((2 * M + N + 2) * T.U52 * (T.absmul(T.absmul(A.T, W), np.abs(A).sum(axis=1, keepdims=True))[:, 0] + 1.0))
    _within(case, 'g0', np.abs(g0[:N].astype(LD) - want), gb)
    assert g0[N] == 0.0
    if lam1 == 0.0:
        assert (g0 == 0.0).all()


def test_sandi_row_tables_and_their_cache():
    from amico_amd import _capi, get_context
    ctx = get_context()
    K, Rs, d_in, d_isos = T.sandi_dictionary(6, 15)
    A = np.ascontiguousarray(K['signal'])
    y, _ = _signals(lambda d: A, 15, 13)
    words = 15 * 22 + 15 * 6 + 16 + 8 * 16

    def run(lut, lam1, lam2):
        _capi.sandi_fit(ctx, lut, y, lam1, lam2)
        assert 'k_sandi_rows<6,15>' in ctx.last_path(), ctx.last_path()
        return _fetch(ctx, lut, 'sandi_prep', (words,))

    lut = _capi.upload_sandi(ctx, K, Rs, d_in, d_isos)
    (l1a, l2a), (l1b, l2b), (l1c, l2c) = T.SANDI_ROWS_LAMBDAS
    ta, tb, tc, ta2 = run(lut, l1a, l2a), run(lut, l1b, l2b), run(lut, l1c, l2c), run(lut, l1a, l2a)
    with pytest.raises(ValueError, match='bytes asked'):
        _fetch(ctx, lut, 'sandi_prep', (words + 1,))
    for tab, (lam1, lam2) in zip((ta, tb, tc), T.SANDI_ROWS_LAMBDAS):
        _check_sandi_rows('SANDI 6 x 15, %g %g' % (lam1, lam2), tab, A, lam1, lam2)
    assert np.array_equal(_bits(ta[:words - 32]), _bits(ta2[:words - 32])), 'lambda a, b, c, a: the last tables are not the first'
    fresh = run(_capi.upload_sandi(ctx, K, Rs, d_in, d_isos), l1b, l2b)
    assert np.array_equal(_bits(tb[:words - 32]), _bits(fresh[:words - 32])), 'tables at b differ from a fresh handle'


# ================================================================================================ SANDI, long protocols: G | H | A' operand
@pytest.mark.parametrize('nS,n_atoms', T.SANDI_LONG_SHAPES)
def test_sandi_long_tables_and_their_cache(nS, n_atoms):
    from amico_amd import _capi, get_context
    ctx = get_context()
    K, Rs, d_in, d_isos = T.sandi_dictionary(nS, n_atoms)
    A = np.ascontiguousarray(K['signal'])
    y, _ = _signals(lambda d: A, n_atoms, 14)
    NP, KS = -(-n_atoms // 16) * 16, 4 * -(-nS // 16)
    words = 2 * NP * NP + (NP // 16) * KS * 64
    a, b = T.SANDI_LONG_LAM2

    def run(lut, lam2):
        _capi.sandi_fit(ctx, lut, y, 0.1, lam2)
        assert 'k_sandi_project<double>' in ctx.last_path(), ctx.last_path()
        return _fetch(ctx, lut, 'sandi_long_prep', (words,))

    lut = _capi.upload_sandi(ctx, K, Rs, d_in, d_isos)
    ta, tb, ta2 = run(lut, a), run(lut, b), run(lut, a)
    with pytest.raises(ValueError, match='bytes asked'):
        _fetch(ctx, lut, 'sandi_long_prep', (words + 1,))
    Gref, S = T.gram(A)
    op = T.sandi_long_operand(A, NP, KS)
    for tab, lam2 in ((ta, a), (tb, b)):
        case = 'SANDI %d x %d, %g' % (nS, n_atoms, lam2)
        G, H, At = tab[:NP * NP].reshape(NP, NP), tab[NP * NP:2 * NP * NP].reshape(NP, NP), tab[2 * NP * NP:]
        # float64 tiles: every product rounds once as well -- one more term than the sums of exact products
        _within(case, 'G', np.abs(G[:n_atoms, :n_atoms].astype(LD) - Gref), T.gram_bound(S, nS + 1))
        assert np.array_equal(_bits(G), _bits(np.ascontiguousarray(G.T))), (case, 'G symmetric')
        pad = np.zeros((NP, NP))
        pad[:n_atoms, :n_atoms] = G[:n_atoms, :n_atoms]
        assert np.array_equal(G, pad), (case, 'G padding')
        want = G + np.diag(np.where(np.arange(NP) < n_atoms, lam2, 1.0))           # lambda2 added exactly once, identity on the padding
        assert np.array_equal(_bits(H), _bits(want)), (case, 'H')
        assert np.array_equal(_bits(At), _bits(op)), (case, "A' operand")
    assert np.array_equal(_bits(ta), _bits(ta2)), 'lambda2 a, b, a: the third tables are not the first'
    assert np.array_equal(_bits(tb), _bits(run(_capi.upload_sandi(ctx, K, Rs, d_in, d_isos), b))), 'tables at b differ from a fresh handle'


# ================================================================================================ Gram tables of the dense routes
@pytest.mark.parametrize('n_atoms', [65, 66, 256])
@pytest.mark.parametrize('model', ['FreeWater', 'SANDI'])
def test_big_gram(model, n_atoms):
    """k_big_gram<float> (FreeWater tiles) and <double> (SANDI tiles), ldG = (n + 3) & ~3: 68 with padding, 256 without"""
    from amico_amd import _capi, get_context
    from amico_amd import synthetic as S
    ctx = get_context()
    ldG = (n_atoms + 3) & ~3
    case = 'big Gram %s %d' % (model, n_atoms)
    if model == 'FreeWater':
        sch = T.fw_scheme()
        K = S.freewater_kernels(sch, T.orientations()[0], d_perps=np.linspace(0.05, 1.0, n_atoms - 1) * 1e-3)
        lut = _capi.upload_freewater(ctx, K, T.orientations()[1])
        atoms, nd, terms = [T.fw_atoms(K, d) for d in range(T.N_ORI)], T.N_ORI, sch.nS
    else:
        K, Rs, d_in, d_isos = T.sandi_dictionary(20, n_atoms)
        lut = _capi.upload_sandi(ctx, K, Rs, d_in, d_isos)
        atoms, nd, terms = [np.ascontiguousarray(K['signal'])], 1, 20 + 1          # (float64 tiles: the products round too)
    G = _fetch(ctx, lut, 'gram', (nd, n_atoms, ldG))
    with pytest.raises(ValueError, match='bytes asked'):
        _fetch(ctx, lut, 'gram', (nd, n_atoms, ldG + 1))
    for d in range(nd):
        _check_gram(case, 'gram', G[d], atoms[d], None, n_atoms, ldG, terms)


@pytest.mark.parametrize('n', [7, 8, 66])
def test_dict_gram(n):
    """k_dict_gram of a dense Dict: odd and even n (ldG = n rounded up to odd: 7, 9, 67), two dictionaries"""
    from amico_amd import _capi, get_context
    ctx = get_context()
    rng = np.random.default_rng(n)
    m = 13
    A = rng.standard_normal((2, m, n))
    dic = _capi.Dict(ctx, A, dense=True)
    ldG = n | 1
    G = _fetch(ctx, dic, 'dict_gram', (2, n, ldG))
    with pytest.raises(ValueError, match='bytes asked'):
        _fetch(ctx, dic, 'dict_gram', (2, n + 1, ldG))
    for d in range(2):
        _check_gram('Dict %d' % n, 'gram', G[d], A[d], None, n, ldG, m + 1)
    dic.set_dense(False)
    with pytest.raises(ValueError, match='not dense'):
        _fetch(ctx, dic, 'dict_gram', (1,))
