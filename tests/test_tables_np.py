"""tables_np.py on hand cases, and the conditions test_gpu_tables.py relies on: numpy's own float64 inverse stays within the inverse
bound on every matrix chosen there, the chosen NODDI shapes take the branches they are named for, the rank-deficient dictionaries are
rank deficient.  CPU only."""
import numpy as np
import pytest

import tables_np as T

LD = T.LD


def test_high_precision_is_wider_than_double():
    a = np.array([[1.0, 2.0 ** -60]])
    assert float(T.matmul(a, np.array([[1.0], [1.0]]))[0, 0] - LD(1)) == 2.0 ** -60 or not T.WIDE
    # the rational fallback gives the exactly rounded product whatever long double is
    wide, T.WIDE = T.WIDE, False
    try:
        x = np.array([[1e16, 1.0, -1e16]])
        assert float(T.matmul(x, np.ones((3, 1)))[0, 0]) == 1.0
    finally:
        T.WIDE = wide


def test_gram_2x2_and_rows():
    A = np.array([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]], dtype=np.float32)
    G, S = T.gram(A)
    assert np.array_equal(G.astype(np.float64), [[35.0, 44.0], [44.0, 56.0]])
    assert np.array_equal(S, [[35.0, 44.0], [44.0, 56.0]])
    G, S = T.gram(A * np.array([1.0, -1.0], dtype=np.float32), rows=[0, 2])
    assert np.array_equal(G.astype(np.float64), [[26.0, -32.0], [-32.0, 40.0]]) and np.array_equal(S, [[26.0, 32.0], [32.0, 40.0]])
    assert np.array_equal(T.gram_bound(S, 2), 2 * 2.0 ** -53 * S)


def test_gram_bound_holds_for_a_float64_sum_of_float32_products():
    rng = np.random.default_rng(0)
    A = rng.standard_normal((288, 7)).astype(np.float32)
    G, S = T.gram(A)
    acc = np.zeros((7, 7))
    for i in range(A.shape[0]):                        # the kernels' order: one row after the other
        acc += np.outer(A[i].astype(np.float64), A[i].astype(np.float64))
    err = np.abs(acc.astype(LD) - G).astype(np.float64)
    assert (err <= T.gram_bound(S, A.shape[0])).all() and err.max() > 0.0


def test_ridge_pads_with_identity():
    G, S = T.gram(np.array([[1.0, 0.0], [0.0, 2.0]], dtype=np.float32))
    H, SH = T.ridge(G, S, 0.5, n_pad=4)
    assert np.array_equal(H.astype(np.float64), np.diag([1.5, 4.5, 1.0, 1.0]))
    assert np.array_equal(SH, np.diag([1.5, 4.5, 0.0, 0.0]))
    H0, _ = T.ridge(G, S, 0.5, n_pad=3, pad_diag=0.0)
    assert np.array_equal(H0.astype(np.float64), np.diag([1.5, 4.5, 0.0]))
    X = T.inverse(H)
    assert np.array_equal(X.astype(np.float64), np.diag([1.0 / 1.5, 1.0 / 4.5, 1.0, 1.0]))
    assert T.inverse_residual(H, X) < 1e-18 or not T.WIDE


def test_inverse_reference_beats_float64():
    H = np.array([[4.0, 1.0], [1.0, 3.0]])
    X = T.inverse(H)
    assert np.abs(X.astype(np.float64) - np.array([[3.0, -1.0], [-1.0, 4.0]]) / 11.0).max() < 1e-16
    assert T.cond2(np.diag([4.0, 0.5])) == 8.0
    assert T.inverse_bound(np.diag([4.0, 0.5])) == 8 * 2 * 2.0 ** -52 * 8.0


def test_numpy_inverse_meets_the_inverse_bound_on_every_chosen_matrix():
    """what test_gpu_tables.py asks of the device inverses, asked of numpy's float64 inverse first; also that the long-double
    reference inverse is far inside it"""
    worst = 0.0
    count = 0
    for label, H in T.inverse_inputs():
        bound = T.inverse_bound(H)
        res = T.inverse_residual(H, np.linalg.inv(H.astype(np.float64)))
        assert res <= bound, (label, res, bound)
        assert T.inverse_residual(H, T.inverse(H)) <= 1e-3 * bound, label
        assert np.isfinite(bound) and T.cond2(H) < 1e9, (label, T.cond2(H))       # the bound says something
        worst = max(worst, res / bound)
        count += 1
    assert count == len(T.FW_ATOMS) * len(T.FW_LAM2) * T.N_ORI + len(T.CZB_SHAPES) * len(T.CZB_LAM2) * T.N_ORI + len(T.SANDI_ROWS_LAMBDAS)
    print('numpy inverse: largest residual / bound %.3g over %d matrices' % (worst, count))


def test_product_bound():
    X = np.array([[1.0, -2.0, 3.0]])
    Y = np.array([[1.0], [1.0], [-1.0]])
    assert T.product_bound(X, Y)[0, 0] == 3 * 2.0 ** -52 * 6.0
    assert T.product_bound(X, Y, n_terms=10)[0, 0] == 10 * 2.0 ** -52 * 6.0


def test_tile_layout():
    A = np.arange(6, dtype=np.float32).reshape(3, 2) + 1
    assert T.lda_of(2) == 3 and T.lda_of(145) == 145 and T.tile_stride_of(3, 2) == 12 and T.tile_stride_of(99, 145) == 14356
    t = T.tile_layout(A, 3, 12)
    assert np.array_equal(t, [1, 2, 0, 3, 4, 0, 5, 6, 0, 0, 0, 0])


def test_basis_properties_on_hand_cases():
    U = np.zeros((4, T.KD))
    U[0, 0] = U[1, 1] = 1.0                           # two live directions, ten dead ones
    d, off = T.basis_defect(U)
    assert np.array_equal(d, [1.0, 1.0] + [0.0] * 10) and off == 0.0
    A = np.array([[1.0, 0.0], [2.0, 0.0], [0.0, 3.0], [0.0, 4.0]])
    E = T.residual_columns(U, A)
    assert np.array_equal(E.astype(np.float64), [[0, 0], [0, 0], [0, 3], [0, 4]])
    assert np.array_equal(T.column_norms(E), [0.0, 5.0])
    U[:, 2] = [1.0, 0.0, 0.0, 0.0]                    # a repeated direction is a defect
    assert T.basis_defect(U)[1] == 1.0


def test_screen_restatement():
    """ut in float32 in the kernel's order; the slack is zero where the screen is exactly tight"""
    Sf = np.array([[1.0, 2.0], [0.5, -1.0]], dtype=np.float32)
    ut = T.screen_values(Sf, np.array([[2.0], [4.0]]))
    assert ut.dtype == np.float32 and np.array_equal(ut[:, 0], [4.0, 0.0])
    # float32 rounding of the projected residual enters: 1 + 2^-30 is 1 in float32
    assert T.screen_values(Sf, np.array([[1.0 + 2.0 ** -30], [0.0]]))[0, 0] == 1.0
    U = np.eye(3)[:, :2]
    A = np.array([[1.0, 0.0], [0.0, 1.0], [0.0, 0.5]])        # atom 1 has a part outside the basis
    S2 = np.ascontiguousarray((U.T @ A)).astype(np.float32)                  # [d][j]
    r = np.array([[0.0], [0.0], [1.0]])
    assert T.screen_slack(A, U, S2, 0.0, r) == -0.5           # kappa too small: the screen misjudges atom 1 by e_1'r
    assert T.screen_slack(A, U, S2, 0.5 / 1.0625, r) == 0.0   # kappa = ||e_1||: tight
    assert T.screen_slack(A, U, S2, 0.5, np.hstack([r, 2 * r])) == 0.03125      # 1.0625 * 0.5 - 0.5, the smaller of the two vectors'


def test_sandi_row_tables_on_a_hand_case():
    A = np.array([[1.0, 0.0, 0.5], [0.0, 2.0, 0.5]])          # M = 2 rows, N = 3 atoms
    t = T.sandi_row_tables(A, 0.0, 1.0)
    assert np.array_equal(t['T'], [[1.0, 0.0, 0.0], [0.0, 0.0, 4.0], [0.25, 0.25, 0.25]])      # packed (0,0) (1,0) (1,1)
    B = np.array([[2.25, 0.25], [0.25, 5.25]])
    assert np.array_equal(t['B'].astype(np.float64), B)
    assert np.abs(t['G'].astype(np.float64) - A.T @ np.linalg.inv(B)).max() < 1e-15
    assert np.array_equal(t['g0'].astype(np.float64), np.zeros(3))
    # the Woodbury form is the full-set optimum: z0 = (A'A + lambda2 I)^-1 (A'y - lambda1)
    lam1, lam2, y = 0.3, 0.7, np.array([1.0, 2.0])
    t = T.sandi_row_tables(A, lam1, lam2)
    z0 = np.linalg.solve(A.T @ A + lam2 * np.eye(3), A.T @ y - lam1)
    assert np.abs((t['G'] @ y + t['g0']).astype(np.float64) - z0).max() < 1e-14


def test_sl_volume_and_operand_order():
    vols = sorted(T.sl_volume(s, q) for s in range(8) for q in range(4))
    assert vols == list(range(32))                            # every volume of two 16-volume chunks exactly once
    assert [T.sl_volume(s, 1) for s in range(4)] == [4, 5, 6, 7] and T.sl_volume(4, 0) == 16
    A = np.arange(1, 18 * 3 + 1, dtype=np.float64).reshape(18, 3)      # 18 volumes, 3 atoms: NP 16, KS 8
    op = T.sandi_long_operand(A, 16, 8)
    assert op.size == 8 * 64
    assert op[0] == A[0, 0] and op[1] == A[0, 1] and op[16] == A[4, 0] and op[64 + 2] == A[1, 2]
    assert op[4 * 64] == A[16, 0] and op[5 * 64 + 1] == A[17, 1]
    assert op[4 * 64 + 16] == 0.0 and op[3] == 0.0            # volume 20 and atom 3 do not exist
    assert np.count_nonzero(op) == A.size


def test_table_splits():
    nSp = 100
    tab = np.arange(2 * 32 * 33 + 32 + 2 * 32 * nSp, dtype=np.float64)
    M, H, m1, B, At = T.czb_split(tab, nSp)
    assert M[1, 0] == 33 and H[0, 0] == 32 * 33 and m1[0] == 2 * 32 * 33 and B[1, 0] == 2 * 32 * 33 + 32 + nSp and At[0, 0] == B[0, 0] + 32 * nSp
    tab = np.arange((33 * 12 + 11 * 12 + 121 + 1) & ~1, dtype=np.float64)
    A, Hi, H = T.fw_split(tab, 33, 11)
    assert A.shape == (33, 12) and Hi[0, 0] == 33 * 12 and H[0, 0] == 33 * 12 + 11 * 12 and H.shape == (11, 11)


def test_noddi_shapes_take_the_branches_they_are_named_for():
    want = {'bench': (99, 145, True, True, True), 'v150': (150, 145, True, False, True), 'v288': (288, 145, False, False, True),
            'exvivo': (99, 146, True, True, True), 'single_b0': (91, 145, True, True, True), 'nonunit_b0': (99, 145, True, True, True),
            'grid3x3': (99, 10, True, True, True), 'atoms5': (99, 5, True, True, True), 'v10': (10, 145, True, True, True),
            'dup3': (99, 7, True, True, True), 'noseed': (99, 170, True, True, False)}
    assert set(want) == set(T.NODDI_SHAPES)
    for name in T.NODDI_SHAPES:
        K, sch, exvivo = T.noddi_case(name)
        n_atoms = K['wm'].shape[0] + 1 + int(exvivo)
        b = T.noddi_branches(sch.nS, n_atoms)
        assert (sch.nS, n_atoms, b['gram_in_lds'], b['basis_in_lds'], b['seeds']) == want[name], name
        assert K['wm'].shape[1] == T.N_ORI <= 5 and K['norms'].shape == (sch.dwi_count, K['wm'].shape[0])
    assert T.noddi_case('single_b0')[1].nS == 1 + T.noddi_case('single_b0')[1].dwi_count
    K, sch, _ = T.noddi_case('nonunit_b0')
    assert (K['wm'][:, :, sch.b0_idx] != 1.0).sum() == T.N_ORI and (T.noddi_case('bench')[0]['wm'][:, :, sch.b0_idx] == 1.0).all()


@pytest.mark.parametrize('name,rank', [('grid3x3', 10), ('atoms5', 5), ('v10', 10), ('dup3', 4)])
def test_rank_deficient_shapes_are_rank_deficient(name, rank):
    """fewer than kSeedKD = 12 directions exist in these dictionaries: the basis kernel must run out of pivots"""
    K, sch, exvivo = T.noddi_case(name)
    for d in range(T.N_ORI):
        s = np.linalg.svd(T.noddi_atoms(K, d, exvivo).astype(np.float64), compute_uv=False)
        assert (s > 1e-10 * s[0]).sum() <= rank < T.KD, (name, d, s)
    for full in ('bench', 'exvivo'):
        K, sch, exvivo = T.noddi_case(full)
        s = np.linalg.svd(T.noddi_atoms(K, 0, exvivo).astype(np.float64), compute_uv=False)
        assert (s > 1e-10 * s[0]).sum() >= T.KD
