"""The mask gather (amx_prep_gather*) on protocols of up to 512 volumes: k_prep_long, one wavefront and one tile per workgroup, where
two of k_prep_gather's tiles no longer fit 160 KB of LDS.  Every result is held bit for bit to oracle/signal_np.prepare_signal (the
numpy statements of core.py:209-268, 451-452).

Volume counts: the first one the two-tile size check refuses for the route under test (computed here from that check's expression),
449 (odd, a ragged last group of 64 samples) and 512 (the bound).  Spatial shapes are ragged: the fastest axis is never a multiple of
the 64-voxel tile, the mask has holes and holds the first and the last voxel.

Without the long route every test of the gather fails with `scheme too long for the LDS tile` -- the b0 merge on a planar image
included: its streaming kernels need no tile, but the size check came first.  The selection test reads amx_prep_last_launch, which
came with the long route; the 513-volume refusal holds with and without it."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LDS_MAX = 160 * 1024
SHAPE = (70, 9, 5)
TOL = 1e-6                     # maps and error maps against the oracle (tests/test_gpu_sandi_long.py)


def _scheme(n, dwi_first=False):
    """nine b0 volumes + two shells, n volumes in all; dwi_first: the last DWI volume moved to the front"""
    from amico_amd import synthetic as S
    sc = S.make_scheme(n_b0=9, shells=((700.0, 30), (2000.0, n - 39)), seed=0)
    if dwi_first:
        sc = S.SimpleScheme(np.vstack([sc.raw[-1:], sc.raw[:-1]]))
    assert sc.nS == n
    return sc


def _first_refused(row, merged):
    """first volume count whose two tiles (+ the plan's lists) exceed 160 KB: lds = (2 * per_wave + n_b0 + n_out + 1 + n_gidx) * 4"""
    per_wave = {'direct': lambda n: n * 65, 'tile': lambda n: 64 * (n | 1), 'twice': lambda n: 2 * 64 * (n | 1)}[row]
    for n in range(40, 600):
        n_out = n - 8 if merged else n
        if (2 * per_wave(n) + 9 + n_out + 1 + n) * 4 > LDS_MAX:
            assert (150 <= n <= 170) if row == 'twice' else (300 <= n <= 320), n
            return n
    raise AssertionError('no count refused')


def _fill(shape, sc, seed):
    rng = np.random.default_rng(seed)
    img = rng.uniform(0.0, 900.0, shape + (sc.nS,)).astype(np.float32)
    img[..., sc.b0_idx] += 600.0
    img[0, 0, 0, :] = 0.0                          # b0 mean 0 -> norm factor 0
    img[1, 2, 1, 3] = -7.5                         # negative sample -> clipped
    img[2, 1, 0, sc.b0_idx] = -1.0                 # negative b0 mean -> norm factor 0
    img[5, 4, 3, sc.nS - 1] = -0.25                # ... and one in the last, ragged group of 64 samples
    mask = (rng.uniform(size=shape) < 0.6).astype(np.uint8)
    mask[0, 0, 0] = mask[1, 2, 1] = mask[2, 1, 0] = mask[5, 4, 3] = mask[-1, -1, -1] = 1
    mask[3, 3, 2] = 2                              # only == 1 counts (core.py:451)
    return img, mask


@functools.lru_cache(maxsize=4)
def _volume(n, order, dwi_first=False):
    """image [70, 9, 5, n] in the given memory order, its mask and its scheme: made once per shape, shared, read-only"""
    sc = _scheme(n, dwi_first)
    img, mask = _fill(SHAPE, sc, seed=3)
    img = np.asarray(img, order=order)
    img.setflags(write=False)
    mask.setflags(write=False)
    return sc, img, mask


def _flat(img):
    return np.lib.stride_tricks.as_strided(img, shape=(1 + sum((d - 1) * s // 4 for d, s in zip(img.shape, img.strides)),), strides=(4,))


def _gather_device(sp, img, f32, fused_with=None):
    """amx_prep_gather_device[_f32] (or the _directions_ form with the helper `fused_with`) on a device copy -> (y, mean_b0[, dirs]) tensors"""
    import torch
    from amico_amd import _capi
    L, c = _capi.lib(), sp.ctx
    dev = torch.device('cuda', 0)
    d_img = torch.from_numpy(_flat(img).copy()).to(dev)
    y = torch.zeros((sp.n_vox, sp.n_out), dtype=torch.float32 if f32 else torch.float64, device=dev)
    mb = torch.zeros(sp.n_vox, dtype=torch.float32, device=dev)
    thr = float(sp.b0_threshold(img))
    if fused_with is None:
        fn = L.amx_prep_gather_device_f32 if f32 else L.amx_prep_gather_device
        c.check(fn(c._h, sp._plan._h, d_img.data_ptr(), int(sp.do_normalize), thr, y.data_ptr(), mb.data_ptr(), None))
        c.sync(None)
        return y, mb
    dirs = torch.zeros((sp.n_vox, 3), dtype=torch.float64, device=dev)
    fn = L.amx_prep_gather_directions_device_f32 if f32 else L.amx_prep_gather_directions_device
    c.check(fn(c._h, sp._plan._h, fused_with._dti._h, d_img.data_ptr(), int(sp.do_normalize), thr, y.data_ptr(), mb.data_ptr(),
               dirs.data_ptr(), None))
    c.sync(None)
    return y, mb, dirs


def _check_exact(sp, img, ref, mb0, mask, kernel):
    """float64 rows through the host call, twice on one plan (the ring of tile counters), then float32 rows on the device"""
    for _ in range(2):
        y, m = sp.gather(img)
        assert y.shape == ref.shape and np.array_equal(y, ref)
        if sp.do_normalize:
            assert np.array_equal(m, mb0[mask == 1])
    name, grid, block, lds = sp._plan.last_launch()
    assert name.startswith(kernel) and lds <= LDS_MAX and (block == 64) == name.startswith('k_prep_long'), (name, grid, block, lds)
    y32, m32 = _gather_device(sp, img, f32=True)
    assert np.array_equal(y32.cpu().numpy().astype(np.float64), ref)
    if sp.do_normalize:
        assert np.array_equal(m32.cpu().numpy(), mb0[mask == 1])


OPTS = {'plain': dict(), 'raw': dict(do_normalize=False), 'merge': dict(do_merge_b0=True), 'b0min': dict(b0_min_signal=0.9)}


@pytest.mark.parametrize('count', ['first', 449, 512])
@pytest.mark.parametrize('opts', list(OPTS))
@pytest.mark.parametrize('order', ['F', 'C'])
def test_gather_bit_exact(order, opts, count):
    """identity groups in both memory orders (T[volume][voxel] / T[voxel][volume]) and the b0 merge.  The merge on the planar image takes
    the streaming kernels, as it does on short protocols: the control that runs no new kernel"""
    from amico_amd import prep
    from oracle import signal_np
    merged = opts == 'merge'
    n = _first_refused('direct' if order == 'F' and not merged else 'tile', merged) if count == 'first' else count
    sc, img, mask = _volume(n, order)
    ref, mb0 = signal_np.prepare_signal(img, mask, sc.b0_idx, sc.dwi_idx, **OPTS[opts])
    sp = prep.SignalPreparation(sc, img, mask, **OPTS[opts])
    _check_exact(sp, img, ref, mb0, mask, 'k_prep_stream' if merged and order == 'F' else 'k_prep_long')


def _sandi_512(which):
    from amico_amd import synthetic as S
    if which == 'b order':
        return S.make_sandi_scheme(ndir_per_shell=100, n_b0=12)
    sc = S.make_sandi_scheme(bvals=(4000.0, 1000.0, 8000.0, 2500.0, 6000.0), ndir_per_shell=100, n_b0=12)
    if which == 'shells first':                    # b0 volumes at the END: every shell's group reads volumes earlier outputs replaced
        sc = S.SimpleScheme(np.roll(sc.raw, -12, axis=0))
    return sc


@pytest.mark.parametrize('which', ['b order', 'not in b order', 'shells first'])
@pytest.mark.parametrize('order', ['F', 'C'])
def test_directional_average_with_the_view_aliasing(order, which):
    """5 shells x 100 directions + 12 b0 = 512 volumes -> 6: exact against the numpy statements, which write the averages into a view
    of the image they go on reading.  With the b0 volumes first no group reads a replaced volume (planar: streaming kernels); with
    the shells first every later group does, in both orders, and the tile is overwritten in place like the view"""
    from amico_amd import prep
    from oracle import signal_np
    sc = _sandi_512(which)
    assert sc.nS == 512 and len(sc.shells) == 5
    img, mask = _fill((33, 6, 4), sc, seed=5)
    img = np.asarray(img, order=order)
    ref, mb0 = signal_np.prepare_signal(img, mask, sc.b0_idx, sc.dwi_idx, shells=sc.shells, do_directional_average=True)
    sp = prep.SignalPreparation(sc, img, mask, do_directional_average=True)
    assert ref.shape == (int((mask == 1).sum()), 6)
    _check_exact(sp, img, ref, mb0, mask, 'k_prep_stream' if order == 'F' and which != 'shells first' else 'k_prep_long')


@pytest.mark.parametrize('count', ['first', 288, 512])
@pytest.mark.parametrize('order', ['C', 'F'])
def test_groups_not_in_place(order, count):
    """a scheme whose first volume is a DWI, b0 merged: output 1 would replace a volume that later outputs read, so the outputs are made
    beside the tile, 64 at a time (288 volumes: 280 outputs = four full chunks and 24; 512: 504 = seven and 56)"""
    from amico_amd import prep
    from oracle import signal_np
    n = _first_refused('twice', True) if count == 'first' else count
    sc, img, mask = _volume(n, order, dwi_first=True)
    assert sc.b0_idx[0] == 1 and sc.dwi_idx[0] == 0
    ref, mb0 = signal_np.prepare_signal(img, mask, sc.b0_idx, sc.dwi_idx, do_merge_b0=True)
    sp = prep.SignalPreparation(sc, img, mask, do_merge_b0=True)
    _check_exact(sp, img, ref, mb0, mask, 'k_prep_long<false,false>')


@pytest.mark.parametrize('merged', [False, True])
def test_generic_strides(merged):
    """every second x of a planar image twice as long: neither the voxels nor the volumes are contiguous (the plan's layout 0)"""
    from amico_amd import prep
    from oracle import signal_np
    sc = _scheme(512)
    img, mask = _fill(SHAPE, sc, seed=7)
    big = np.zeros((2 * SHAPE[0],) + SHAPE[1:] + (512,), dtype=np.float32, order='F')
    big[::2] = img
    big[1::2] = -3.0                               # never read
    view = big[::2]
    assert view.strides[0] == 8 and view.strides[3] != 4 and not view.flags.f_contiguous
    opts = dict(do_merge_b0=True) if merged else {}
    ref, mb0 = signal_np.prepare_signal(view, mask, sc.b0_idx, sc.dwi_idx, **opts)
    sp = prep.SignalPreparation(sc, view, mask, **opts)
    _check_exact(sp, view, ref, mb0, mask, 'k_prep_long')


@pytest.mark.parametrize('f32', [True, False])
@pytest.mark.parametrize('n', [449, 512])
@pytest.mark.parametrize('order', ['F', 'C'])
def test_gather_with_directions_equals_gather_then_tensor_fit(order, n, f32):
    """amx_prep_gather_directions_device[_f32] on a long protocol against the plain gather followed by amx_dti_directions_device[_f32]:
    y and mean_b0 bit for bit, the directions within 1e-12 wherever the axis is defined"""
    import torch
    from amico_amd import prep, dti
    sc, img, mask = _volume(n, order)
    sp = prep.SignalPreparation(sc, img, mask)
    td = dti.TensorDirections.from_scheme(sc, ctx=sp.ctx)
    y_a, mb_a = _gather_device(sp, img, f32)
    d_a = torch.zeros((sp.n_vox, 3), dtype=torch.float64, device=y_a.device)
    td.fit_device(y_a.data_ptr(), sp.n_vox, d_a.data_ptr(), None, f32=f32)
    sp.ctx.sync(None)
    y_b, mb_b, d_b = _gather_device(sp, img, f32, fused_with=td)
    assert torch.equal(y_a, y_b) and torch.equal(mb_a, mb_b)
    a, b = d_a.cpu().numpy(), d_b.cpu().numpy()
    assert np.isfinite(b).all() == np.isfinite(a).all()
    yv = y_a.cpu().numpy().astype(np.float64)
    flat_row = np.ptp(np.log(np.maximum(yv, 1e-4)), axis=1) == 0.0          # (norm factor 0 -> a constant row: a zero tensor, any direction)
    ok = np.isfinite(a).all(axis=1) & ~flat_row
    assert ok.sum() > 0.9 * sp.n_vox and np.abs(a[ok] - b[ok]).max() < 1e-12


@pytest.mark.parametrize('stored', ['int16 + scaling, F', 'float32, C'])
def test_evaluation_sandi_512_volumes_without_directional_average(stored):
    """raw image 6 x 5 x 4 x 512 -> (ingest) -> prepared signals, directions, SANDI fit, volumes, predicted signal"""
    import amico_amd
    from amico_amd import prep, synthetic as S
    from oracle import oracle, signal_np
    full = S.make_sandi_scheme(ndir_per_shell=100, n_b0=12)
    K, Rs, d_in, d_isos = S.sandi_kernels(full, Rs=np.linspace(1.0, 12.0, 5) * 1e-6, d_in=np.linspace(0.25, 3.0, 5) * 1e-3,
                                          d_isos=np.linspace(0.25, 3.0, 5) * 1e-3)
    shape = (6, 5, 4)
    ys = S.sandi_signals(int(np.prod(shape)), K, full, seed=11, navg=1)
    sig = 1000.0 * ys.reshape(shape + (-1,))
    if stored.startswith('int16'):
        raw, scaling = np.asfortranarray(np.rint(sig * 8.0).astype(np.int16)), (0.125, 0.0)
        assert 0 < raw.max() < 32767
    else:
        raw, scaling = np.ascontiguousarray(sig.astype(np.float32)), None
    img = prep.to_float32(raw, prep.check_scaling(scaling))
    mask = np.ones(shape, dtype=np.uint8)
    mask[0, :, :] = 0
    mask[3, 2, 1] = 0
    sel = mask == 1
    ae = amico_amd.Evaluation()
    ae.set_config('doComputeNRMSE', True)
    ae.set_config('doSavePredictedSignal', True)
    ae.set_data(raw, full, mask, scaling=scaling)
    assert ae.scheme.nS == 512
    ae.set_model('SANDI')
    ae.set_kernels(S.sandi_kernels(ae.scheme, Rs=Rs, d_in=d_in, d_isos=d_isos)[0])
    res = ae.fit()
    y_ref, mean_b0 = signal_np.prepare_signal(img, mask, full.b0_idx, full.dwi_idx)
    assert np.array_equal(ae.y, y_ref)
    ref = oracle.sandi_fit(y_ref, K, Rs, d_in, d_isos, nrmse=True, return_x=True)
    assert np.abs(res['estimates'] - ref['estimates']).max() < TOL
    assert ae.RESULTS['MAPs'].shape == shape + (6,) and not ae.RESULTS['MAPs'][~sel].any()
    assert np.abs(ae.RESULTS['MAPs'][sel] - ref['estimates']).max() < 1e-5       # (float32 volume: Rsoma is in micrometres)
    assert np.allclose(ae.RESULTS['NRMSE'][sel], ref['nrmse'], atol=TOL)
    assert ae.RESULTS['DIRs'].shape == shape + (3,) and ae.DIRs.shape == (int(sel.sum()), 3)
    pred = ref['x'] @ np.asarray(K['signal'], dtype=np.float64).T
    vol = ae.RESULTS['DWI_predicted']
    assert vol.dtype == np.float32 and vol.shape == shape + (512,) and not vol[~sel].any()
    assert np.abs(res['y_est'] - pred).max() < TOL
    m = mean_b0[sel].astype(np.float64)[:, None]
    assert np.abs(vol[sel] / m - pred).max() < TOL


def test_freewater_volume_pipeline_400_volumes_equals_evaluation(htable500):
    """raw image in HBM -> FreeWater maps and directions at 400 volumes, with the directions asked of the gather (fused=True) and of
    a tensor pass of their own: both equal to Evaluation's volumes on the same image"""
    import torch
    import amico_amd
    from amico_amd import pipeline, synthetic as S
    ht = htable500['htable']
    sch = S.make_scheme(5, ((1000.0, 395),), seed=3)
    K = S.freewater_kernels(sch, htable500['dirs'])
    shape = (10, 8, 5)
    y, _ = S.freewater_signals(int(np.prod(shape)), K, ht, sch, seed=8)
    img = np.asfortranarray((y.reshape(shape + (-1,)) * 700.0).astype(np.float32))
    mask = np.random.default_rng(3).choice(np.array([0, 1, 1, 1, 2], dtype=np.uint8), size=shape)
    ae = amico_amd.Evaluation()
    ae.set_data(img, sch, mask)
    ae.set_model('FreeWater')
    ae.set_kernels(K, ht)
    ae.fit()
    for fused in (True, False):
        pl = pipeline.FreeWaterVolumePipeline(sch, img, mask, K, ht, fused=fused)
        maps, dirs = pl.run(torch.from_numpy(_flat(img).copy()).to('cuda:0'))
        assert maps.shape == shape + (2,) and maps.cpu().numpy()[mask == 1].any()
        assert np.array_equal(maps.cpu().numpy(), ae.RESULTS['MAPs']) and np.array_equal(dirs.cpu().numpy(), ae.RESULTS['DIRs']), fused


def _n_live(mask, order):
    """tiles of 64 voxels along the image's fastest axis that hold a voxel with mask == 1"""
    sel = np.moveaxis(mask == 1, 0 if order == 'F' else 2, -1)
    pad = (-sel.shape[-1]) % 64
    sel = np.pad(sel, [(0, 0), (0, 0), (0, pad)])
    return int(sel.reshape(sel.shape[0], sel.shape[1], -1, 64).any(axis=-1).sum())


@pytest.mark.parametrize('n', [99, 288])
@pytest.mark.parametrize('order', ['F', 'C'])
def test_selection_is_unchanged_where_two_tiles_fit(order, n):
    """make_scheme()'s default protocol and 288 volumes: k_prep_gather, 128 threads, the LDS and the grid of the two-tile route"""
    from amico_amd import prep, synthetic as S
    from oracle import signal_np
    sc = S.make_scheme() if n == 99 else _scheme(n)
    assert sc.nS == n
    img, mask = _fill(SHAPE, sc, seed=3)
    img = np.asarray(img, order=order)
    sp = prep.SignalPreparation(sc, img, mask)
    y, _ = sp.gather(img)
    assert np.array_equal(y, signal_np.prepare_signal(img, mask, sc.b0_idx, sc.dwi_idx)[0])
    lds = (2 * (n * 65 if order == 'F' else 64 * (n | 1)) + 9 + n + 1 + n) * 4
    grid = min(256 * min(8, LDS_MAX // lds), (_n_live(mask, order) + 1) // 2)
    assert sp._plan.last_launch() == ('k_prep_gather<true,true>' if order == 'F' else 'k_prep_gather<true,false>', grid, 128, lds)
    # grouped, in place (interleaved) and the streaming kernel (planar)
    sp = prep.SignalPreparation(sc, img, mask, do_merge_b0=True)
    sp.gather(img)
    name, _, block, lds_m = sp._plan.last_launch()
    if order == 'F':
        assert name.startswith('k_prep_stream') and block == 256 and lds_m == (9 + n - 8 + 1 + n) * 4
    else:
        assert (name, block, lds_m) == ('k_prep_gather<false,false>', 128, (2 * 64 * (n | 1) + 9 + n - 8 + 1 + n) * 4)


def test_513_volumes_are_refused():
    """beyond the fits' limit the refusal stays: on the host, before any launch"""
    from amico_amd import prep, synthetic as S
    sc = S.make_scheme(n_b0=9, shells=((700.0, 30), (2000.0, 474)), seed=0)
    assert sc.nS == 513
    img = np.ones((4, 3, 2, 513), dtype=np.float32)
    for order in ('F', 'C'):
        sp = prep.SignalPreparation(sc, np.asarray(img, order=order), np.ones((4, 3, 2)))
        with pytest.raises(ValueError, match='scheme too long for the LDS tile'):
            sp.gather(np.asarray(img, order=order))
