#!/usr/bin/env python3
"""Golden vectors for the Rician debias: the reference's `debiasRician` (amico/preproc.py, imported from /root/reference in the
build container -- pure Python, numpy + scipy) on a small noisy image, one call per SNR level.  Only inputs and outputs are
stored (tests/golden/debias_fixture.npz); nothing of the reference travels.

    python tests/golden/make_debias_fixture.py

    img        f32 [6, 6, 6, 99]   Rician-distributed samples, some set to 0; 9 b0 volumes (b0_idx)
    mask       u8  [6, 6, 6]       0, 1 and 2
    region     i8  [6, 6, 6]       index into snr_levels of the call that debiased the voxel, -1 where mask == 0
    snr_levels f64 [5]             the SNR handed to each call (a Python float, as a user's set_config('DWI-SNR', 30.0) is)
    vox        i32 [n, 3]          the masked voxels in C order; the arrays below have one row each
    ref_E      f64 [n, 99]         what the reference returned
    ref_F      f64 [n]             the functional F of tests/debias_np.py (sigma = b0 mean / SNR in float64) at ref_E
    ref_F_reported f64 [n]         scipy's `fun` of the same run.  NOT comparable with F to better than ~1e-7 relative: numpy keeps
                                   `b0 / SNR`, its square and sqrt(pi sig2 / 2) in float32 (a float32 scalar with Python floats), so the
                                   run minimised a functional whose sigma is rounded to float32 -- twice, inconsistently
    exact_E    f64 [n, 99]         the exact minimiser: scipy.optimize.brentq on scipy's `ive`, sample by sample (tests/debias_np.py)
    gap        f64 [5]             per SNR level, max |ref_E - exact_E| / b0 mean: how far the reference stops from its minimum
"""
import os
import sys
import types

import numpy as np
import scipy.optimize

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..'))
import debias_np as D                          # noqa: E402

m = types.ModuleType('amico')
m.__path__ = ['/root/reference/amico']
sys.modules['amico'] = m
util = types.ModuleType('amico.util')
util.get_verbose = lambda: 0
sys.modules['amico.util'] = util


class ProgressBar:
    def __init__(self, **kw):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False

    def update(self):
        pass


dl, ui = types.ModuleType('dicelib'), types.ModuleType('dicelib.ui')
ui.ProgressBar = ProgressBar
sys.modules['dicelib'], sys.modules['dicelib.ui'] = dl, ui
from amico import preproc as ref               # noqa: E402

# the reference keeps only scipy's `x`; its objective value is taken from the same call
_minimize, FUNS = ref.minimize, []


def minimize(*a, **kw):
    r = _minimize(*a, **kw)
    FUNS.append(float(r.fun))
    return r


ref.minimize = minimize

rng = np.random.default_rng(20261016)
shape, nS = (6, 6, 6), 99
b0_idx = np.arange(0, nS, 11, dtype=np.int32)                        # 9 b0 volumes
snr_levels = np.array([5.0, 10.0, 20.0, 30.0, 50.0])
mask = rng.choice(np.array([0, 1, 1, 1, 1, 1, 2, 2, 2, 2], dtype=np.uint8), size=shape)
region = np.where(mask != 0, rng.integers(0, len(snr_levels), size=shape), -1).astype(np.int8)
bval = np.where(np.isin(np.arange(nS), b0_idx), 0.0, rng.choice([700.0, 2000.0, 3000.0], size=nS))
img = np.zeros(shape + (nS,), dtype=np.float32)
for idx in np.ndindex(*shape):
    amp = 400.0 + 1200.0 * rng.random()
    snr = snr_levels[region[idx]] if region[idx] >= 0 else 20.0
    clean = amp * (0.15 * np.exp(-bval * 3.0e-3) + 0.85 * np.exp(-bval * rng.uniform(0.1e-3, 1.7e-3, size=nS)))
    sig = amp / snr
    img[idx] = np.abs(clean + sig * rng.standard_normal(nS) + 1j * sig * rng.standard_normal(nS)).astype(np.float32)
    img[idx][rng.random(nS) < 0.01] = 0.0                            # some samples at 0
img[..., b0_idx] = np.maximum(img[..., b0_idx], 1.0)

scheme = types.SimpleNamespace(b0_idx=b0_idx)
vox = np.argwhere(mask != 0).astype(np.int32)
ref_vol = np.zeros(shape + (nS,))
ref_F_vol = np.zeros(shape)
for k, snr in enumerate(snr_levels):
    sub = np.where(region == k, mask, 0).astype(np.uint8)
    FUNS.clear()
    out = ref.debiasRician(img, float(snr), sub, scheme)
    ref_vol[sub != 0] = out[sub != 0]
    ref_F_vol[sub != 0] = FUNS                                        # debiasRician walks the voxels in C order, like the boolean index
    assert not out[sub == 0].any()
S = img[mask != 0]
lvl = region[mask != 0]
sigma = D.sigma_of(S, b0_idx, 1.0) / snr_levels[lvl]
exact_E = D.exact_minimiser(S, sigma)
ref_E, ref_F_reported = ref_vol[mask != 0], ref_F_vol[mask != 0]
ref_F = D.objective(ref_E, S, sigma)
b0 = sigma * snr_levels[lvl]
gap = np.array([np.max(np.abs(ref_E[lvl == k] - exact_E[lvl == k]) / b0[lvl == k, None]) for k in range(len(snr_levels))])
F_exact = D.objective(exact_E, S, sigma)
print('voxels', len(vox), 'samples at or below the floor', int((S <= D.floor_of(sigma)[:, None]).sum()))
print('gap per level', gap)
print('F(exact) <= F(ref_E) on', int((F_exact <= ref_F).sum()), 'of', len(vox), 'voxels; <= scipy\'s reported value on',
      int((F_exact <= ref_F_reported).sum()), '; F(ref_E) / F(exact) - 1 in', np.min(ref_F / F_exact - 1), np.max(ref_F / F_exact - 1))
print('largest residual of the exact minimiser above the floor',
      np.max(np.where(S > D.floor_of(sigma)[:, None], np.abs(D.mu(exact_E, sigma[:, None]) - S) / np.maximum(S, 1e-30), 0.0)))
np.savez_compressed(os.path.join(HERE, 'debias_fixture.npz'), img=img, mask=mask, region=region, snr_levels=snr_levels,
                    b0_idx=b0_idx, vox=vox, ref_E=ref_E, ref_F=ref_F, ref_F_reported=ref_F_reported, exact_E=exact_E, gap=gap)
