"""Golden vectors for the WLS and NLLS tensor fits (DTI_fit_method, core.py:419-420, 436).

The 224 voxels of dti_fixture.npz (160 noisy NODDI voxels + 64 noise-free single-tensor voxels).  The expected
parameters come from routes that share no code with tests/dti_methods_np.py or the HIP kernels:
  WLS   scipy.linalg.lstsq (LAPACK gelsd) on the weighted system, the weights from a gelsd OLS fit
  NLLS  scipy.optimize.least_squares (trust-region reflective, finite tolerances at fp64 noise) from the OLS parameters
Run:  python tests/golden/make_dti_methods_fixture.py
"""
import os
import numpy as np
import scipy.linalg as sl
import scipy.optimize as opt

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    f = np.load(os.path.join(HERE, 'dti_fixture.npz'))
    scheme, y = f['scheme'], f['y']
    b, g = scheme[:, 3], scheme[:, :3]
    B = -np.column_stack([b * g[:, 0] ** 2, 2 * b * g[:, 0] * g[:, 1], b * g[:, 1] ** 2, 2 * b * g[:, 0] * g[:, 2],
                          2 * b * g[:, 1] * g[:, 2], b * g[:, 2] ** 2, np.ones_like(b)])
    s = np.maximum(y, 1e-4)
    ls = np.log(s)
    p_ols = sl.lstsq(B, ls.T, lapack_driver='gelsd')[0].T
    p_wls = np.zeros_like(p_ols)
    p_nlls = np.zeros_like(p_ols)
    for i in range(len(y)):
        w = np.exp(B @ p_ols[i])
        p_wls[i] = sl.lstsq(B * w[:, None], w * ls[i], lapack_driver='gelsd')[0]
        r = opt.least_squares(lambda p: s[i] - np.exp(B @ p), p_ols[i], jac=lambda p: -np.exp(B @ p)[:, None] * B,
                              method='trf', x_scale='jac', ftol=1e-15, xtol=1e-15, gtol=1e-15, max_nfev=2000)
        p_nlls[i] = r.x
    np.savez_compressed(os.path.join(HERE, 'dti_methods_fixture.npz'), p_wls=p_wls, p_nlls=p_nlls)
    print('dti_methods_fixture.npz:', p_wls.shape)


if __name__ == '__main__':
    main()
