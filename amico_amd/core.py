"""``Evaluation`` with the fields ``model.fit(evaluation)`` reads (amico/core.py:42-104, 407-498): ``y``,
``DIRs``, ``htable``, ``KERNELS``, ``nthreads``, ``get_config`` -- and the caller contract around the hot path for
in-memory volumes, every per-voxel step on the GPU:

  set_data   ~ load_data's preprocessing inputs (core.py:201-268): raw image (float32, or as it is stored + the NIfTI scaling), scheme, mask
  fit        an image kept in its stored dtype -> float32 in HBM (core.py:136), the scan below in the same kernel (amx_prep_ingest);
             NaN / Inf scan of the raw image, replacement with replace_bad_voxels (core.py:152-158)    (amx_prep_sanitize);
             CONFIG['bad_samples_raw'] = samples found; the same for ``y`` after the gather (core.py:270-276) (amx_sanitize),
             CONFIG['bad_samples_preprocessed']
             with doEstimateNoise: SNR and sigma from the spread of the b0 repeats (amx_prep_noise_b0, amx_nanmedian; not the reference's),
             or with doEstimateNoise = 'MPPCA' a sigma per voxel from its local patch (amx_prep_noise_mppca);
             with doDenoise the image denoised by that patch PCA, which everything below then reads (amx_prep_noise_mppca_denoise);
             with doUnring the Gibbs ringing of every slice removed by local sub-voxel shifts, behind the denoising (amx_prep_unring);
             Rician debias of the image when doDebiasSignal is set (core.py:201-206) (amx_prep_debias);
             CONFIG['debias_unconverged'] = samples that reached the root search's trip cap
             b0 normalisation / b0 merge / shell average + mask gather + clip  -> ``y``      (amx_prep_gather)
             principal directions from the tensor fit (DTI_fit_method)          -> ``DIRs``   (amx_dti_directions)
             with doSaveTensorMaps: the same fit's eigenvalues, FA, MD, AD, RD   -> ``DTI_evals``, ``DTI_MAPs`` (amx_dti_fit)
             model.fit(self)                                                    -> maps       (amx_*_fit)
             scatter into float32 volumes (core.py:472-498)                     -> ``RESULTS`` (amx_prep_scatter)

NIfTI / scheme-file I/O stays out of scope.
"""
import inspect
import time
import warnings
from os import cpu_count
import numpy as np
from . import models as _models
from . import _capi
from . import prep as _prep
from . import dti as _dti
from . import bootstrap as _bootstrap
from . import noise as _noise
from . import unring as _unring
from .synthetic import SimpleScheme


class Evaluation:
    def __init__(self, study_path='.', subject='.', output_path=None):
        self._raw = None              # the image as set_data received it, when fit() uploads it in its stored dtype
        self._raw_scaling = None
        self.niiDWI_img = None
        self.scheme = None
        self.niiMASK_img = None
        self.model = None
        self.KERNELS = None
        self._y = None
        self._DIRs = None
        self._dev = None
        self.nthreads = None
        self.RESULTS = None
        self.mean_b0s = None
        self.htable = None
        self._dirs_img = None
        self.CONFIG = {}
        self.set_config('study_path', study_path)
        self.set_config('subject', subject)
        self.set_config('OUTPUT_path', output_path)
        # defaults of core.py:82-96
        self.set_config('peaks_filename', None)
        self.set_config('doNormalizeSignal', True)
        self.set_config('doKeepb0Intact', False)
        self.set_config('doComputeRMSE', False)
        self.set_config('doComputeNRMSE', False)
        self.set_config('doSaveModulatedMaps', False)
        self.set_config('doSaveCorrectedDWI', False)
        self.set_config('doMergeB0', False)
        self.set_config('doDebiasSignal', False)
        self.set_config('DWI-SNR', None)
        self.set_config('doDirectionalAverage', False)
        self.set_config('nthreads', -1)
        self.set_config('DTI_fit_method', 'OLS')
        self.set_config('DTI_sigma', None)             # not a key of the reference: see fit()
        self.set_config('BLAS_nthreads', 1)
        self.set_config('doSaveTensorMaps', False)     # not a key of the reference: see fit()
        self.set_config('doEstimateNoise', False)      # not a key of the reference: see fit()
        self.set_config('noise_patch', 5)              # edge of the patch of doEstimateNoise = 'MPPCA': 3 | 5
        self._estimate_noise = False                   # the key as set_data() read it
        self._noise_patch = None                       # 'MPPCA': the patch edge as set_data() read it; None: the b0 repeats
        self.set_config('doDenoise', False)            # not a key of the reference: see fit()
        self.set_config('doSaveDenoisedDWI', False)
        self.set_config('doUnring', False)             # not a key of the reference: see fit()
        self.set_config('unring_axes', (0, 1))
        self.set_config('doSaveUnringedDWI', False)
        self._unring_axes = None                       # doUnring: the in-plane axes as set_data() read them; None: no unringing
        self._denoise_patch = None                     # doDenoise: the patch edge as set_data() read it; None: no denoising
        self._b0_estimate = False                      # doEstimateNoise asks for the b0 estimator (with doDenoise: it runs first)
        self._debias_estimated = False                 # doDebiasSignal without DWI-SNR: fit() fills the estimate in

    # `niiDWI_img` (core.py:136) is the raw float32 image.  When set_data kept the image in its stored dtype the float32 array is made
    # on first read, by the numpy expression the ingest kernel is held to, and cached; fit() itself never needs it
    @property
    def niiDWI_img(self):
        if self._img32 is None and self._raw is not None:
            self._img32 = _prep.to_float32(self._raw, self._raw_scaling)
        return self._img32

    @niiDWI_img.setter
    def niiDWI_img(self, value):
        self._img32 = value
        self._raw = self._raw_scaling = None              # an image assigned by the caller is the float32 image from here on

    # `y` / `DIRs` (core.py:451-458) are produced on the GPU by fit() and stay there for model.fit (self._dev); the
    # numpy arrays the reference exposes are fetched on first access
    @property
    def y(self):
        if self._y is None and self._dev is not None:
            self._y = self._dev['y'].cpu().numpy().astype(np.float64, copy=False)      # (held as float32 in HBM: core.py:451-452 widen)
        return self._y

    @y.setter
    def y(self, value):
        self._y = value
        self._dev = None

    @property
    def DIRs(self):
        if self._DIRs is None and self._dev is not None and self._dev.get('dirs') is not None:
            self._DIRs = self._dev['dirs'].cpu().numpy()
        return self._DIRs

    @DIRs.setter
    def DIRs(self, value):
        self._DIRs = value
        if self._dev is not None:
            self._dev.pop('dirs', None)       # directions assigned by the caller replace the ones held in HBM

    def set_config(self, key, value):
        self.CONFIG[key] = value

    def get_config(self, key):
        return self.CONFIG.get(key)

    # ---- in-memory replacement of load_data (core.py:107-278): volumes are given directly
    def set_data(self, dwi, scheme, mask=None, directions=None, b0_min_signal=0, replace_bad_voxels=None, scaling=None):
        """dwi [X,Y,Z,nS] raw signal (C or Fortran order), mask [X,Y,Z], directions [X,Y,Z,3] (optional peaks,
        core.py:438-447: when absent they come from the tensor fit).  The options doDebiasSignal / DWI-SNR /
        doNormalizeSignal / doMergeB0 / doDirectionalAverage are read here, like load_data reads them.
        With doDebiasSignal the image is debiased in HBM inside fit(): `niiDWI_img` keeps the RAW image (the reference's load_data
        replaces it with the debiased one); fit() leaves CONFIG['debias_unconverged'], the number of samples whose root search
        reached its trip cap (0 on every signal tried; a warning is raised otherwise).
        replace_bad_voxels (core.py:122-123): value that takes the place of NaN and Inf samples; None (the default) = refuse them.
        fit() scans the image in HBM before any other kernel reads it (core.py:152-158) and the prepared signals `y` after the
        gather (core.py:270-276); it leaves the counts in CONFIG['bad_samples_raw'] / ['bad_samples_preprocessed'], and a count
        that is not 0 raises the reference's RuntimeError (no value given) or its warning (the samples are replaced, the fit goes
        on).  Replacement happens in HBM only: `niiDWI_img` keeps the RAW image with its NaNs, as it does with the debias.
        Two deliberate differences from load_data: (1) the second check covers the rows of the masked voxels, not the whole
        pre-processed image -- nothing outside the mask reaches a result; (2) it runs after the gather's clip (core.py:452), so a
        -Inf has already become 0 like every negative sample where the reference would flag it first (-Inf can only come from
        float32 overflow in the normalisation of a negative sample).
        scaling: (scl_slope, scl_inter) of the NIfTI header when `dwi` holds the stored values; None, or a slope of None as nibabel
        reports an unscaled image, means none.  An image of dtype uint8 / int16 / uint16 / int32 / float64 (or float32 with a scaling)
        in C or Fortran order is kept as it is: fit() uploads those bytes and its first kernel makes the float32 image of
        core.py:136 in HBM -- np.float32(dwi), or np.float32(np.float64(dwi) * slope + inter) as nibabel scales -- bit for bit, and
        scans it in the same pass.  `niiDWI_img` is then made by that numpy expression when it is first read.  Any other dtype or
        layout is converted here, on the host, by the same expression.  float32 without scaling is uploaded as it is."""
        _prep.check_replace_bad_voxels(replace_bad_voxels)                       # before any context is made or anything uploaded
        scaling = _prep.check_scaling(scaling)
        self.set_config('replace_bad_voxels', replace_bad_voxels)               # core.py:134
        estimate = bool(self.get_config('doEstimateNoise'))
        noise_patch = None
        if _noise.is_mppca(self.get_config('doEstimateNoise')):
            noise_patch = _noise.check_patch(self.get_config('noise_patch'))     # (ValueError; Marchenko-Pastur needs no b0 repeat)
        elif estimate:
            _noise.check_b0_count(scheme.b0_count)                               # (RuntimeError naming the key, before anything is uploaded)
        b0_estimate = estimate and noise_patch is None
        denoise_patch = None
        if _noise.is_denoise(self.get_config('doDenoise')):                      # (ValueError for anything but 'MPPCA' / True / False)
            denoise_patch = _noise.check_patch(self.get_config('noise_patch'))
            estimate = True                                                      # the denoising launch delivers an estimate as well
        unring_axes = None
        if _unring.is_unring(self.get_config('doUnring')):                       # (ValueError for anything but 'kellner' / True / False)
            unring_axes = _unring.check_axes(self.get_config('unring_axes'))
        debias_snr = None
        if self.get_config('doDebiasSignal'):                                    # core.py:201-206, before anything touches the GPU
            debias_snr = self.get_config('DWI-SNR')
            if debias_snr is None and not estimate:
                raise RuntimeError('Set noise variance for debiasing (eg. ae.set_config(\'RicianNoiseSigma\', sigma))')   # core.py:205
            if scheme.b0_count == 0:
                raise RuntimeError('No b0 volume to estimate the noise level from (doDebiasSignal)')   # preproc.py:30-31
            if scheme.b0_count > _prep.MAX_DEBIAS_B0:
                raise RuntimeError(f'doDebiasSignal: more than {_prep.MAX_DEBIAS_B0} b0 volumes are not supported')
        img = np.asarray(dwi)
        if img.ndim != 4:
            raise ValueError('DWI file is not a 4D image')                       # core.py:138-139
        if (img.dtype != np.float32 or scaling is not None) and _prep.streamable(img):
            self.niiDWI_img = None
            self._raw, self._raw_scaling = img, scaling                          # as stored: no float32 copy on the host
        else:
            self.niiDWI_img = _prep.to_float32(img, scaling)                     # core.py:136
            if any(st % 4 or st <= 0 for st in self.niiDWI_img.strides):
                self.niiDWI_img = np.ascontiguousarray(self.niiDWI_img)
            img = self.niiDWI_img
        self.set_config('dim', img.shape[:3])
        self.set_config('b0_min_signal', b0_min_signal)
        if scheme.nS != img.shape[3]:
            raise ValueError('Scheme does not match with DWI data')
        if noise_patch is not None or denoise_patch is not None:
            # (RuntimeError naming the key, before anything is uploaded)
            _noise.check_patch_fits(img.shape[:3], noise_patch if noise_patch is not None else denoise_patch)
        if unring_axes is not None:
            _unring.check_extents(img.shape[:3], unring_axes)                    # (RuntimeError naming the key and the limit)
        self.niiMASK_img = np.ones(img.shape[:3], dtype=np.uint8) if mask is None \
            else np.asarray(mask, dtype=np.uint8)
        if self.niiMASK_img.shape != img.shape[:3]:
            raise ValueError('MASK geometry does not match with DWI data')
        if directions is not None and (np.ndim(directions) != 4 or np.shape(directions)[:3] != self.niiMASK_img.shape
                                       or np.shape(directions)[3] < 3):
            raise ValueError('PEAKS geometry does not match with DWI data')      # core.py:444-445
        # a peaks file holds 3*npeaks values per voxel: the fit uses the first peak
        self._dirs_img = None if directions is None else np.ascontiguousarray(np.asarray(directions, dtype=np.float32)[..., :3])   # core.py:442
        self._raw_scheme = scheme
        self._prep = _prep.SignalPreparation(
            scheme, img, self.niiMASK_img, do_normalize=self.get_config('doNormalizeSignal'),
            do_merge_b0=self.get_config('doMergeB0'), do_directional_average=self.get_config('doDirectionalAverage'),
            b0_min_signal=b0_min_signal, debias_snr=debias_snr, replace_bad_voxels=replace_bad_voxels,
            scaling=scaling if self._raw is not None else None)
        self._estimate_noise = estimate
        self._noise_patch = noise_patch
        self._denoise_patch = denoise_patch
        self._unring_axes = unring_axes
        self._b0_estimate = b0_estimate
        self._debias_estimated = bool(self.get_config('doDebiasSignal')) and debias_snr is None      # (only with the key: see above)
        if self._debias_estimated:
            self._prep._plan.set_debias_mask(self.niiMASK_img)                   # the SNR comes in fit(); the mask is known now
        # the scheme the model sees: one row per shell after the directional average (core.py:254-255)
        self.scheme = SimpleScheme(_prep.directional_average_table(scheme), scheme.b0_thr) \
            if self.get_config('doDirectionalAverage') else scheme

    def set_model(self, model_name):
        if not hasattr(_models, model_name):
            raise ValueError(f'Model "{model_name}" not recognized')
        self.model = getattr(_models, model_name)()
        self.set_solver()

    def set_solver(self, **params):
        if self.model is None:
            raise RuntimeError('Model not set; call "set_model()" method first')
        allowed = list(inspect.signature(self.model.set_solver).parameters)
        params_new = {k: v for k, v in params.items() if k in allowed}     # core.py:314-322
        self.model.set_solver(**params_new)
        self.set_config('solver_params', params_new)

    def set_kernels(self, kernels, htable=None):
        """stands in for generate_kernels()/load_kernels() (core.py:328-404)"""
        self.KERNELS = kernels
        self.htable = None if htable is None else np.ascontiguousarray(htable, dtype=np.int16)
        if self.model is not None:
            self.model.scheme = self.scheme

    def generate_kernels(self, lut_dirs, out_path=None, lmax=12):
        """core.py:328-372 `generate_kernels`: response functions of the model on the high-resolution scheme (500 directions
        per shell) -> SH coefficients rotated to every LUT orientation.  Writes `A_###.npy` under `out_path` when given and
        returns the list of arrays (what `load_kernels` takes as `in_path`).  `lut_dirs` [ndirs, 3]: the LUT orientations."""
        from . import lut as _lut
        if self.model is None:
            raise RuntimeError('Model not set; call "set_model()" method first')
        if self.scheme is None:
            raise RuntimeError('Scheme not loaded; call "set_data()" first')
        t = time.time()
        self.model.scheme = self.scheme
        lut_dirs = np.asarray(lut_dirs, dtype=np.float64)
        aux = _lut.aux_matrices(lmax, lut_dirs)
        idx_in, idx_out = _lut.aux_structures_generate(self.scheme, lmax)
        if out_path is not None:
            import os
            os.makedirs(out_path, exist_ok=True)
        lms = self.model.generate(out_path, aux, idx_in, idx_out, len(lut_dirs))
        self.set_config('generate_kernels_time', time.time() - t)
        return lms

    def load_kernels(self, in_path, lut_dirs, lmax=12):
        """core.py:374-404 `load_kernels`: resample the rotated SH coefficients (folder of A_###.npy files written by
        generate_kernels, or the list of arrays) to this subject's scheme -- one GEMM on the GPU -- and set KERNELS /
        htable.  `lut_dirs` [ndirs, 3]: the LUT orientations (amico/directions/ndirs=*.bin in the reference)."""
        from . import lut as _lut
        from .synthetic import build_htable
        if self.model is None:
            raise RuntimeError('Model not set; call "set_model()" method first')
        if self.scheme is None:
            raise RuntimeError('Scheme not loaded; call "set_data()" first')
        t = time.time()
        self.model.scheme = self.scheme
        idx_out, ylm_out = _lut.aux_structures_resample(self.scheme, lmax)
        self.KERNELS = self.model.resample(in_path, idx_out, ylm_out, self.get_config('doMergeB0'), len(lut_dirs))
        self.htable = build_htable(np.asarray(lut_dirs, dtype=np.float64))
        self.set_config('ndirs', len(lut_dirs))
        self.set_config('lmax', lmax)
        self.set_config('load_kernels_time', time.time() - t)

    def fit(self):
        """The chain of the module docstring.  Config keys that are not the reference's:

        doSavePredictedSignal   RESULTS['DWI_predicted'], results['y_est'].
        bootstrap_samples       B in 2 .. 10 000 (None or 0: off), with bootstrap_seed (default 0): the wild (residual) bootstrap of the
            maps, B refits per voxel on the GPU (amico_amd.bootstrap).  RESULTS['MAPs_std'] and RESULTS['MAPs_boot_mean'],
            float32 [X, Y, Z, n_maps], zero outside the mask: standard deviation (ddof = 1) and mean of the maps over the replicates;
            results['estimates_std'] / ['estimates_boot_mean'] float64 [n, n_maps].  The replicates keep the original fit's
            directions (the tensor fit is not repeated: the uncertainty is conditional on the direction); RESULTS['MAPs'] is what the
            fit without the key gives, bit for bit.  NODDI, FreeWater and CylinderZeppelinBall; SANDI, several devices and an assigned
            `y` raise NotImplementedError, a bad value ValueError, before anything is uploaded.  A progress_callback sees the ticks
            of every replicate's fit.
        DTI_sigma               (default None) the noise level of DTI_fit_method 'RT' | 'RESTORE' | 'restore', one finite number > 0 in the
            units of the prepared signal `y` (dti.TensorDirections; the reference passes dipy none and fails there).  Unset, it is
            1 / DWI-SNR when DWI-SNR is set, doNormalizeSignal is on and the scheme has b0 volumes (the signals are divided by their
            b0 mean, so sigma = b0 / SNR becomes 1 / SNR); with neither the robust names raise NotImplementedError where the tensor
            fit would run, as they always have.  A bad value raises ValueError before anything is uploaded.  With doMergeB0 the
            one sigma applies to the merged b0 as well, as dipy would do with that table.  get_config('dti_robust') holds the four
            counters of `TensorDirections.last_robust` after the fit; with doSaveTensorMaps RESULTS['DTI_outliers'] float32 [X, Y, Z]
            is the number of samples left out per voxel (zero outside the mask), and Free-Water's second tensor fit on the corrected
            rows is robust too and leaves RESULTS['DTI_outliers_corrected'].  The volume pipelines (pipeline.py) do not take it.
        doEstimateNoise         (default False; read by set_data like the other preprocessing keys) the noise level from the spread of the
            b0 repeats (amico_amd.noise), taken in HBM directly after the ingest / scan kernel and before the debias: one
            kernel over the b0 samples of the voxels with mask == 1, two exact medians, one small wait.  It leaves
            CONFIG['DWI-SNR_estimated'], ['noise_sigma_estimated'] (image units) and ['noise_voxels'] (eligible voxels: finite b0
            samples, a positive mean and a spread; none is a RuntimeError) and RESULTS['NOISE_MAPs'] float32 [X, Y, Z, 2] = b0 mean and
            b0 sample standard deviation (ddof = 1, uncorrected), zero outside the mask and where the voxel was not eligible.  The scheme
            needs 2 to 128 b0 volumes (RuntimeError in set_data otherwise).  An explicit DWI-SNR or DTI_sigma always wins and the
            estimate is still reported.  With DWI-SNR None, doDebiasSignal no longer raises in set_data and debiases with the estimated
            SNR; a robust DTI_fit_method without DTI_sigma takes 1 / SNR_est on normalised signals (the rule above) and
            noise_sigma_estimated otherwise -- `y` is in image units then, which an SNR alone cannot be turned into.  Without the key
            every call, its order and every result and error are what they were.  The volume pipelines (pipeline.py), the host path
            SignalPreparation.gather and models.X().fit(evaluation) do not take it.
            'MPPCA' (any letter case) selects a second estimator in the same place: a sigma per voxel by Marchenko-Pastur PCA of the voxel's
            patch of edge noise_patch (3 | 5, default 5; anything else is a ValueError in set_data) over all volumes (amico_amd.noise,
            DESIGN 7n).  It needs no b0 repeat -- set_data drops the 2-b0 minimum and instead raises RuntimeError when an axis of the
            volume is shorter than the patch; doDebiasSignal still needs a b0 volume, by its own check.  noise_sigma_estimated is the median
            of the sigma map and DWI-SNR_estimated the median of b0 mean / sigma over the eligible voxels (half of the patch inside the
            mask, finite samples; no chi-square factor), CONFIG['noise_method'] = 'MPPCA', and RESULTS['NOISE_MAPs'] is float32
            [X, Y, Z, 3] = b0 mean, sigma, number of signal components.  The estimates feed the debias and the robust fit by the rules
            above; where one of them needs the SNR and there is none (no voxel with a positive b0 mean) fit() raises before the debias.
            sigma is a few percent low on small patches.  Every other value of the key behaves as it always has.
        doDenoise               (default False; 'MPPCA' in any letter case or True; anything else is a ValueError in set_data) the image
            denoised by that Marchenko-Pastur PCA (amico_amd.noise.denoise_mppca_device): one k_mppca_denoise launch where the
            estimators run -- after the ingest / scan kernel, before the debias -- gives every voxel of the mask that has a patch the
            centre column of its patch's best approximation of rank n_signal; a voxel without one is passed through.  Debias, mean_b0,
            gather, directions, fit, corrected and predicted DWI all read the denoised image; `niiDWI_img` keeps the RAW one.  noise_patch
            is the estimator's key (an axis shorter than it: the same RuntimeError in set_data).  The launch delivers the 'MPPCA' estimate
            too, bit for bit: with doEstimateNoise unset or 'MPPCA' the CONFIG keys and RESULTS['NOISE_MAPs'] above are set and feed the
            debias and the robust fit by the rules above, with no second launch; with doEstimateNoise = True the b0 estimator runs on the
            raw image first.  It leaves CONFIG['denoise_voxels'] / ['denoise_passed_through'], and with doSaveDenoisedDWI
            RESULTS['DWI_denoised'] float32 [X, Y, Z, nS] in image units (before the debias).  No voxel with a patch at all is the
            RuntimeError of 'MPPCA'.  The volume pipelines (pipeline.py), SignalPreparation.gather and models.X().fit(evaluation) do not
            take it.
        doUnring                (default False; 'kellner' in any letter case or True; anything else is a ValueError in set_data) the Gibbs
            ringing of every slice removed by local sub-voxel shifts (Kellner et al. 2016; amico_amd.unring.unring_device):
            one launch behind the denoising block and before the debias, on the slices along unring_axes (default (0, 1): two different
            axes out of 0, 1, 2; each extent 8 to 256, anything else is a RuntimeError in set_data).  The mask plays no part; a slice
            with a NaN / Inf sample is passed through.  Debias, mean_b0, gather, directions, fit, corrected and predicted DWI all read
            the unringed image; `niiDWI_img` keeps the RAW one.  The noise estimators run before it, on the image they always saw.  It
            leaves CONFIG['unring_slices'] / ['unring_passed_through'], and with doSaveUnringedDWI RESULTS['DWI_unringed'] float32
            [X, Y, Z, nS] in image units (before the debias).  The volume pipelines (pipeline.py), SignalPreparation.gather and
            models.X().fit(evaluation) do not take it.
        doSaveTensorMaps       (default False) the tensor fit that gives `DIRs` also leaves RESULTS['DTI_MAPs'] float32 [X, Y, Z, 4] =
            FA, MD, AD, RD and RESULTS['DTI_evals'] float32 [X, Y, Z, 3] (descending, clipped at dipy's min_diffusivity), zero outside
            the mask: `dti.TensorDirections.fit_maps` of `y`, with DTI_fit_method and the table doMergeB0 gives.  The fit runs as
            two kernels, the gather and then the tensor pass, for every method -- here that is the route of always; in the volume
            pipelines (pipeline.py, tensor_maps=True) it means that the OLS fit no longer rides on the fused gather.  With
            `directions` given to set_data the tensor pass runs for the maps only and `DIRs` stay the caller's.  'RT' / 'RESTORE'
            without a sigma raise NotImplementedError as they do whenever a tensor fit would run; doDirectionalAverage leaves no gradient
            directions to fit a tensor to and raises ValueError before anything is uploaded.
            Free-Water: also RESULTS['DTI_MAPs_corrected'] / ['DTI_evals_corrected'], the same fit on the free-water-corrected rows
            (results['y_corrected'], made in HBM from the fit's isotropic coefficients; doSaveCorrectedDWI need not be set;
            min_signal clips what the correction left non-positive, as for any signal)."""
        tensor_maps = bool(self.get_config('doSaveTensorMaps'))
        # (a contradiction in the configuration itself: said first, before a context is made or anything is uploaded)
        if tensor_maps and self.get_config('doDirectionalAverage'):
            raise ValueError('doSaveTensorMaps needs the gradient directions: with doDirectionalAverage the signal is one value per '
                             'shell and there is no tensor to fit')
        if self._raw is None and self._img32 is None:
            raise RuntimeError('Data not loaded; call "set_data()" first')
        if self.model is None:
            raise RuntimeError('Model not set; call "set_model()" first')
        if self.KERNELS is None:
            raise RuntimeError('Response functions not set; call "set_kernels()" first')
        if self.KERNELS['model'] != self.model.id:
            raise RuntimeError('Response functions were not created with the same model')
        _dti.check_fit_method(self.get_config('DTI_fit_method'))     # core.py:419-420: before anything is uploaded
        dti_sigma = None
        normalized = False
        if self.get_config('DTI_fit_method') in _dti.ROBUST_METHODS:
            normalized = bool(self.get_config('doNormalizeSignal')) and self.scheme.b0_count > 0
            # (ValueError for a bad DTI_sigma / DWI-SNR; None leaves the refusal to where the tensor fit would run -- or, with
            #  doEstimateNoise, the choice to the estimate, once it is there)
            dti_sigma = _dti.resolve_sigma(self.get_config('DTI_fit_method'), self.get_config('DTI_sigma'), self.get_config('DWI-SNR'),
                                           normalized)
        if tensor_maps and len(_models.get_contexts()) > 1:
            raise NotImplementedError('doSaveTensorMaps is not built for several devices (set_devices)')
        if self.get_config('doSavePredictedSignal') and len(_models.get_contexts()) > 1:
            raise NotImplementedError('doSavePredictedSignal is not built for several devices (set_devices)')
        boot = _bootstrap.config(self)                                # (ValueError for a bad bootstrap_samples / bootstrap_seed)
        if boot is not None and self.model.id == 'SANDI':
            raise NotImplementedError(_bootstrap.REFUSE_SANDI)
        if boot is not None and len(_models.get_contexts()) > 1:
            raise NotImplementedError('bootstrap_samples is not built for several devices (set_devices)')
        nt = self.get_config('nthreads')
        self.nthreads = nt if nt > 0 else cpu_count()
        self.model.scheme = self.scheme
        sel = self.niiMASK_img == 1                                   # core.py:451 (== 1, not nonzero)
        import torch                                                  # device buffers only
        dev = torch.device('cuda', torch.cuda.current_device())
        ctx, plan = self._prep.ctx, self._prep._plan
        t = time.time()
        # ---- raw image -> HBM once; everything up to the map volumes stays there (one stream, default)
        raw = self._raw
        shape3 = self.niiMASK_img.shape
        n = self._prep.n_vox
        # core.py:152-158: the first kernel of the chain; its count comes home before anything else is enqueued (one small wait), so
        # that nothing downstream ever reads a NaN / Inf image.  A refusal leaves RESULTS and the device state as they were.
        bad_value = self.get_config('replace_bad_voxels')
        if raw is not None:
            # the bytes as they are stored cross the link; core.py:136 and the scan are one kernel, and no separate scan follows
            d_raw = torch.from_numpy(plan._raw_buffer(raw).view(np.uint8)).to(dev)
            d_img = torch.empty(plan.extent, dtype=torch.float32, device=dev)
            plan.ingest_device(d_raw.data_ptr(), raw.dtype, d_img.data_ptr(), self._raw_scaling, bad_value)
        else:
            img = self._img32
            d_img = torch.from_numpy(np.lib.stride_tricks.as_strided(img, shape=(plan.extent,), strides=(4,))).to(dev)
            plan.sanitize_device(d_img.data_ptr(), bad_value)
        self.set_config('bad_samples_raw', ctx.sanitize_last())
        d_raw = None
        _prep.refuse_or_warn(self.get_config('bad_samples_raw'), bad_value, _prep.BAD_RAW)
        debias_snr = self._prep.debias_snr
        d_noise = None
        self.CONFIG.pop('noise_method', None)                     # (set below by 'MPPCA' only: an earlier fit()'s does not linger)
        self.CONFIG.pop('denoise_voxels', None)                   # (doDenoise only)
        self.CONFIG.pop('denoise_passed_through', None)
        self.CONFIG.pop('unring_slices', None)                    # (doUnring only)
        self.CONFIG.pop('unring_passed_through', None)
        den = None
        # doDenoise with doEstimateNoise = True: the b0 estimator below on the raw image as always, the denoising launch after it
        b0_estimate = self._b0_estimate
        if self._estimate_noise:
            # doEstimateNoise: on the raw float32 image, before the debias changes it -- one k_noise_b0 launch, two medians, and one
            # small wait like the scan count's above.  An explicit DWI-SNR / DTI_sigma wins; the estimate is reported either way.
            # 'MPPCA': one k_mppca launch in the place of k_noise_b0 -- a sigma per voxel from its patch, all volumes, no b0 repeat needed
            # doDenoise: one k_mppca_denoise launch in that place delivers the same estimate, bit for bit, and the denoised image
            mppca = self._noise_patch is not None or (self._denoise_patch is not None and not b0_estimate)
            if self._denoise_patch is not None and not b0_estimate:
                noise = den = _noise.denoise_mppca_device(plan, d_img.data_ptr(), self._denoise_patch)
            else:
                noise = _noise.estimate_mppca_device(plan, d_img.data_ptr(), self._noise_patch) if mppca \
                    else _noise.estimate_device(plan, d_img.data_ptr())
            self.set_config('DWI-SNR_estimated', noise['snr'])
            self.set_config('noise_sigma_estimated', noise['sigma'])
            self.set_config('noise_voxels', noise['voxels'])
            if mppca:
                self.set_config('noise_method', _noise.MPPCA)
            if noise['voxels'] == 0 and mppca:
                raise RuntimeError(f'doEstimateNoise: no voxel of the mask has a patch to estimate the noise from (at least half of the '
                                   f'{self._noise_patch or self._denoise_patch}^3 voxels around it inside the mask and finite samples are needed)')
            if noise['voxels'] == 0:
                raise RuntimeError('doEstimateNoise: no voxel of the mask has b0 repeats to estimate the noise from (finite samples, a '
                                   'positive mean and a spread are needed)')
            # b0 mean and sample standard deviation (ddof = 1), zero where the voxel was not eligible: scattered with the results below
            # ('MPPCA': b0 mean, sigma, signal components)
            maps = (noise['mean'], noise['sd'], noise['signal']) if mppca else (noise['mean'], noise['sd'])
            d_noise = torch.nan_to_num(torch.stack(maps, dim=1), nan=0.0).contiguous()
            needs_snr = self._debias_estimated or (self.get_config('DTI_fit_method') in _dti.ROBUST_METHODS and dti_sigma is None
                                                   and normalized)
            if mppca and needs_snr and not np.isfinite(noise['snr']):
                raise RuntimeError("doEstimateNoise: 'MPPCA' found a sigma but no DWI-SNR (no voxel with a positive b0 mean): set DWI-SNR "
                                   '/ DTI_sigma')
            if self._debias_estimated:
                debias_snr = noise['snr']
            if self.get_config('DTI_fit_method') in _dti.ROBUST_METHODS and dti_sigma is None:
                # resolve_sigma's rule with the estimate in DWI-SNR's place: 1 / SNR on normalised signals; otherwise y is in image units
                # and the estimate has the unit an SNR lacks
                dti_sigma = _dti.resolve_sigma(self.get_config('DTI_fit_method'), None, noise['snr'], True) if normalized \
                    else _capi.check_sigma(noise['sigma'])
        d_denoised = None
        if self._denoise_patch is not None:
            # doDenoise: every eligible voxel of the mask becomes the centre column of its patch's best approximation of rank n_signal;
            # everything below -- debias, mean_b0, gather, directions, fit, corrected and predicted DWI -- reads the denoised image
            if den is None:
                den = _noise.denoise_mppca_device(plan, d_img.data_ptr(), self._denoise_patch)
            if den['denoised'] == 0:
                raise RuntimeError(f'doEstimateNoise: no voxel of the mask has a patch to estimate the noise from (at least half of the '
                                   f'{self._denoise_patch}^3 voxels around it inside the mask and finite samples are needed)')
            self.set_config('denoise_voxels', den['denoised'])
            self.set_config('denoise_passed_through', den['passed_through'])
            d_img = den['image']
            if self.get_config('doSaveDenoisedDWI'):
                d_denoised = d_img.clone() if debias_snr is not None else d_img      # (the debias works in place)
            den = None
        d_unringed = None
        if self._unring_axes is not None:
            # doUnring: a new image (the launch never works in place); everything below reads it
            unr = _unring.unring_device(plan, d_img.data_ptr(), self._unring_axes)
            self.set_config('unring_slices', unr['slices'])
            self.set_config('unring_passed_through', unr['passed_through'])
            d_img = unr['image']
            if self.get_config('doSaveUnringedDWI'):
                d_unringed = d_img.clone() if debias_snr is not None else d_img      # (the debias works in place)
            unr = None
        if debias_snr is not None:
            # core.py:201-206: in place in HBM, float32(E) where mask != 0 and 0 elsewhere; everything below reads the debiased image
            self._prep._plan.debias_device(d_img.data_ptr(), debias_snr)
        # the prepared signals stay float32 in HBM (every value of core.py:209-268 is a float32; core.py:451-452 only widen them):
        # the tensor fit and the model fit read them in place, half the bytes of the float64 rows
        d_y = torch.empty((n, self._prep.n_out), dtype=torch.float32, device=dev)
        d_mb0 = torch.empty(n, dtype=torch.float32, device=dev)
        thr = 0.0
        if self._prep.do_normalize and self._prep.b0_min_signal != 0.0:              # core.py:217
            d_vol = torch.empty(shape3, dtype=torch.float32, device=dev)
            plan.mean_b0_device(d_img.data_ptr(), d_vol.data_ptr())
            mean_b0s = d_vol.cpu().numpy()
            thr = float(self._prep.b0_min_signal * mean_b0s[mean_b0s > 0].mean())
        plan.gather_device(d_img.data_ptr(), d_y.data_ptr(), d_mb0.data_ptr(), self._prep.do_normalize, thr)      # core.py:209-268 + 451-452
        # core.py:270-276 on the rows the fit reads (float32 overflow in the normalisation is what can make one), before the tensor fit
        _capi.sanitize_device(ctx, d_y.data_ptr(), n * self._prep.n_out, bad_value)
        self.set_config('bad_samples_preprocessed', ctx.sanitize_last())
        _prep.refuse_or_warn(self.get_config('bad_samples_preprocessed'), bad_value, _prep.BAD_PREPROCESSED)
        # precompute directions (core.py:428-458)
        d_dirs = est = d_tmaps = None
        if self.get_config('doDirectionalAverage'):
            pass
        elif self._dirs_img is not None:
            d_dirs = torch.from_numpy(np.ascontiguousarray(self._dirs_img[sel, :], dtype=np.float64)).to(dev)
        if (d_dirs is None and not self.get_config('doDirectionalAverage')) or tensor_maps:
            # (raises NotImplementedError for 'RT' / 'RESTORE' without a sigma: only here, where a tensor fit would actually run)
            est = _dti.TensorDirections.from_scheme(self._raw_scheme, do_merge_b0=self.get_config('doMergeB0'), ctx=ctx,
                                                    fit_method=self.get_config('DTI_fit_method'), sigma=dti_sigma)
            robust = dti_sigma is not None
            d_fit_dirs = None
            if d_dirs is None:
                d_fit_dirs = d_dirs = torch.empty((n, 3), dtype=torch.float64, device=dev)
            if tensor_maps:
                # doSaveTensorMaps: the kernel variant that also writes what its eigen-solve has; given directions stay the caller's
                d_tmaps = {'DTI_evals': torch.empty((n, 3), dtype=torch.float64, device=dev),
                           'DTI_MAPs': torch.empty((n, 4), dtype=torch.float64, device=dev)}
                if robust:
                    d_tmaps['DTI_outliers'] = torch.empty(n, dtype=torch.int32, device=dev)
                est.fit_device(d_y.data_ptr(), n, None if d_fit_dirs is None else d_fit_dirs.data_ptr(), f32=True,
                               d_evals=d_tmaps['DTI_evals'].data_ptr(), d_scalars=d_tmaps['DTI_MAPs'].data_ptr(),
                               d_outliers=d_tmaps['DTI_outliers'].data_ptr() if robust else None)
            else:
                est.fit_device(d_y.data_ptr(), n, d_fit_dirs.data_ptr(), f32=True)
            if robust:
                self.set_config('dti_robust', est.last_robust())
        ctx.sync()
        del d_img
        if debias_snr is not None:
            # samples whose root search reached its trip cap (none on any signal tried: include/amico_amd.h); reported, not hidden
            self.set_config('debias_unconverged', ctx.debias_last_unconverged())
            if self.get_config('debias_unconverged'):
                warnings.warn(f"Rician debias: {self.get_config('debias_unconverged')} samples did not converge")
        self._y, self._DIRs = None, None
        self._dev = {'y': d_y, 'dirs': d_dirs, 'mb0': d_mb0}
        self.mean_b0s = d_mb0.cpu().numpy() if self._prep.do_normalize else None
        self.set_config('dirs_precomputing_time', time.time() - t)
        t = time.time()
        # models.pyx:28-43, 981 feed a ProgressBar while the chunks are fitted; here the whole fit is enqueued at once and
        # the library reports from the stream (amx_set_progress: after each NODDI stage / at the end of the other models)
        cb = self.get_config('progress_callback')
        if callable(cb):
            ctx.set_progress(cb)
        try:
            results = self.model.fit(self)                            # reads self._dev in place
        finally:
            if callable(cb):
                ctx.sync()
                ctx.set_progress(None)
        self.set_config('fit_time', time.time() - t)
        out = self._dev.get('out', {})

        def sc(key, host_values):
            """per-voxel values -> float32 volume (core.py:472-498); from the device copy when the fit left one"""
            t_ = out.get(key)
            if t_ is None:
                return self._prep.scatter(host_values)
            k = 1 if t_.dim() == 1 else t_.shape[1]
            vol = torch.empty(shape3 + (k,), dtype=torch.float32, device=dev)
            plan.scatter_device(t_.data_ptr(), k, vol.data_ptr())
            ctx.sync()
            v = vol.cpu().numpy()
            return v[..., 0] if t_.dim() == 1 else v

        self.RESULTS = {}
        self.RESULTS['MAPs'] = sc('estimates', results['estimates'])
        if boot is not None:
            if 'estimates_std' not in results:
                raise NotImplementedError("bootstrap_samples: this model's fit() ran no bootstrap (it does not go through BaseModel._run)")
            self.RESULTS['MAPs_std'] = sc('estimates_std', results['estimates_std'])
            self.RESULTS['MAPs_boot_mean'] = sc('estimates_boot_mean', results['estimates_boot_mean'])
        if d_dirs is not None:
            out['DIRs'] = d_dirs
            self.RESULTS['DIRs'] = sc('DIRs', None)
        if d_noise is not None:
            out['NOISE_MAPs'] = d_noise
            self.RESULTS['NOISE_MAPs'] = sc('NOISE_MAPs', None)
        if d_denoised is not None:
            # image units, the shape and memory order of the image given to set_data
            self.RESULTS['DWI_denoised'] = np.lib.stride_tricks.as_strided(d_denoised.cpu().numpy(), shape=plan.shape,
                                                                           strides=tuple(4 * st for st in plan.strides))
            d_denoised = None
        if d_unringed is not None:
            self.RESULTS['DWI_unringed'] = np.lib.stride_tricks.as_strided(d_unringed.cpu().numpy(), shape=plan.shape,
                                                                           strides=tuple(4 * st for st in plan.strides))
            d_unringed = None
        if self.get_config('doComputeRMSE'):
            self.RESULTS['RMSE'] = sc('rmse', results['rmse'])
        if self.get_config('doComputeNRMSE'):
            self.RESULTS['NRMSE'] = sc('nrmse', results['nrmse'])
        if self.model.name == 'NODDI' and self.get_config('doSaveModulatedMaps'):
            self.RESULTS['MAPs_mod'] = sc('estimates_mod', results['estimates_mod'])
        if self.model.name == 'Free-Water' and self.get_config('doSaveCorrectedDWI'):
            b0_idx = self.scheme.b0_idx                               # core.py:488-498
            rescale = bool(self.get_config('doNormalizeSignal')) and self.scheme.b0_count > 0
            keep_b0 = bool(self.get_config('doKeepb0Intact')) and self.scheme.b0_count > 0
            x_iso = out.get('x_iso')
            # (amx_prep_corrected_device keeps at most 128 b0 columns -- kCorrMaxB0, like the debias kernel's limit; a scheme with more and
            #  doKeepb0Intact takes the rows results['y_corrected'] -- still the GPU kernel's -- through the host block below)
            if x_iso is not None and not (keep_b0 and self.scheme.b0_count > 128):
                # the fit left the isotropic coefficients in HBM: y, x_iso (and mean_b0) -> the float32 volume in one kernel, one copy home;
                # neither y nor the rows results['y_corrected'] come to the host (amx_prep_corrected_device)
                vol = torch.empty(shape3 + (self._prep.n_out,), dtype=torch.float32, device=dev)
                plan.corrected_device(self._dev['lut'], self._dev['y'], x_iso, vol, self._dev['mb0'] if rescale else None,
                                      b0_idx if keep_b0 else ())
                ctx.sync()
                self.RESULTS['DWI_corrected'] = vol.cpu().numpy()
            else:
                y_corrected = results['y_corrected']
                if rescale:
                    y_corrected = y_corrected * np.reshape(self.mean_b0s, (-1, 1))
                if keep_b0:
                    y_corrected[:, b0_idx] = self.y[:, b0_idx] * np.reshape(self.mean_b0s, (-1, 1))
                self.RESULTS['DWI_corrected'] = self._prep.scatter(y_corrected)
        if tensor_maps:
            if self.model.name == 'Free-Water':
                # the same tensor fit on the free-water-corrected rows: made in HBM from the isotropic coefficients by the kernel behind
                # results['y_corrected'], read in place by the tensor pass; they never come to the host
                x_iso = out.get('x_iso')
                if x_iso is None:
                    raise NotImplementedError("doSaveTensorMaps: this Free-Water fit left no isotropic coefficients in HBM")
                d_yc = _capi.freewater_corrected_device(ctx, self._dev['lut'], self._dev['y'], x_iso)
                for key, k in (('DTI_evals', 3), ('DTI_MAPs', 4)):
                    d_tmaps[key + '_corrected'] = torch.empty((n, k), dtype=torch.float64, device=dev)
                if 'DTI_outliers' in d_tmaps:
                    d_tmaps['DTI_outliers_corrected'] = torch.empty(n, dtype=torch.int32, device=dev)
                est.fit_device(d_yc.data_ptr(), n, None, d_evals=d_tmaps['DTI_evals_corrected'].data_ptr(),
                               d_scalars=d_tmaps['DTI_MAPs_corrected'].data_ptr(),
                               d_outliers=d_tmaps['DTI_outliers_corrected'].data_ptr() if 'DTI_outliers' in d_tmaps else None)
            for key in ('DTI_MAPs', 'DTI_evals', 'DTI_MAPs_corrected', 'DTI_evals_corrected'):
                if key in d_tmaps:
                    out[key] = d_tmaps[key]
                    self.RESULTS[key] = sc(key, None)
            for key in ('DTI_outliers', 'DTI_outliers_corrected'):
                if key in d_tmaps:
                    # (the scatter kernel moves floating-point rows: the counts, at most 512, are exact in them)
                    out[key] = d_tmaps[key].to(torch.float64)
                    self.RESULTS[key] = sc(key, None)
        if self.get_config('doSavePredictedSignal'):
            # the fit left its coefficients in HBM: dictionary, x, DIRs (and mean_b0) -> the float32 volume in one kernel, one copy home;
            # neither y nor the rows results['y_est'] come to the host (amx_prep_predicted_device)
            rescale = bool(self.get_config('doNormalizeSignal')) and self.scheme.b0_count > 0
            if 'predict' not in self._dev:
                raise NotImplementedError("doSavePredictedSignal: this model's fit() left no coefficients in HBM (it does not go through "
                                          "BaseModel._run)")
            vol = torch.empty(shape3 + (self._prep.n_out,), dtype=torch.float32, device=dev)
            p_lut, p_x, p_dirs = self._dev['predict']
            plan.predicted_device(p_lut, p_x, vol, p_dirs, self._dev['mb0'] if rescale else None)
            ctx.sync()
            self.RESULTS['DWI_predicted'] = vol.cpu().numpy()
        self._dev.pop('out', None)
        self._dev.pop('lut', None)
        self._dev.pop('predict', None)
        return results
