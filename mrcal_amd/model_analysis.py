"""Projection uncertainty: mrcal.projection_uncertainty() (mrcal/model_analysis.py:1192-1517) with the propagation on
the device (include/mrcal_amd.h, mrcal_amd_uncertainty_*; csrc/projection_uncertainty.hip).

    u = mrcal.ProjectionUncertainty(model)                 # C (k x k) computed once, on the GPU
    var  = u.evaluate(p_cam)                               # (..., 2,2)
    s    = u.evaluate(p_cam, atinfinity=True, what='worstdirection-stdev')
    var  = mrcal.projection_uncertainty(p_cam, model)      # the one-shot form

The methods are the cross-reprojection ones, "cross-reprojection-ccp" (the default) and
"cross-reprojection-rrp-Jfp". "mean-pcam" is not provided: asking for it raises.
"""
import ctypes as C
import re
import numpy as np

from ._cabi import _ptr

_known_methods = ('mean-pcam', 'cross-reprojection-ccp', 'cross-reprojection-rrp-Jfp')
_methods       = {'cross-reprojection-ccp': 0, 'cross-reprojection-rrp-Jfp': 1}
_whats         = {'covariance': 0, 'worstdirection-stdev': 1, 'rms-stdev': 2}


def worst_direction_stdev(cov):
    """The worst-direction standard deviation of (..., N,N) covariances: the sqrt of the largest eigenvalue
    (mrcal/model_analysis.py:398-489). Closed form for 2x2, sqrt for 1x1; host numpy"""
    cov = np.asarray(cov, dtype=float)
    if cov.ndim < 2:
        cov = cov.reshape((1,)*(2 - cov.ndim) + cov.shape)
    if cov.shape[-2:] == (1,1):
        return np.sqrt(cov[..., 0,0])
    if cov.shape[-2:] == (2,2):
        a = cov[..., 0,0]
        b = cov[..., 1,0]
        c = cov[..., 1,1]
        return np.sqrt((a+c)/2 + np.sqrt((a-c)*(a-c)/4 + b*b))
    if cov.shape[-1] != cov.shape[-2]:
        raise Exception(f"covariance matrices must be square. Got cov.shape = {cov.shape}")
    return np.sqrt(np.linalg.eigvalsh(cov)[..., -1])


def _check_what(what):
    if what not in _whats:
        raise Exception(f"'what' kwarg must be in {set(_whats)}, but got '{what}'")


def _inputs_of(model, method):
    """(optimization_inputs, icam_intrinsics) after every refusal of the reference that can be decided on the host"""
    if method not in _known_methods:
        raise Exception(f"Unknown uncertainty method: '{method}'. I know about {_known_methods}")
    if method == 'mean-pcam':
        raise Exception("method='mean-pcam' is not implemented here: only the cross-reprojection methods "
                        "('cross-reprojection-ccp', 'cross-reprojection-rrp-Jfp') are")
    icam_intrinsics = model.icam_intrinsics()
    optimization_inputs = model.optimization_inputs()
    if optimization_inputs is None:
        raise Exception("optimization_inputs are unavailable in this model. Uncertainty cannot be computed")
    from .cameramodel import _is_poison
    optimization_inputs = {k: v for k, v in optimization_inputs.items() if not _is_poison(v)}

    from . import _api
    Nmeasurements_boards         = _api.num_measurements_boards(**optimization_inputs)
    Nmeasurements_points         = _api.num_measurements_points(**optimization_inputs)
    Nmeasurements_regularization = _api.num_measurements_regularization(**optimization_inputs)
    Nmeasurements_all            = _api.num_measurements(**optimization_inputs)
    if Nmeasurements_boards + Nmeasurements_points + Nmeasurements_regularization != Nmeasurements_all:
        raise Exception("Some measurements other than boards, points and regularization are present. Don't know what to do")

    if re.match('cross-reprojection-rrp', method):
        def indices(name):
            v = optimization_inputs.get(name)
            return np.zeros((0,3), dtype=np.int32) if v is None or np.size(v) == 0 else np.asarray(v).reshape(-1,3)
        icice = np.concatenate((indices('indices_frame_camintrinsics_camextrinsics')[:,1:],
                                indices('indices_point_camintrinsics_camextrinsics')[:,1:]), axis=0)
        icam_extrinsics = np.unique(icice[icice[:,0] == icam_intrinsics, 1])
        if icam_extrinsics.size == 0:
            raise Exception(f"No extrinsics corresponding to {icam_intrinsics=}. I don't know what to do")
        if icam_extrinsics.size > 1:
            d = np.unique(np.diff(icam_extrinsics))
            if not (d.size == 1 and d[0] == 1):
                raise Exception("At this point I'm only supporting consecutive block of extrinsics for a given icam_intrinsics")
            if icam_extrinsics[0] < 0:
                raise Exception("Have moving camera, some poses are at the reference. This isn't supported yet")
            raise Exception("I only handle stationary cameras for now")
    return optimization_inputs, icam_intrinsics


def _declare(L):
    if getattr(L, "_mrcal_amd_uncertainty_declared", False):
        return
    vp = C.c_void_p
    L.mrcal_amd_uncertainty_create.restype  = vp
    L.mrcal_amd_uncertainty_create.argtypes = [vp, C.c_int, C.c_int, C.c_double]
    L.mrcal_amd_uncertainty_evaluate.restype  = C.c_bool
    L.mrcal_amd_uncertainty_evaluate.argtypes = [vp, vp, C.c_int, C.c_bool, C.c_int, vp]
    L.mrcal_amd_uncertainty_observed_pixel_uncertainty.restype  = C.c_double
    L.mrcal_amd_uncertainty_observed_pixel_uncertainty.argtypes = [vp]
    L.mrcal_amd_uncertainty_destroy.restype  = None
    L.mrcal_amd_uncertainty_destroy.argtypes = [vp]
    L._mrcal_amd_uncertainty_declared = True


class ProjectionUncertainty:
    """The projection uncertainty of one calibrated camera, kept resident: the k x k matrix C of
    Var(q) = sigma^2 G(p) C G(p)^T is computed once, on the GPU, from the solve the model stores
    (model.optimization_inputs(), model.icam_intrinsics(); never the model's current pose). evaluate() then costs a
    projection with gradients and a k x k quadratic form a point. One context serves atinfinity both ways"""

    def __init__(self, model, *, method='cross-reprojection-ccp', observed_pixel_uncertainty=None):
        optimization_inputs, icam_intrinsics = _inputs_of(model, method)
        from . import _lib, _api
        from .resident import Problem
        self._L = _lib.lib
        self._api = _api
        _declare(self._L)
        self.method = method
        self.handle = None
        sigma = -1.0 if observed_pixel_uncertainty is None else float(observed_pixel_uncertainty)
        if observed_pixel_uncertainty is not None and not sigma > 0.0:
            raise Exception(f"observed_pixel_uncertainty must be > 0, got {observed_pixel_uncertainty}")
        with Problem(**optimization_inputs) as problem:
            # (the regularization rows of J and K are read off the problem's Jacobian: it must be streamed)
            problem.set_jacobian_stream(True)
            self.handle = self._L.mrcal_amd_uncertainty_create(problem.handle, int(icam_intrinsics), _methods[method], sigma)
        if not self.handle:
            raise Exception("projection uncertainty failed:" + _api._last_error())
        self.observed_pixel_uncertainty = float(self._L.mrcal_amd_uncertainty_observed_pixel_uncertainty(self.handle))

    def evaluate(self, p_cam, *, atinfinity=False, what='covariance'):
        """Var(q) (..., 2,2) for what='covariance', else the standard deviation (...): the worst direction's or the
        RMS of the two. p_cam (..., 3) in the camera frame"""
        _check_what(what)
        if self.handle is None:
            raise Exception("this ProjectionUncertainty has been closed")
        p = np.asarray(p_cam, dtype=np.float64)
        if p.shape[-1:] != (3,):
            raise Exception(f"p_cam must have shape (..., 3), got {p.shape}")
        lead = p.shape[:-1]
        pf = np.ascontiguousarray(p.reshape(-1, 3))
        N = pf.shape[0]
        out = np.empty((N, 4) if what == 'covariance' else (N,), dtype=np.float64)
        if N > 0 and not self._L.mrcal_amd_uncertainty_evaluate(self.handle, _ptr(pf), N, bool(atinfinity),
                                                                _whats[what], _ptr(out)):
            raise Exception("projection uncertainty failed:" + self._api._last_error())
        if what == 'covariance':
            return out.reshape(lead + (2, 2))
        return out.reshape(lead) if lead else out[0]

    def close(self):
        if getattr(self, "handle", None):
            self._L.mrcal_amd_uncertainty_destroy(self.handle)
            self.handle = None
    def __del__(self):
        try:    self.close()
        except Exception: pass
    def __enter__(self): return self
    def __exit__(self, *a): self.close()


def projection_uncertainty(p_cam, model, *, method='cross-reprojection-ccp', atinfinity=False, what='covariance',
                           observed_pixel_uncertainty=None):
    """mrcal.projection_uncertainty() (mrcal/model_analysis.py:1192-1517): the one-shot form of
    ProjectionUncertainty(model, ...).evaluate(p_cam, ...)"""
    _check_what(what)
    with ProjectionUncertainty(model, method=method, observed_pixel_uncertainty=observed_pixel_uncertainty) as u:
        return u.evaluate(p_cam, atinfinity=atinfinity, what=what)
