"""Model analysis: the projection uncertainty and the projection differences between models.

Projection differences: mrcal.projection_diff() (mrcal/model_analysis.py:1520-1928) and the fit in its middle,
implied_Rt10__from_unprojections() (:27-395), on the device (include/mrcal_amd.h, mrcal_amd_implied_rt10,
mrcal_amd_projection_diff_*; csrc/projection_diff.hip). See the end of this file.

Projection uncertainty: mrcal.projection_uncertainty() (mrcal/model_analysis.py:1192-1517) with the propagation on
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
import sys
import numpy as np

from . import _handle
from ._cabi import _ptr
from ._handle import Handle, _failed

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


class ProjectionUncertainty(Handle):
    """The projection uncertainty of one calibrated camera, kept resident: the k x k matrix C of
    Var(q) = sigma^2 G(p) C G(p)^T is computed once, on the GPU, from the solve the model stores
    (model.optimization_inputs(), model.icam_intrinsics(); never the model's current pose). evaluate() then costs a
    projection with gradients and a k x k quadratic form a point. One context serves atinfinity both ways"""

    _destroy = "mrcal_amd_uncertainty_destroy"

    def __init__(self, model, *, method='cross-reprojection-ccp', observed_pixel_uncertainty=None):
        optimization_inputs, icam_intrinsics = _inputs_of(model, method)
        from .resident import Problem
        self.method = method
        sigma = -1.0 if observed_pixel_uncertainty is None else float(observed_pixel_uncertainty)
        if observed_pixel_uncertainty is not None and not sigma > 0.0:
            raise Exception(f"observed_pixel_uncertainty must be > 0, got {observed_pixel_uncertainty}")
        with Problem(**optimization_inputs) as problem:
            # (the regularization rows of J and K are read off the problem's Jacobian: it must be streamed)
            problem.set_jacobian_stream(True)
            self._create("projection uncertainty", "mrcal_amd_uncertainty_create", problem.handle, int(icam_intrinsics),
                         _methods[method], sigma)
        self.observed_pixel_uncertainty = float(self._function("mrcal_amd_uncertainty_observed_pixel_uncertainty")(self.handle))

    def evaluate(self, p_cam, *, atinfinity=False, what='covariance'):
        """Var(q) (..., 2,2) for what='covariance', else the standard deviation (...): the worst direction's or the
        RMS of the two. p_cam (..., 3) in the camera frame"""
        _check_what(what)
        self._open()
        p = np.asarray(p_cam, dtype=np.float64)
        if p.shape[-1:] != (3,):
            raise Exception(f"p_cam must have shape (..., 3), got {p.shape}")
        lead = p.shape[:-1]
        pf = np.ascontiguousarray(p.reshape(-1, 3))
        N = pf.shape[0]
        out = np.empty((N, 4) if what == 'covariance' else (N,), dtype=np.float64)
        if N > 0:
            self._call("projection uncertainty", "mrcal_amd_uncertainty_evaluate", _ptr(pf), N, bool(atinfinity), _whats[what],
                       _ptr(out))
        if what == 'covariance':
            return out.reshape(lead + (2, 2))
        return out.reshape(lead) if lead else out[0]


def projection_uncertainty(p_cam, model, *, method='cross-reprojection-ccp', atinfinity=False, what='covariance',
                           observed_pixel_uncertainty=None):
    """mrcal.projection_uncertainty() (mrcal/model_analysis.py:1192-1517): the one-shot form of
    ProjectionUncertainty(model, ...).evaluate(p_cam, ...)"""
    _check_what(what)
    with ProjectionUncertainty(model, method=method, observed_pixel_uncertainty=observed_pixel_uncertainty) as u:
        return u.evaluate(p_cam, atinfinity=atinfinity, what=what)


# ---------------------------------------------------------------------------------------------------------------------
# projection differences

def _Rt_from_fit(rt, atinfinity):
    """(..., 4,3) from the fitted (..., 6): at infinity the fit is a rotation, and row 3 is 0"""
    from .poseutils import R_from_r
    rt = np.asarray(rt, dtype=float)
    Rt = np.zeros(rt.shape[:-1] + (4, 3))
    Rt[..., :3, :] = R_from_r(rt[..., :3])
    if not atinfinity:
        Rt[..., 3, :] = rt[..., 3:]
    return Rt


def _implied_rt10(q0, p0, v1, weights, atinfinity, focus_center, focus_radius):
    """The fit and what it reports: (rt (6,), dict(cost, Nevaluations, Nused, status))"""
    q0 = np.asarray(q0, dtype=float)
    p0 = np.asarray(p0, dtype=float)
    v1 = np.asarray(v1, dtype=float)
    if q0.ndim < 2 or q0.shape[-1] != 2:
        raise Exception(f"q0 must have shape (Nh,Nw,2), got {q0.shape}")
    grid = q0.shape[:-1]
    if v1.shape != grid + (3,):
        raise Exception(f"v1 must have shape {grid + (3,)}, got {v1.shape}")
    if p0.shape[-1:] != (3,) or p0.shape[-1-len(grid):-1] != grid:
        raise Exception(f"p0 must have shape (...,{','.join(str(n) for n in grid)},3), got {p0.shape}")
    N = int(np.prod(grid))
    q0 = np.ascontiguousarray(q0.reshape(N, 2))
    v1 = np.ascontiguousarray(v1.reshape(N, 3))
    p0 = np.ascontiguousarray(p0.reshape(-1, N, 3))
    M = p0.shape[0]
    if weights is not None:
        weights = np.asarray(weights, dtype=float)
        if weights.size != M*N or weights.shape[-len(grid):] != grid:
            raise Exception(f"weights must have the shape of p0 less its last dimension, got {weights.shape}")
        weights = np.ascontiguousarray(weights.reshape(M, N))
    fc = np.ascontiguousarray(np.asarray(focus_center, dtype=float).reshape(2))

    L = _handle._libs()[0].lib
    rt = np.zeros(6)
    cost = C.c_double(0.0)
    Nevaluations, Nused, status = C.c_int(0), C.c_int(0), C.c_int(-1)
    ok = L.mrcal_amd_implied_rt10(_ptr(rt), C.byref(cost), C.byref(Nevaluations), C.byref(Nused), C.byref(status),
                                  _ptr(q0), _ptr(p0), _ptr(v1), _ptr(weights), M, N, bool(atinfinity), _ptr(fc),
                                  float(focus_radius))
    if not ok:
        if status.value == 2:
            raise Exception("Focus region contained too few points")
        raise _failed("implied_Rt10__from_unprojections()")
    return rt, dict(cost=cost.value, Nevaluations=Nevaluations.value, Nused=Nused.value, status=status.value)


def implied_Rt10__from_unprojections(q0, p0, v1, *, weights=None, atinfinity=True, focus_center=(0, 0), focus_radius=1.0e8):
    """mrcal.implied_Rt10__from_unprojections() (mrcal/model_analysis.py:27-395): the Rt (4,3) from camera 0 to camera 1
    that best lines up the unprojections p0 (...,Nh,Nw,3) of camera 0 with the unit vectors v1 (Nh,Nw,3) of camera 1 at
    the pixels q0 (Nh,Nw,2) inside the focus region, weighted by weights (...,Nh,Nw). Every leading dimension of p0
    takes part in the one fit. atinfinity: a rotation only (row 3 is 0), p0 are unit vectors. The reference's cost
    (Huber at (5 deg)^2), minimised on the GPU in one launch from rt = 0: the same bits on every call, and exactly the
    identity for a model against itself (csrc/projection_diff.hip)"""
    rt, _ = _implied_rt10(q0, p0, v1, weights, atinfinity, focus_center, focus_radius)
    return _Rt_from_fit(rt, atinfinity)


def _is_noncentral(lensmodel):
    # (mrcal_lensmodel_metadata(): of the models here only CAHVORE is)
    return re.match("LENSMODEL_CAHVORE_", lensmodel) is not None


class _DiffContext(Handle):
    """The gridded unprojections of two or more models, resident (mrcal_amd_projection_diff_*)"""
    _destroy = "mrcal_amd_projection_diff_destroy"

    def __init__(self, lensmodels, intrinsics_data, q0):
        _lib, _ = _handle._libs()
        self.Nmodels = len(lensmodels)
        self.grid = q0.shape[:-1]
        self.N = int(np.prod(self.grid))
        ms = [_lib.lensmodel(name) for name in lensmodels]
        arr = (type(ms[0])*self.Nmodels)(*ms)
        intr = [np.ascontiguousarray(i, dtype=np.float64) for i in intrinsics_data]
        for name, m, i in zip(lensmodels, ms, intr):
            Ni = _lib.lib.mrcal_lensmodel_num_params(C.byref(m))
            if i.shape != (Ni,):
                raise Exception(f"{name} takes {Ni} intrinsics, got an array of shape {i.shape}")
        ptrs = (C.c_void_p*self.Nmodels)(*[i.ctypes.data for i in intr])
        q = np.ascontiguousarray(q0.reshape(self.N, 2), dtype=np.float64)
        self._create("projection_diff()", "mrcal_amd_projection_diff_create", self.Nmodels, arr, ptrs, _ptr(q), self.N)

    def evaluate(self, distance, atinfinity, uncertainties, Rt10, focus_center, focus_radius):
        """(difflen (Nd,Nh,Nw), diff (Nfits,Nd,Nh,Nw,2), Rt10 (Nfits,4,3), report). Rt10 None: the fit"""
        Nfits, Nd = self.Nmodels - 1, len(distance)
        d = np.ascontiguousarray(distance, dtype=np.float64)
        fit = Rt10 is None
        Rt = np.zeros((Nfits, 4, 3)) if fit else np.ascontiguousarray(Rt10, dtype=np.float64).reshape(Nfits, 4, 3).copy()
        rt = np.zeros((Nfits, 6))
        cost = np.zeros(Nfits)
        Nevaluations, Nused, status = (np.full(Nfits, -1, dtype=np.int32) for _ in range(3))
        difflen = np.empty((Nd,) + self.grid)
        diff    = np.empty((Nfits, Nd) + self.grid + (2,))
        us = None
        if fit and uncertainties is not None:
            us = (C.c_void_p*self.Nmodels)(*[u.handle for u in uncertainties])
        fc = np.ascontiguousarray(np.asarray(focus_center, dtype=float).reshape(2))
        try:
            self._call("projection_diff()", "mrcal_amd_projection_diff_evaluate", _ptr(d), Nd, bool(atinfinity), us, fit, _ptr(fc),
                       float(focus_radius), _ptr(Rt), _ptr(rt), _ptr(cost), _ptr(Nevaluations), _ptr(Nused), _ptr(status),
                       _ptr(difflen), _ptr(diff))
        except Exception:
            if fit and (status == 2).any():
                raise Exception("Focus region contained too few points") from None
            raise
        if fit:
            # (the same conversion as implied_Rt10__from_unprojections(): the same bits; the device's own R differs from
            #  it by rounding)
            Rt = _Rt_from_fit(rt, atinfinity)
        return difflen, diff, Rt, dict(rt=rt, cost=cost, Nevaluations=Nevaluations, Nused=Nused, status=status)

    def time_fit(self, on=True):
        return self._function("mrcal_amd_projection_diff_time_fit")(self.handle, bool(on))


def projection_diff(models, *, implied_Rt10=None, gridn_width=60, gridn_height=None, intrinsics_only=False, distance=None,
                    use_uncertainties=True, focus_center=None, focus_radius=-1.):
    """mrcal.projection_diff() (mrcal/model_analysis.py:1520-1928): the difference in projection between models, on a
    grid of the imager. Returns (difflen, diff, q0, Rt10):
      difflen (gridn_height,gridn_width), with a leading len(distance) if distance is iterable: |diff|; with more than
              two models sqrt(mean_i |q_i - q0|^2) over models 1..
      diff    difflen's shape + (2,): q1 - q0, or None with more than two models
      q0      (gridn_height,gridn_width,2): the grid
      Rt10    (4,3), or (len(models)-1,4,3) with more than two models: the transformation used - implied_Rt10 as given;
              the identity if intrinsics_only; the models' own extrinsics if focus_radius == 0; otherwise the fit of
              implied_Rt10__from_unprojections() over all the distances, weighted by 1/(u0 u1)^2 of the models'
              worst-direction projection uncertainties if use_uncertainties (with a WARNING on stderr, and without
              weights, if those cannot be computed).
    distance None: infinity. focus_center None: the imager's centre. focus_radius < 0: the whole imager with
    uncertainties, min(W,H)/6 without. The grid's unprojections, the weights and the pixels stay on the GPU between
    the stages (csrc/projection_diff.hip)"""
    return _projection_diff(models, None, None, implied_Rt10=implied_Rt10, gridn_width=gridn_width, gridn_height=gridn_height,
                            intrinsics_only=intrinsics_only, distance=distance, use_uncertainties=use_uncertainties,
                            focus_center=focus_center, focus_radius=focus_radius)


def _projection_diff(models, _uncertainties, _report, *, implied_Rt10=None, gridn_width=60, gridn_height=None,
                     intrinsics_only=False, distance=None, use_uncertainties=True, focus_center=None, focus_radius=-1.):
    """projection_diff(), and for the tools: _uncertainties, ProjectionUncertainty contexts (one a model) to use instead of
    making them; _report, a dict that receives what the fit reported (rt, cost, Nevaluations, Nused, status)"""
    from .poseutils import identity_Rt, compose_Rt
    from .utils import sample_imager

    if len(models) < 2:
        raise Exception("At least 2 models are required to compute the diff")
    if len(models) > 2 and implied_Rt10 is not None:
        raise Exception("A given implied_Rt10 is currently supported ONLY if exactly 2 models are being compared")

    distance_is_iterable = True
    try:    len(distance)
    except Exception: distance_is_iterable = False
    if distance is None:
        atinfinity = True
        distance   = np.ones((1,), dtype=float)
    else:
        atinfinity = False
        distance   = np.atleast_1d(np.array(distance, dtype=float)).ravel()

    imagersizes = np.array([model.imagersize() for model in models])
    if np.linalg.norm(np.std(imagersizes, axis=-2)) != 0:
        raise Exception("The diff function needs all the imager dimensions to match. Instead got {}".format(imagersizes))
    W, H = (int(x) for x in imagersizes[0])

    lensmodels      = [model.intrinsics()[0] for model in models]
    intrinsics_data = [np.array(model.intrinsics()[1], dtype=float) for model in models]
    for i in range(len(models)):
        if _is_noncentral(lensmodels[i]) and not np.sum(intrinsics_data[i][-3:]**2) < 1e-12:
            if not atinfinity:
                raise Exception(f"Model {i} is noncentral, so I can only evaluate the diff at infinity")
            if use_uncertainties:
                raise Exception("I have a noncentral model. No usable uncertainties for those yet")
            # (the reference's special case: CAHVORE is compared with its E set to 0)
            intrinsics_data[i][-3:] = 0

    want_fit     = implied_Rt10 is None and not intrinsics_only and focus_radius != 0
    want_weights = use_uncertainties and want_fit
    if implied_Rt10 is not None:
        implied_Rt10 = np.asarray(implied_Rt10, dtype=float)
        if implied_Rt10.shape != (4, 3):
            raise Exception(f"implied_Rt10 must have shape (4,3), got {implied_Rt10.shape}")

    # everything the host can refuse has been refused: the device from here on
    uncertainties, made_here = None, []
    if want_weights:
        try:
            if _uncertainties is not None:
                uncertainties = list(_uncertainties)
                if len(uncertainties) != len(models):
                    raise Exception(f"{len(uncertainties)} uncertainty contexts for {len(models)} models")
            else:
                for model in models:
                    made_here.append(ProjectionUncertainty(model))
                uncertainties = made_here
        except Exception as e:
            print("WARNING: projection_diff() was asked to use uncertainties, but they aren't available/couldn't be "
                  f"computed. Falling back on the region-based-only logic. Caught exception: {e}", file=sys.stderr)
            for u in made_here: u.close()
            uncertainties, made_here = None, []

    try:
        if focus_center is None:
            focus_center = ((W - 1.)/2., (H - 1.)/2.)
        if focus_radius < 0:
            focus_radius = float(max(W, H)*100.) if uncertainties is not None else float(min(W, H)/6.)

        Nfits = len(models) - 1
        if implied_Rt10 is not None:
            Rt10 = implied_Rt10[None]
        elif intrinsics_only:
            Rt10 = np.tile(identity_Rt(), (Nfits, 1, 1))
        elif focus_radius == 0:
            Rt10 = np.array([compose_Rt(models[i].Rt_cam_ref(), models[0].Rt_ref_cam()) for i in range(1, len(models))])
        else:
            Rt10 = None

        q0 = sample_imager(gridn_width, gridn_height, W, H)
        with _DiffContext(lensmodels, intrinsics_data, q0) as ctx:
            difflen, diff, Rt10, report = ctx.evaluate(distance, atinfinity, uncertainties, Rt10, focus_center, focus_radius)
        if _report is not None:
            _report.update(report)
    finally:
        for u in made_here: u.close()

    if len(models) == 2:
        diff, Rt10 = diff[0], Rt10[0]
    else:
        diff = None
    if not distance_is_iterable:
        difflen = difflen[0]
        if diff is not None: diff = diff[0]
    return difflen, diff, q0, Rt10
