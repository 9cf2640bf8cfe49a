"""Lens-model conversion: the reference's mrcal-convert-lensmodel as a function.

fit_lensmodel()      the sampled fit as the device runs it (include/mrcal_amd.h, "lens-model fit"; csrc/lensfit.hip):
                     fixed points, one parametric lens model's intrinsics and optionally the pose as unknowns, every
                     start of a call in one launch
convert_lensmodel()  the tool's semantics around it (mrcal-convert-lensmodel:402-842): the sampled fit, or the
                     re-optimization of the model's own calibration problem through optimize(). The tool's error
                     messages, raised"""
import copy
import ctypes as C
import re

import numpy as np

from . import _handle
from ._cabi import _ptr
from ._handle import Handle, _failed

STATUS_CONVERGED, STATUS_BOUND, STATUS_TOO_FEW_POINTS, STATUS_STALLED = 0, 1, 2, 3
STATUS_NAMES = ("converged", "bound on evaluations reached", "too few points", "stalled")


PLAN_FIELDS = ("proj", "ndist", "Nintrinsics", "ivar0", "Nstages", "NP1", "NP2", "Nsums", "threads", "row_doubles",
               "chunk_rows", "lds_bytes", "Nmeasurements", "lds_limit")


def fit_lensmodel_plan(lensmodel, N, *, Ntrials=1, imagersize=(2, 2), optimize_core=True, optimize_extrinsics=False,
                       do_apply_regularization=True):
    """What fit_lensmodel() decides on the host for these arguments (csrc/lensfit_plan.hpp), as a dict of PLAN_FIELDS:
    the kernel's instantiation, the unknowns of each stage, threads, the chunk of rows, LDS. Raises what
    fit_lensmodel() would refuse with. No device is touched"""
    _lib, _ = _handle._libs()
    m = _lib.lensmodel(lensmodel)
    out = np.zeros(len(PLAN_FIELDS), dtype=np.int32)
    size = np.ascontiguousarray(np.asarray(imagersize).reshape(2), dtype=np.int32)
    if not _lib.lib.mrcal_amd_lensfit_plan(_ptr(out), C.byref(m), int(N), int(Ntrials), _ptr(size), bool(optimize_core),
                                           bool(optimize_extrinsics), bool(do_apply_regularization)):
        raise _failed("fit_lensmodel()")
    return dict(zip(PLAN_FIELDS, (int(v) for v in out)))


class LensFitter(Handle):
    """The resident form (mrcal_amd_lensfit_*): keeps its device buffers and stream between fits"""
    _destroy = "mrcal_amd_lensfit_destroy"

    def __init__(self):
        self._create("fit_lensmodel()", "mrcal_amd_lensfit_create")

    def fit(self, p, q, lensmodel, intrinsics_seed, *, imagersize, weights=None, rt_seed=None, optimize_core=True,
            optimize_extrinsics=False, do_apply_regularization=True, max_evaluations=None):
        p = np.ascontiguousarray(p, dtype=np.float64)
        q = np.ascontiguousarray(q, dtype=np.float64)
        if p.ndim != 2 or p.shape[1] != 3:
            raise Exception(f"p must have shape (N,3), got {p.shape}")
        N = p.shape[0]
        if q.shape != (N, 2):
            raise Exception(f"q must have shape ({N},2), got {q.shape}")
        if weights is not None:
            weights = np.ascontiguousarray(weights, dtype=np.float64)
            if weights.shape != (N,):
                raise Exception(f"weights must have shape ({N},), got {weights.shape}")
        m = _handle._libs()[0].lensmodel(lensmodel)
        Ni = self._function("mrcal_lensmodel_num_params")(C.byref(m))
        seed = np.ascontiguousarray(intrinsics_seed, dtype=np.float64)
        one = seed.ndim == 1
        if one: seed = seed.reshape(1, -1)
        if seed.ndim != 2 or seed.shape[1] != Ni:
            raise Exception(f"{lensmodel} takes {Ni} intrinsics: intrinsics_seed must have shape (Ntrials,{Ni}), got {seed.shape}")
        Nt = seed.shape[0]
        if rt_seed is not None:
            rt_seed = np.ascontiguousarray(rt_seed, dtype=np.float64).reshape(-1, 6)
            if rt_seed.shape != (Nt, 6):
                raise Exception(f"rt_seed must have shape ({Nt},6), got {rt_seed.shape}")
        size = np.ascontiguousarray(np.asarray(imagersize).reshape(2), dtype=np.int32)
        intrinsics, rt = np.zeros((Nt, Ni)), np.zeros((Nt, 6))
        cost, rms = np.zeros(Nt), np.zeros(Nt)
        Nevaluations, status = np.zeros(Nt, dtype=np.int32), np.full(Nt, -1, dtype=np.int32)
        ibest = C.c_int(-1)
        self._call("fit_lensmodel()", "mrcal_amd_lensfit_fit", _ptr(p), _ptr(q), _ptr(weights), N, C.byref(m), _ptr(size),
                   _ptr(seed), _ptr(rt_seed), Nt,
                   bool(optimize_core), bool(optimize_extrinsics), bool(do_apply_regularization),
                   0 if max_evaluations is None else int(max_evaluations),
                   _ptr(intrinsics), _ptr(rt), _ptr(cost), _ptr(rms), _ptr(Nevaluations), _ptr(status), C.byref(ibest))
        return dict(intrinsics=intrinsics, rt_cam_ref=rt, cost=cost, rms_reproj_error__pixels=rms,
                    Nevaluations=Nevaluations, status=status, ibest=ibest.value)

    def last_ms(self):
        return self._function("mrcal_amd_lensfit_last_ms")(self.handle)


def fit_lensmodel(p, q, lensmodel, intrinsics_seed, *, imagersize, weights=None, rt_seed=None, optimize_core=True,
                  optimize_extrinsics=False, do_apply_regularization=True, max_evaluations=None):
    """Fit the intrinsics of a parametric lens model, and optionally the pose rt_cam_ref, to fixed points: minimise the
    reference's cost x.x, x = w (project(T p) - q) and mrcal_optimize()'s regularization rows, by damped Gauss-Newton
    on the GPU (include/mrcal_amd.h, "lens-model fit").
    p (N,3) in the from-camera's coordinates, q (N,2), weights (N,) or None; intrinsics_seed (Ntrials,Nintrinsics) or
    (Nintrinsics,): every row is a start, and all starts run in one launch; rt_seed (Ntrials,6) or None: the pose's
    starts in stage 2. optimize_core=False keeps fx,fy,cx,cy as seeded. max_evaluations: the bound on the cost
    evaluations of a stage (None: 200).
    Returns a dict: intrinsics (Ntrials,Nintrinsics), rt_cam_ref (Ntrials,6), cost, rms_reproj_error__pixels,
    Nevaluations, status (Ntrials each: 0 converged, 1 bound reached, 2 too few points, 3 stalled), ibest: the trial of
    the lowest rms among those that did not fail (-1: none)"""
    with LensFitter() as f:
        return f.fit(p, q, lensmodel, intrinsics_seed, imagersize=imagersize, weights=weights, rt_seed=rt_seed,
                     optimize_core=optimize_core, optimize_extrinsics=optimize_extrinsics,
                     do_apply_regularization=do_apply_regularization, max_evaluations=max_evaluations)


# ---------------------------------------------------------------------------------------------------------------------
# the tool

def _is_splined(lensmodel):
    return re.match("LENSMODEL_SPLINED_STEREOGRAPHIC_", lensmodel) is not None


def _rational_terms(lensmodel_to):
    """The distortion terms k5, k6, k7 of OPENCV8 and OPENCV12 - the denominator of the radial factor - as a slice of the
    intrinsics vector; None for every other model"""
    return slice(9, 12) if lensmodel_to in ("LENSMODEL_OPENCV8", "LENSMODEL_OPENCV12") else None


def _scale_down_rational_intrinsics(lensmodel_to, intrinsics):
    """The tool starts the denominator's terms a thousand times nearer 0 than the others, so that the radial factor
    cannot begin near 0/0 (mrcal-convert-lensmodel:379-398). In place, on the last axis"""
    terms = _rational_terms(lensmodel_to)
    if terms is not None:
        intrinsics[..., terms] *= 1e-3


def _sample_grid(dims, gridn, where, radius):
    """mrcal-convert-lensmodel:636-681: the (Ny*Nx,2) pixels of an Nx by Ny grid over the imager, cut to those within
    radius of where (None: the centre). radius None: minus a quarter of the smaller dimension; < 0: the half
    diagonal less that much, about the centre only; 0: everything"""
    dims = np.asarray(dims)
    center = (dims - 1.)/2.
    if where is not None:
        where = np.asarray(where, dtype=float)
    if radius is None:
        radius = -np.min(dims)//4
        if where is not None and np.sum((where - center)**2) > 1e-3:
            raise Exception("A radius <0 is only implemented if we're focusing on the imager center: use an explicit --radius, or omit --where")
    Nx, Ny = gridn
    qx = np.linspace(0, dims[0] - 1, Nx)
    qy = np.linspace(0, dims[1] - 1, Ny)
    q = np.ascontiguousarray(np.stack(np.meshgrid(qx, qy), axis=-1).reshape(-1, 2))
    if radius != 0:
        focus_center = center if where is None else where
        if radius > 0:
            r = radius
        else:
            if np.sum((focus_center - center)**2) > 1e-3:
                raise Exception("A radius <0 is only implemented if we're focusing on the imager center")
            r = np.sqrt(np.sum(dims.astype(float)**2))/2. + radius
        off = q - focus_center
        q = q[np.sum(off*off, axis=-1) < r*r]
    return q


def _starts(lensmodel_to, core, Ndistortions, num_trials, seed, distortion_seeds, with_pose):
    """mrcal-convert-lensmodel:727-731, 786, trial by trial from numpy.random.default_rng(seed): the from-model's core,
    distortions (u - 0.5) 1e-3 with the rational terms pushed down, the pose (u - 0.5) 1e-6. distortion_seeds
    (num_trials,Ndistortions) are taken as they are, instead of the draw.
    Returns (intrinsics (num_trials,4+Ndistortions), rt (num_trials,6) or None)"""
    rng = np.random.default_rng(seed)
    if distortion_seeds is not None:
        distortion_seeds = np.asarray(distortion_seeds, dtype=float)
        if distortion_seeds.shape != (num_trials, Ndistortions):
            raise Exception(f"distortion_seeds must have shape ({num_trials},{Ndistortions}), got {distortion_seeds.shape}")
    intrinsics = np.zeros((num_trials, 4 + Ndistortions))
    rt = np.zeros((num_trials, 6)) if with_pose else None
    for i in range(num_trials):
        intrinsics[i, :4] = core
        if distortion_seeds is None:
            intrinsics[i, 4:] = (rng.random(Ndistortions) - 0.5)*1e-3
            _scale_down_rational_intrinsics(lensmodel_to, intrinsics[i])
        else:
            intrinsics[i, 4:] = distortion_seeds[i]
        if with_pose:
            rt[i] = (rng.random(6) - 0.5)*1e-6
    return intrinsics, rt


def _sampled_inputs(p, q, weights, lensmodel_to, intrinsics, dims, rt_cam_ref, optimize_core):
    """the optimization_inputs of mrcal-convert-lensmodel:734-767 (and :784-787 with a pose)"""
    N = len(p)
    idx = np.zeros((N, 3), dtype=np.int32)
    idx[:, 0] = np.arange(N, dtype=np.int32)
    idx[:, 2] = -1 if rt_cam_ref is None else 0
    return dict(intrinsics=np.array(intrinsics, dtype=float).reshape(1, -1),
                rt_cam_ref=None if rt_cam_ref is None else np.array(rt_cam_ref, dtype=float).reshape(1, 6),
                rt_ref_frame=None, points=np.ascontiguousarray(p),
                observations_board=None, indices_frame_camintrinsics_camextrinsics=None,
                observations_point=np.ascontiguousarray(np.column_stack((q, weights))),
                indices_point_camintrinsics_camextrinsics=idx,
                lensmodel=lensmodel_to, imagersizes=np.asarray(dims, dtype=np.int32).reshape(1, 2),
                do_optimize_intrinsics_core=optimize_core, do_optimize_intrinsics_distortions=True,
                do_optimize_extrinsics=rt_cam_ref is not None, do_optimize_frames=False,
                do_apply_outlier_rejection=False, verbose=False)


def _moved_warning(implied_Rt10, sampled_with_distance):
    from .poseutils import rt_from_Rt
    shift = float(np.linalg.norm(rt_from_Rt(implied_Rt10)[3:]))
    if shift <= 0.01:
        return None
    msg = f"## WARNING: fitted camera moved by {shift:.03f}m. This is probably aphysically high, and something is wrong."
    return msg + " Pass both a high and a low --distance?" if sampled_with_distance else msg


def _convert_sampled(model, lensmodel_to, Ndistortions, gridn, distance, intrinsics_only, where, radius, num_trials, seed,
                     distortion_seeds):
    from . import _api
    from .poseutils import identity_Rt, Rt_from_rt
    from .cameramodel import cameramodel
    distance_given = distance is not None
    if distance is None:
        if not intrinsics_only:
            raise Exception("--sampled without --intrinsics-only REQUIRES --distance")
        distance = [10.]
    d = np.atleast_1d(np.asarray(distance, dtype=float))
    if not np.all(np.isfinite(d) & (d > 0)):
        raise Exception("All values in --distances must be finite and > 0")
    lensmodel_from, intrinsics_from = model.intrinsics()
    dims = model.imagersize()
    q = _sample_grid(dims, gridn, where, radius)
    v = _api.unproject(q, lensmodel_from, intrinsics_from, normalize=True)
    # (Ndistances, Ngrid, ...) flattened, the distances outermost
    p = (v[None, :, :]*d[:, None, None]).reshape(-1, 3)
    q = np.tile(q, (d.size, 1))
    finite = np.isfinite(p[:, 0])
    p, q = np.ascontiguousarray(p[finite]), np.ascontiguousarray(q[finite])
    weights = np.ones(len(q))

    seeds, rt_seeds = _starts(lensmodel_to, intrinsics_from[:4], Ndistortions, num_trials, seed, distortion_seeds,
                              not intrinsics_only)
    info = dict(Npoints=len(q), warning_status=None)
    if not _is_splined(lensmodel_to):
        fit = fit_lensmodel(p, q, lensmodel_to, seeds, imagersize=dims, weights=weights, rt_seed=rt_seeds,
                            optimize_extrinsics=not intrinsics_only)
        info.update(rms_reproj_error__pixels=fit["rms_reproj_error__pixels"], status=fit["status"],
                    Nevaluations=fit["Nevaluations"], cost=fit["cost"], ibest=fit["ibest"])
        if fit["ibest"] < 0:
            raise Exception("No valid intrinsics found!")
        if fit["status"][fit["ibest"]] != STATUS_CONVERGED:
            info["warning_status"] = (f"## WARNING: the best trial did not converge (status {int(fit['status'][fit['ibest']])}: "
                                      f"{STATUS_NAMES[int(fit['status'][fit['ibest']])]}) and ended at rms {fit['rms_reproj_error__pixels'][fit['ibest']]:.3f} "
                                      "pixels. More trials (num_trials) may find a better fit")
        intrinsics_best = fit["intrinsics"][fit["ibest"]]
        rt_best         = fit["rt_cam_ref"][fit["ibest"]]
    else:
        # thousands of unknowns, each seen by a few points: the sparse solver's problem, the core locked
        # (mrcal-convert-lensmodel:769-773), one trial after another
        rms = np.full(num_trials, np.nan)
        intrinsics_best = rt_best = None
        best = -1
        for i in range(num_trials):
            oi = _sampled_inputs(p, q, weights, lensmodel_to, seeds[i], dims, None, False)
            stats = _api.optimize(**oi)
            if not intrinsics_only:
                oi = _sampled_inputs(p, q, weights, lensmodel_to, oi["intrinsics"][0], dims, rt_seeds[i], False)
                stats = _api.optimize(**oi)
            rms[i] = stats["rms_reproj_error__pixels"]
            if np.isfinite(rms[i]) and (best < 0 or rms[i] < rms[best]):
                best = i
                intrinsics_best = oi["intrinsics"][0].copy()
                rt_best = None if intrinsics_only else oi["rt_cam_ref"][0].copy()
        info.update(rms_reproj_error__pixels=rms, status=np.where(np.isfinite(rms), STATUS_CONVERGED, STATUS_STALLED).astype(np.int32),
                    ibest=best)
        if best < 0:
            raise Exception("No valid intrinsics found!")

    model_to = cameramodel(intrinsics=(lensmodel_to, np.array(intrinsics_best)), imagersize=dims)
    implied_Rt10 = identity_Rt() if intrinsics_only else Rt_from_rt(rt_best)
    info["warning"] = None if intrinsics_only else _moved_warning(implied_Rt10, distance_given)
    return model_to, implied_Rt10, info


def _monocular_inputs(optimization_inputs, icam_intrinsics):
    """mrcal-convert-lensmodel:422-501: the calibration problem cut down to one camera sitting at the reference"""
    from .poseutils import compose_rt
    oi = optimization_inputs
    ipc = oi.get('indices_point_camintrinsics_camextrinsics')
    if ipc is not None and np.size(ipc) > 0:
        raise Exception("--monocular can be used ONLY to re-optimize vanilla calibration problems. This one has points")
    ifce = oi['indices_frame_camintrinsics_camextrinsics']
    mask = ifce[:, 1] == icam_intrinsics
    ifce = ifce[mask].copy()
    oi['observations_board'] = oi['observations_board'][mask]
    if 'imagepaths' in oi and oi['imagepaths'] is not None:
        oi['imagepaths'] = np.asarray(oi['imagepaths'])[mask]
    ifce[:, 1] = 0
    oi['intrinsics']  = oi['intrinsics'][(icam_intrinsics,), :]
    oi['imagersizes'] = oi['imagersizes'][(icam_intrinsics,), :]
    icam_extrinsics = ifce[0, 2]
    if not np.all(ifce[:, 2] == icam_extrinsics):
        raise Exception("Error: --monocular can work ONLY if the calibration-time cameras are stationary. Here the requested camera was moving")
    ifce[:, 2] = -1
    rt_ref_frame = oi['rt_ref_frame']
    if icam_extrinsics >= 0:
        # the reference moves to this camera
        rt_ref_frame = compose_rt(oi['rt_cam_ref'][icam_extrinsics], rt_ref_frame)
    oi['rt_cam_ref'] = np.empty((0, 6), dtype=float)
    oi['rt_ref_frame'] = np.ascontiguousarray(rt_ref_frame[ifce[:, 0], :])
    ifce[:, 0] = np.arange(len(ifce))
    oi['indices_frame_camintrinsics_camextrinsics'] = np.ascontiguousarray(ifce)
    return oi


def _cull_past_radius(oi, where, radius):
    """mrcal-convert-lensmodel:512-538: observations further than the radius from the focus are made outliers"""
    if radius is None or radius == 0:
        return
    for icam in range(len(oi['intrinsics'])):
        dims = oi['imagersizes'][icam].astype(float)
        center = (dims - 1)/2
        focus_center = center if where is None else np.asarray(where, dtype=float)
        if radius > 0:
            r = radius
        else:
            if np.sum((focus_center - center)**2) > 1e-3:
                raise Exception("A radius <0 is only implemented if we're focusing on the imager center")
            r = np.sqrt(np.sum(dims*dims))/2. + radius
        obs = oi['observations_board']
        thiscam = oi['indices_frame_camintrinsics_camextrinsics'][:, 1] == icam
        past = np.sum((obs[..., :2] - focus_center)**2, axis=-1) > r*r
        obs[thiscam[:, None, None] & past, 2] = -1


def _convert_stages(oi, lensmodel_to, Ndistortions, seed, distortion_seeds, optimize):
    """mrcal-convert-lensmodel:541-577: the four stages, in place. optimize: the solver (the tests hand the
    reference's in). Returns the last stage's stats"""
    Ncameras = len(oi['intrinsics'])
    core = oi['intrinsics'][..., :4].copy()
    oi['verbose'] = False
    oi['lensmodel'] = lensmodel_to
    oi['intrinsics'] = np.zeros((Ncameras, Ndistortions + 4))
    oi['intrinsics'][:, :4] = core
    # the frames and the extrinsics, under a core-only model
    oi['do_optimize_intrinsics_core']        = False
    oi['do_optimize_intrinsics_distortions'] = False
    oi['do_optimize_calobject_warp']         = False
    oi['do_apply_outlier_rejection']         = False
    oi['do_apply_regularization']            = False
    optimize(**oi)
    # the core as well
    oi['do_optimize_intrinsics_core'] = True
    optimize(**oi)
    # the distortions
    oi['do_optimize_intrinsics_distortions'] = True
    oi['do_apply_outlier_rejection']         = True
    oi['do_apply_regularization']            = True
    if _is_splined(lensmodel_to):
        oi['do_optimize_intrinsics_core'] = False
    if distortion_seeds is None:
        oi['intrinsics'][:, 4:] = (np.random.default_rng(seed).random((Ncameras, Ndistortions)) - 0.5)*2.*1e-6
        _scale_down_rational_intrinsics(lensmodel_to, oi['intrinsics'])
    else:
        oi['intrinsics'][:, 4:] = np.asarray(distortion_seeds, dtype=float).reshape(Ncameras, Ndistortions)
    optimize(**oi)
    # and the board's warp
    oi['do_optimize_calobject_warp'] = True
    return optimize(**oi)


def _convert_full(model, lensmodel_to, Ndistortions, where, radius, monocular, seed, distortion_seeds):
    from . import _api
    from .cameramodel import cameramodel
    from .calibration import align_procrustes_points_Rt01
    from .utils import hypothesis_board_corner_positions
    oi = model.optimization_inputs()
    if oi is None:
        raise Exception("optimization_inputs not available in this model, so only sampled fits are possible. Pass --sampled")
    oi = {k: v for k, v in oi.items() if not (isinstance(v, str) and v.startswith("ERROR:"))}
    icam_intrinsics = model.icam_intrinsics()
    if monocular:
        oi = _monocular_inputs(oi, icam_intrinsics)
        icam_intrinsics = 0
    before = copy.deepcopy(oi)
    _cull_past_radius(oi, where, radius)
    stats = _convert_stages(oi, lensmodel_to, Ndistortions, seed, distortion_seeds, _api.optimize)
    inliers_after = oi['observations_board'][..., 2] > 0
    pcam_before = hypothesis_board_corner_positions(icam_intrinsics, idx_inliers=inliers_after.copy(), **before)[-2]
    pcam_after  = hypothesis_board_corner_positions(icam_intrinsics, idx_inliers=inliers_after.copy(), **oi)[-2]
    implied_Rt10 = align_procrustes_points_Rt01(pcam_after, pcam_before)
    model_to = cameramodel(optimization_inputs=oi, icam_intrinsics=icam_intrinsics)
    info = dict(rms_reproj_error__pixels=np.array((stats['rms_reproj_error__pixels'],)),
                status=np.array((STATUS_CONVERGED,), dtype=np.int32), ibest=0, stats=stats,
                optimization_inputs=oi, warning=_moved_warning(implied_Rt10, False), warning_status=None)
    return model_to, implied_Rt10, info


def convert_lensmodel(model, lensmodel_to, *, sampled=None, gridn=(30, 20), distance=None, intrinsics_only=False,
                      where=None, radius=None, monocular=False, num_trials=1, seed=0, distortion_seeds=None):
    """The reference's mrcal-convert-lensmodel: a camera model re-expressed with another lens model. Returns
    (model_to, info).

    sampled (the default when the model carries no optimization_inputs): the imager is sampled on a grid of gridn
    pixels within radius of where (mrcal-convert-lensmodel:636-681), unprojected through the model to the distances
    given (intrinsics_only: any one distance), and lensmodel_to is fitted to those points from num_trials starts made
    from numpy.random.default_rng(seed) as the tool makes them, or with distortion_seeds (num_trials,Ndistortions)
    in place of the random distortions. A parametric target is fitted on the GPU, all starts in one launch
    (fit_lensmodel()); a splined target goes to optimize(), its core locked, start by start. Unless intrinsics_only
    the pose is fitted too. The best trial becomes the model.
    sampled=False: the model's own calibration problem is solved again with lensmodel_to in the tool's four stages
    through optimize(); monocular: with this camera alone, at the reference; radius: observations beyond it are
    culled. The implied transformation is then the Procrustes fit of the board corners before and after.

    model_to's pose is implied_Rt10 composed with the model's. info: rms_reproj_error__pixels and status of every
    trial, ibest, implied_Rt10, warning: the tool's text if the fitted camera moved more than 1 cm, or None,
    warning_status: a text if the trial chosen in sampled mode did not converge, or None"""
    from . import _api
    from .cameramodel import cameramodel
    from .poseutils import compose_Rt, Rt_from_rt, identity_Rt
    if not isinstance(model, cameramodel):
        model = cameramodel(model)
    try:
        Ndistortions = _api.lensmodel_num_params(lensmodel_to) - 4
    except Exception:
        raise Exception(f"Unknown lens model: '{lensmodel_to}'")
    if sampled is None:
        sampled = model.optimization_inputs() is None
    if num_trials < 1:
        raise Exception(f"num_trials must be at least 1, got {num_trials}")
    if not sampled and intrinsics_only:
        raise Exception("--intrinsics-only requires --sampled")

    if model.intrinsics()[0] == lensmodel_to:
        # "Input and output have the same lens model. Nothing to do"
        return cameramodel(model), dict(rms_reproj_error__pixels=np.zeros(1), status=np.zeros(1, dtype=np.int32), ibest=0,
                                        implied_Rt10=identity_Rt(), warning=None, warning_status=None)
    if sampled:
        model_to, implied_Rt10, info = _convert_sampled(model, lensmodel_to, Ndistortions, gridn, distance, intrinsics_only,
                                                        where, radius, num_trials, seed, distortion_seeds)
    else:
        model_to, implied_Rt10, info = _convert_full(model, lensmodel_to, Ndistortions, where, radius, monocular, seed,
                                                     distortion_seeds)
    info["implied_Rt10"] = implied_Rt10
    model_to.Rt_cam_ref(compose_Rt(implied_Rt10, Rt_from_rt(model.rt_cam_ref())))
    return model_to, info
