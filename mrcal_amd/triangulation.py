"""Triangulation: two observation rays -> the point they see.

    p = mrcal_amd.triangulate_leecivera_mid2(v0, v1, t01)
    p, dp_dv0, dp_dv1, dp_dt01 = mrcal_amd.triangulate_geometric(v0, v1, t01, get_gradients = True)
    p = mrcal_amd.triangulate_lindstrom(v0_local, v1_local, Rt01)

The names, arguments, conventions and exceptions are those of the reference's
mrcal/triangulation.py:27-949; the points and their gradients come from one
launch of csrc/triangulation.hip over the whole broadcast batch (one lane per
pair). Where the rays are parallel or divergent the point is (0,0,0), as in the
reference, and its gradients are all zero. There is no CPU fallback.

    p, Var_p_calibration, Var_p_observation, Var_p_joint = \
        mrcal_amd.triangulate(q, (model0, model1), q_calibration_stdev = -1, q_observation_stdev = 0.3)

    with mrcal_amd.Triangulation((model0, model1), calibration = True) as t:     # the problem is built once
        for q in frames: p, Var = t.triangulate(q, q_calibration_stdev = -1)

triangulate() (mrcal/triangulation.py:1616-2018) unprojects, composes the poses, triangulates and propagates the
observation-time and the calibration-time noise on the GPU: include/mrcal_amd.h, mrcal_amd_triangulation_*.
"""
import ctypes as C
import numpy as np

from . import _handle
from ._cabi import _ptr, Lensmodel
from ._handle import Handle, _failed
from .poseutils import rotate_point_R


def _parse_args(v1, t01, get_gradients, v_are_local, Rt01):
    """the arguments of the functions that take camera-0 vectors AND t01
    (mrcal/triangulation.py:27-58): -> v1 in camera-0 coordinates, t01"""
    if Rt01 is not None and t01 is not None:
        raise Exception("Exactly one of Rt01 and t01 must be None. Both were non-None")
    if Rt01 is None and t01 is None:
        raise Exception("Exactly one of Rt01 and t01 must be None. Both were None")
    if v_are_local:
        if get_gradients:
            raise Exception("get_gradients is True, so v_are_local MUST be the default: False")
        if Rt01 is None:
            raise Exception("v_are_local is True, so Rt01 MUST have been given")
        Rt01 = np.asarray(Rt01, dtype=np.float64)
        v1   = rotate_point_R(Rt01[...,:3,:], np.asarray(v1, dtype=np.float64))
        t01  = Rt01[...,3,:]
    elif t01 is None:
        if get_gradients:
            raise Exception("get_gradients is True, so t01 MUST have been given")
        t01 = np.asarray(Rt01, dtype=np.float64)[...,3,:]
    return v1, t01


def _flat(a, lead, tail):
    return np.ascontiguousarray(np.broadcast_to(a, lead + tail), dtype=np.float64).reshape((-1,) + tail)


def _run(name, v0, v1, pose, pose_shape, get_gradients, out):
    """the broadcast batch through mrcal_amd_triangulate_<name>(). pose_shape: (3,) for t01, (4,3) for Rt01"""
    v0, v1, pose = (np.asarray(a, dtype=np.float64) for a in (v0, v1, pose))
    npose = len(pose_shape)
    if v0.ndim < 1 or v0.shape[-1] != 3 or v1.ndim < 1 or v1.shape[-1] != 3:
        raise Exception("v0 and v1 must have shape (...,3)")
    if pose.ndim < npose or pose.shape[-npose:] != pose_shape:
        raise Exception(f"{'t01' if npose == 1 else 'Rt01'} must have shape (...,{','.join(str(n) for n in pose_shape)})")
    lead = np.broadcast_shapes(v0.shape[:-1], v1.shape[:-1], pose.shape[:pose.ndim - npose])
    shapes = [lead + (3,)]
    if get_gradients: shapes += [lead + (3,3), lead + (3,3), lead + (3,) + pose_shape]
    if out is not None:
        outs = tuple(out) if get_gradients else (out,)
        if len(outs) != len(shapes) or any(o.shape != s for o, s in zip(outs, shapes)):
            raise Exception(f"'out' must be {'arrays' if get_gradients else 'an array'} of shape {shapes if get_gradients else shapes[0]}")

    a, b, c = _flat(v0, lead, (3,)), _flat(v1, lead, (3,)), _flat(pose, lead, pose_shape)
    N = a.shape[0]
    res = [np.empty((N,) + s[len(lead):]) for s in shapes]
    f = getattr(_handle._libs()[0].lib, "mrcal_amd_triangulate_" + name)
    if not f(N, _ptr(a), _ptr(b), _ptr(c), *[_ptr(r) for r in res], *([None]*(4 - len(res)))):
        raise _failed(f"triangulate_{name}()")
    res = [r.reshape(s) for r, s in zip(res, shapes)]
    if out is not None:
        for o, r in zip(outs, res): o[...] = r
        return out
    return tuple(res) if get_gradients else res[0]


def _make(name, doc):
    def f(v0, v1, t01 = None, *, get_gradients = False, v_are_local = False, Rt01 = None, out = None):
        v1, t01 = _parse_args(v1, t01, get_gradients, v_are_local, Rt01)
        return _run(name, v0, v1, t01, (3,), get_gradients, out)
    f.__name__ = f.__qualname__ = "triangulate_" + name
    f.__doc__ = doc + """

v0, v1: (...,3) observation vectors, not necessarily normalized, both in camera-0
coordinates; t01: (...,3), the origin of camera 1 in camera-0 coordinates. All
broadcast. Rt01 (...,4,3) may be given INSTEAD of t01; with v_are_local v1 is in
camera-1 coordinates, and Rt01 must be given. Returns p (...,3) in camera-0
coordinates: (0,0,0) where the rays are parallel or divergent. With get_gradients
(t01 given, not v_are_local): (p, dp_dv0 (...,3,3), dp_dv1 (...,3,3), dp_dt01
(...,3,3)). out: the array, or the tuple of arrays, to fill and return.
Reference: mrcal/triangulation.py, mrcal.triangulate_""" + name + "()"
    return f


triangulate_geometric = _make("geometric",
    "The midpoint of the two rays' closest approach: the simplest method, the largest bias")
triangulate_leecivera_l1 = _make("leecivera_l1",
    "Minimizes the L1 norm of the two angular errors (Lee, Civera: 'Closed-Form Optimal Two-View Triangulation\n"
    "Based on Angular Errors', ICCV 2019)")
triangulate_leecivera_linf = _make("leecivera_linf",
    "Minimizes the L-infinity norm of the two angular errors (Lee, Civera, ICCV 2019)")
triangulate_leecivera_mid2 = _make("leecivera_mid2",
    "The 'Mid2' method of Lee, Civera: 'Triangulation: Why Optimize?' (arXiv 1907.11917): the preferred one")
triangulate_leecivera_wmid2 = _make("leecivera_wmid2",
    "The 'wMid2' method of Lee, Civera: 'Triangulation: Why Optimize?': Mid2 weighted by the inverse ranges, for\n"
    "points near the cameras")


def triangulate_lindstrom(v0, v1, Rt01, *, get_gradients = False, v_are_local = True, out = None):
    """Minimizes the 2-norm of PINHOLE reprojection errors (Lindstrom: 'Triangulation Made Easy', CVPR 2010; two
iterations)

Unlike the other methods (and like the reference's, mrcal/triangulation.py:799-949) this one takes the whole
transformation Rt01 (...,4,3), and by default v1 in camera-1 coordinates; v_are_local = False: v1 is in camera-0
coordinates like the others'. Returns p (...,3) in camera-0 coordinates, (0,0,0) where the rays are parallel or
divergent. With get_gradients (v_are_local only): (p, dp_dv0 (...,3,3), dp_dv1 (...,3,3), dp_dRt01 (...,3,4,3)).
Everything broadcasts"""
    Rt01 = np.asarray(Rt01, dtype=np.float64)
    if not v_are_local:
        if get_gradients:
            raise Exception("get_gradients is True, so v_are_local MUST be True")
        v1 = rotate_point_R(np.swapaxes(Rt01[...,:3,:], -1, -2), np.asarray(v1, dtype=np.float64))
    return _run("lindstrom", v0, v1, Rt01, (4,3), get_gradients, out)


# ---------------------------------------------------------------------------------------------------------------------
# triangulate()

class _Camera(C.Structure):
    """mrcal_amd_triangulation_camera_t"""
    _fields_ = [("lensmodel", Lensmodel), ("intrinsics", C.c_void_p), ("rt_cam_ref", C.c_double*6),
                ("icam_intrinsics", C.c_int), ("icam_extrinsics", C.c_int)]


def _method_id(method):
    for i, f in enumerate((triangulate_geometric, triangulate_lindstrom, triangulate_leecivera_l1,
                           triangulate_leecivera_linf, triangulate_leecivera_mid2, triangulate_leecivera_wmid2)):
        if method is f: return i
    raise Exception("method must be one of the mrcal_amd.triangulate_...() functions")


def _compute_Var_q_triangulation(sigma, stdev_cross_camera_correlation):
    """Var(q0x, q0y, q1x, q1y) of one pair of observations (mrcal/triangulation.py:1090-1125): sigma^2 on the
    diagonal, (sigma stdev_cross_camera_correlation)^2 between q0x, q1x and between q0y, q1y. (The device forms
    the same matrix; this is the host's statement of it)"""
    var_q = np.eye(4)*sigma*sigma
    var_cross = (sigma*stdev_cross_camera_correlation)**2
    var_q[0,2] = var_q[2,0] = var_q[1,3] = var_q[3,1] = var_cross
    return var_q


def _models_array(models):
    if not isinstance(models, np.ndarray):
        models = np.array(models, dtype=object)
    if models.ndim < 1 or models.shape[-1] != 2:
        raise Exception(f"models must have shape (...,2), got {models.shape}")
    return models


def _check_calibration(models_flat):
    """what the reference asks of the models before it propagates calibration-time noise: -> optimization_inputs.
    (The reference compares every two entries of the flattened array; here each distinct model object is looked at
    once, with the same verdicts: 10^5 pairs are mostly the same few cameras, and a comparison reads the whole
    serialized calibration. For the same reason "moved" is judged against the ONE deserialized copy, which is every
    model's once they all match: cameramodel._extrinsics_moved_since_calibration()'s test, not a call of it)"""
    optimization_inputs = models_flat[0].optimization_inputs()
    if optimization_inputs is None:
        raise Exception("optimization_inputs are not available, so I cannot propagate calibration-time noise")
    seen = {}
    for i0, m in enumerate(models_flat):
        if id(m) in seen: continue
        for other in seen.values():
            if not m._optimization_inputs_match(other):
                raise Exception("The optimization_inputs for all of the given models must be identical")
        seen[id(m)] = m
        icam, rt = m.icam_extrinsics(), m.rt_cam_ref()
        if np.max(np.abs(rt if icam < 0 else rt - optimization_inputs["rt_cam_ref"][icam])) > (0.0 if icam < 0 else 1e-6):
            raise Exception(f"The given models must have been fixed inside the initial calibration. Model {i0} has been moved")
    return optimization_inputs


_LINDSTROM_NOISE = ("Triangulation gradients not supported (yet?) with method=triangulate_lindstrom. "
                    "It has slightly different inputs and slightly different gradients")


class Triangulation(Handle):
    """triangulate() on a set of camera models, kept resident: the models' intrinsics and poses go to the device once,
    and with calibration = True so do the calibration's problem, the factorization of its normal equations and the
    estimate of its pixel noise (the models must then come out of ONE calibration and not have been moved since, as
    for mrcal.triangulate()). models: an iterable of any shape (...,2) of cameramodels: the pairs triangulate() uses
    when it is given none"""

    _destroy = "mrcal_amd_triangulation_destroy"

    def __init__(self, models, *, calibration=False, _optimization_inputs=None):
        self._pairs = _models_array(models)
        flat = self._pairs.ravel()
        self._index, self._models = {}, []
        for m in flat:
            if id(m) not in self._index:
                self._index[id(m)] = len(self._models)
                self._models.append(m)
        # (_optimization_inputs: triangulate() has made the checks already)
        optimization_inputs = (_optimization_inputs or _check_calibration(flat)) if calibration else None
        _lib, _ = _handle._libs()
        self.calibration = bool(calibration)
        cams = (_Camera*len(self._models))()
        keep = []
        for c, m in zip(cams, self._models):
            name, intrinsics = m.intrinsics()
            intrinsics = np.ascontiguousarray(intrinsics, dtype=np.float64)
            keep.append(intrinsics)
            c.lensmodel  = _lib.lensmodel(name)
            c.intrinsics = intrinsics.ctypes.data
            c.rt_cam_ref[:] = [float(x) for x in m.rt_cam_ref()]
            c.icam_intrinsics = int(m.icam_intrinsics()) if calibration else -1
            c.icam_extrinsics = int(m.icam_extrinsics()) if calibration else -1
        if calibration:
            from .cameramodel import _is_poison
            from .resident import Problem
            optimization_inputs = {k: v for k, v in optimization_inputs.items() if not _is_poison(v)}
            with Problem(**optimization_inputs) as problem:
                # (the regularization rows are read off the problem's Jacobian: it must be streamed)
                problem.set_jacobian_stream(True)
                self._create("triangulate()", "mrcal_amd_triangulation_create", problem.handle, len(self._models), C.addressof(cams))
        else:
            self._create("triangulate()", "mrcal_amd_triangulation_create", None, len(self._models), C.addressof(cams))
        est = float(self._function("mrcal_amd_triangulation_observed_pixel_uncertainty")(self.handle))
        self.observed_pixel_uncertainty = est if est > 0 else None

    def triangulate(self, q, models=None, *, q_calibration_stdev=None, q_observation_stdev=None,
                    q_observation_stdev_correlation=0, method=triangulate_leecivera_mid2, stabilize_coords=True):
        """mrcal.triangulate() on this context's cameras. models: the pairs (...,2), each one of the context's models;
        None: those the context was made with"""
        self._open()
        if q_observation_stdev is not None and q_observation_stdev < 0:
            raise Exception("q_observation_stdev MUST be None or >= 0")
        pairs = self._pairs if models is None else _models_array(models)
        with_cal = q_calibration_stdev is not None and q_calibration_stdev != 0
        with_obs = q_observation_stdev is not None and q_observation_stdev != 0
        if with_cal and not self.calibration:
            _check_calibration(pairs.ravel())
            raise Exception("this Triangulation was made with calibration = False: it cannot propagate calibration-time noise")
        imethod = _method_id(method)
        if (with_cal or with_obs) and method is triangulate_lindstrom:
            raise Exception(_LINDSTROM_NOISE)
        q = np.asarray(q, dtype=np.float64)
        if q.ndim < 2 or q.shape[-2:] != (2,2):
            raise Exception(f"q must have shape (...,2,2), got {q.shape}")
        lead = np.broadcast_shapes(q.shape[:-2], pairs.shape[:-1])
        qf = np.ascontiguousarray(np.broadcast_to(q, lead + (2,2))).reshape(-1,2,2)
        try:
            icam = np.array([self._index[id(m)] for m in np.broadcast_to(pairs, lead + (2,)).ravel()], dtype=np.int32)
        except KeyError:
            raise Exception("every model of a pair must be one of those this Triangulation was made with")
        N = qf.shape[0]
        p       = np.zeros((N,3))
        var_obs = np.zeros((N,3,3))   if with_obs else None
        var_cal = np.zeros((3*N,3*N)) if with_cal else None
        if N > 0:
            self._call("triangulate()", "mrcal_amd_triangulation_evaluate", N, _ptr(qf), _ptr(icam), imethod,
                       float(q_calibration_stdev) if with_cal else 0.0, float(q_observation_stdev) if with_obs else 0.0,
                       float(q_observation_stdev_correlation), bool(stabilize_coords), _ptr(p), _ptr(var_obs), _ptr(var_cal))

        p = p.reshape(lead + (3,))
        if q_calibration_stdev is None and q_observation_stdev is None:
            return p
        Var_p_calibration = Var_p_observation = None
        if q_calibration_stdev is not None:
            Var_p_calibration = (var_cal if with_cal else np.zeros((3*N,3*N))).reshape(lead + (3,) + lead + (3,))
        if q_observation_stdev is not None:
            Var_p_observation = (var_obs if with_obs else np.zeros((N,3,3))).reshape(lead + (3,3))
        if Var_p_observation is None: return p, Var_p_calibration
        if Var_p_calibration is None: return p, Var_p_observation
        # both: the joint covariance, the observation-time blocks on the diagonal
        Var_p_joint = Var_p_calibration.copy()
        flat = Var_p_joint.reshape(3*N, 3*N)
        if with_obs:
            for i in range(N): flat[3*i:3*i+3, 3*i:3*i+3] += var_obs[i]
        return p, Var_p_calibration, Var_p_observation, Var_p_joint


def triangulate(q, models, *, q_calibration_stdev=None, q_observation_stdev=None, q_observation_stdev_correlation=0,
                method=triangulate_leecivera_mid2, stabilize_coords=True):
    """mrcal.triangulate() (mrcal/triangulation.py:1616-2018): N points from pixel pairs, with the noise propagated

q (...,2,2): a pixel observation from each of the two cameras; models (...,2): the two cameramodels. They broadcast.
p (...,3) is in the coordinates of each pair's first camera; (0,0,0) where the rays are parallel or divergent.

q_observation_stdev: the noise of q, independent in x and y, correlated between the two cameras by
q_observation_stdev_correlation (0..1). q_calibration_stdev: the noise of the calibration's pixel observations,
propagated through the calibration; < 0: estimated from the calibration's residuals. The models must then carry the
optimization_inputs of ONE calibration, and not have been moved since. stabilize_coords: Var_p_calibration in the
coordinates of the first camera's housing. method: one of triangulate_...(); triangulate_lindstrom only without noise.

Each stdev that is None: that noise is neither propagated nor returned; 0: zeros are returned.
Returns p; (p, Var_p_calibration); (p, Var_p_observation); or (p, Var_p_calibration, Var_p_observation, Var_p_joint),
with Var_p_calibration and Var_p_joint (...,3, ...,3) (the cross terms between the points) and Var_p_observation
(...,3,3). One-shot form of Triangulation(models, ...).triangulate(q, ...)"""
    if q_observation_stdev is not None and q_observation_stdev < 0:
        raise Exception("q_observation_stdev MUST be None or >= 0")
    models = _models_array(models)
    with_cal = q_calibration_stdev is not None and q_calibration_stdev != 0
    with_obs = q_observation_stdev is not None and q_observation_stdev != 0
    optimization_inputs = _check_calibration(models.ravel()) if with_cal else None
    _method_id(method)
    if (with_cal or with_obs) and method is triangulate_lindstrom:
        raise Exception(_LINDSTROM_NOISE)
    with Triangulation(models, calibration=with_cal, _optimization_inputs=optimization_inputs) as t:
        return t.triangulate(q, q_calibration_stdev=q_calibration_stdev, q_observation_stdev=q_observation_stdev,
                             q_observation_stdev_correlation=q_observation_stdev_correlation, method=method,
                             stabilize_coords=stabilize_coords)
