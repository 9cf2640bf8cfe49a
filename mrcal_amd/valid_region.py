"""The valid-intrinsics region of a calibrated camera: the step of mrcal-calibrate-cameras between the solve and the
.cameramodel file (mrcal-calibrate-cameras:883-906), and the use of the region afterwards.

    with mrcal.RegionalStatistics(optimization_inputs, gridn_width=30) as s:      # all cameras, one pass on the GPU
        mean, stdev, count = s.of_camera(0)
    mrcal.valid_intrinsics_regions(models)                                         # sets every model's region
    mask = mrcal.is_within_valid_intrinsics_region(q, model)                       # (...,) bool, or None
    image = mrcal.valid_intrinsics_mask(model)                                     # (H,W) uint8

The definitions are in include/mrcal_amd.h ("regional statistics", "valid-intrinsics region"): csrc/regional_stats.hip
bins the residuals, csrc/valid_region.hip makes the mask and applies a region, csrc/region_outline.cpp (host) follows
the mask's outline. The functions with the reference's names and arguments, _report_regional_statistics() and
_compute_valid_intrinsics_region(), are in mrcal_amd.calibration.
"""
import ctypes as C
import re
import sys

import numpy as np

from . import _handle
from ._cabi import _ptr
from ._handle import Handle, _failed


def _grid_height(gridn_width, gridn_height, imagersize):
    if gridn_height is not None:
        return int(gridn_height)
    W, H = (int(v) for v in imagersize)
    return int(round(H/W*gridn_width))


def imagergrid_using(imagersize, gridn_width, gridn_height=None):
    """the gnuplotlib 'using' expression that scales a (gridn_height,gridn_width) array to the imager
    (mrcal.imagergrid_using())"""
    W, H = (int(v) for v in imagersize)
    gridn_height = _grid_height(gridn_width, gridn_height, imagersize)
    return '($1*{}):($2*{}):3'.format(float(W - 1)/(gridn_width - 1), float(H - 1)/(gridn_height - 1))


class RegionalStatistics(Handle):
    """mean, standard deviation and count of the board residuals in every cell of a grid over the imager, for ALL the
    cameras of a solve, binned in one pass on the GPU and kept there. optimization_inputs: of the solve (at its
    optimum: x is evaluated there). gridn_height=None: int(round(H/W*gridn_width)) for each camera's own imager.
    problem: a resident mrcal_amd.resident.Problem to bin at its current state instead of making one"""

    _destroy = "mrcal_amd_regional_statistics_destroy"

    def __init__(self, optimization_inputs, gridn_width=20, gridn_height=None, *, problem=None):
        gw = int(gridn_width)
        gh = -1 if gridn_height is None else int(gridn_height)
        if gridn_height is not None and gh < 2:
            raise Exception(f"regional statistics: gridn_height must be >= 2: got {gridn_height}")
        if problem is not None:
            self._create("regional statistics", "mrcal_amd_regional_statistics_create", problem.handle, gw, gh)
        else:
            from .cameramodel import _is_poison
            from .resident import Problem
            inputs = {k: v for k, v in optimization_inputs.items() if not _is_poison(v)}
            ob = inputs.get('observations_board')
            if ob is None or np.size(ob) == 0:
                raise Exception("regional statistics: the problem has no board observations, and only those are binned")
            with Problem(**inputs) as p:
                self._create("regional statistics", "mrcal_amd_regional_statistics_create", p.handle, gw, gh)
        self.gridn_width = gw

    def grid_of_camera(self, icam_intrinsics):
        """(gridn_width, gridn_height) of one camera"""
        self._open()
        gw, gh = C.c_int(0), C.c_int(0)
        self._call("regional statistics", "mrcal_amd_regional_statistics_grid", int(icam_intrinsics), C.byref(gw), C.byref(gh))
        return gw.value, gh.value

    def of_camera(self, icam_intrinsics):
        """(mean, stdev, count) of one camera, each (gridn_height,gridn_width); count is int32"""
        gw, gh = self.grid_of_camera(icam_intrinsics)
        mean, stdev, count = np.empty((gh, gw)), np.empty((gh, gw)), np.empty((gh, gw), dtype=np.int32)
        self._call("regional statistics", "mrcal_amd_regional_statistics_get", int(icam_intrinsics), _ptr(mean), _ptr(stdev),
                   _ptr(count))
        return mean, stdev, count

    def binning_ms(self):
        """device time of the binning launches"""
        self._open()
        return float(self._function("mrcal_amd_regional_statistics_binning_ms")(self.handle))


def _model_inputs(model):
    optimization_inputs = model.optimization_inputs()
    if optimization_inputs is None:
        raise Exception("optimization_inputs are unavailable in this model. The regional statistics cannot be computed")
    return optimization_inputs, model.icam_intrinsics()


def report_regional_statistics(model, gridn_width=20, gridn_height=None):
    W, H = model.imagersize()
    gridn_height = _grid_height(gridn_width, gridn_height, (W, H))
    optimization_inputs, icam = _model_inputs(model)
    with RegionalStatistics(optimization_inputs, gridn_width, gridn_height) as s:
        mean, stdev, count = s.of_camera(icam)
    return mean, stdev, count, imagergrid_using((W, H), gridn_width, gridn_height)


def region_outline(mask):
    """The outline of the largest 8-connected region of a mask (H,W): its vertices (N,2) int32 as (x,y) = (column,
    row), clockwise on the screen from the topmost-leftmost cell, not closed; and twice its shoelace area. The
    definition: include/mrcal_amd.h. Host code"""
    lib, _ = _handle._libs()
    m = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
    if m.ndim != 2 or m.size == 0:
        raise Exception(f"the mask must have shape (H,W), got {m.shape}")
    h, w = m.shape
    capacity = 64
    while True:
        v = np.zeros((capacity, 2), dtype=np.int32)
        area2 = C.c_int64(0)
        n = lib.lib.mrcal_amd_region_outline(_ptr(m), w, h, _ptr(v), capacity, C.byref(area2))
        if n < 0:
            raise Exception("region_outline(): bad arguments")
        if n <= capacity:
            return v[:n].copy(), int(area2.value)
        capacity = n


def contour_of_mask(mask, imagersize):
    """the closed, scaled, rounded contour (N,2) int32 of a grid mask, as calibration.py:1703-1717 makes it; (0,2) for an
    empty region: no set cell, or fewer than 4 points once closed (a single cell, a line of cells)"""
    from .poseutils import close_contour
    gh, gw = mask.shape
    vertices, _ = region_outline(mask)
    if vertices.shape[0] == 0:
        return np.zeros((0, 2))
    contour = close_contour(vertices.astype(float))
    if contour.ndim != 2 or contour.shape[0] < 4:
        return np.zeros((0, 2))
    W, H = (int(v) for v in imagersize)
    contour[:, 0] *= float(W - 1)/(gw - 1)
    contour[:, 1] *= float(H - 1)/(gh - 1)
    return contour.round().astype(np.int32)


def compute_valid_intrinsics_region(model, threshold_uncertainty, threshold_mean, threshold_stdev, threshold_count,
                                    distance, gridn_width=30, gridn_height=None, *,
                                    uncertainty=None, statistics=None, return_details=False):
    from .model_analysis import ProjectionUncertainty
    lib, api = _handle._libs()
    W, H = (int(v) for v in model.imagersize())
    gridn_width  = int(gridn_width)
    gridn_height = _grid_height(gridn_width, gridn_height, (W, H))
    if gridn_width < 2 or gridn_height < 2:
        raise Exception(f"valid-intrinsics region: gridn_width and gridn_height must be >= 2: got {gridn_width}, {gridn_height}")
    optimization_inputs, icam = _model_inputs(model)
    lensmodel, intrinsics = model.intrinsics()
    own_u, own_s = uncertainty is None, statistics is None
    u = s = None
    try:
        s = RegionalStatistics(optimization_inputs, gridn_width, gridn_height) if own_s else statistics
        u = ProjectionUncertainty(model) if own_u else uncertainty
        u._open()
        s._open()
        m = lib.lensmodel(lensmodel)
        intr = np.ascontiguousarray(intrinsics, dtype=np.float64)
        mask = np.zeros((gridn_height, gridn_width), dtype=np.uint8)
        unc  = np.zeros((gridn_height, gridn_width)) if return_details else None
        if not lib.lib.mrcal_amd_valid_region_mask(u.handle, s.handle, int(icam), C.byref(m), _ptr(intr), W, H,
                                                   gridn_width, gridn_height, float(distance),
                                                   float(threshold_uncertainty), float(threshold_mean), float(threshold_stdev),
                                                   float(threshold_count), _ptr(mask), _ptr(unc)):
            raise _failed("valid-intrinsics region")
        contour = contour_of_mask(mask, (W, H))
        if not return_details:
            return contour
        mean, stdev, count = s.of_camera(icam)
        return contour, dict(mask=mask, uncertainty=unc, mean=mean, stdev=stdev, count=count)
    finally:
        if own_u and u is not None: u.close()
        if own_s and s is not None: s.close()


def valid_intrinsics_regions(models, parameters=(1, 0.5, 1.5, 3, 0), *, gridn_width=30, gridn_height=None):
    """What mrcal-calibrate-cameras:883-906 does with --valid-intrinsics-region-parameters for the models of ONE solve
    (models[i] is camera i of it): observed_pixel_uncertainty = np.std(measurements_board()); the thresholds
    (parameters[0]*that, parameters[1], parameters[2]*that, parameters[3]) and the distance parameters[4]; every
    model's valid_intrinsics_region() is set. One RegionalStatistics serves all the cameras, one ProjectionUncertainty
    each. A camera whose computation raises gets a warning on stderr and no region. Returns the regions (None where it
    failed)"""
    from .model_analysis import ProjectionUncertainty
    from .utils import measurements_board
    from .cameramodel import _is_poison
    from .resident import Problem
    if len(models) == 0:
        return []
    if len(parameters) != 5:
        raise Exception("parameters must be 5 numbers: uncertainty and stdev factors, mean, count, distance")
    optimization_inputs, _ = _model_inputs(models[0])
    inputs = {k: v for k, v in optimization_inputs.items() if not _is_poison(v)}
    with Problem(**inputs) as p:
        # (one evaluation serves the pixel uncertainty and the statistics)
        statistics = RegionalStatistics(inputs, gridn_width, gridn_height, problem=p)
        x = p.x()
    with statistics:
        observed_pixel_uncertainty = np.std(measurements_board(inputs, x=x).ravel())
        threshold_uncertainty = parameters[0]*observed_pixel_uncertainty
        threshold_mean        = parameters[1]
        threshold_stdev       = parameters[2]*observed_pixel_uncertainty
        threshold_count       = parameters[3]
        distance              = parameters[4]
        regions = []
        for i, model in enumerate(models):
            try:
                gw, gh = statistics.grid_of_camera(model.icam_intrinsics())
                with ProjectionUncertainty(model) as u:
                    region = compute_valid_intrinsics_region(model, threshold_uncertainty, threshold_mean, threshold_stdev,
                                                             threshold_count, distance, gw, gh, uncertainty=u, statistics=statistics)
                model.valid_intrinsics_region(region)
                regions.append(region)
            except Exception as e:
                print(f"WARNING: Couldn't compute valid-intrinsics region for camera {i}. Will continue without. Error: {e}",
                      file=sys.stderr)
                regions.append(None)
    return regions


def _region_of(model):
    r = model.valid_intrinsics_region()
    if r is None:
        return None
    return np.ascontiguousarray(np.asarray(r, dtype=np.float64).reshape(-1, 2))


def is_within_valid_intrinsics_region(q, model):
    """Which of the pixels q (...,2) lie STRICTLY inside the model's valid-intrinsics region: a bool array q.shape[:-1], or
    None if the model has no region. An empty region: all False. A point on an edge or a vertex of the region is outside.
    On the GPU, a lane a point (include/mrcal_amd.h; mrcal.is_within_valid_intrinsics_region())"""
    r = _region_of(model)
    if r is None:
        return None
    q = np.asarray(q, dtype=np.float64)
    if q.shape[-1:] != (2,):
        raise Exception(f"q must have shape (..., 2), got {q.shape}")
    lead = q.shape[:-1]
    qf = np.ascontiguousarray(q.reshape(-1, 2))
    out = np.zeros((qf.shape[0],), dtype=np.uint8)
    if r.shape[0] > 0 and qf.shape[0] > 0:
        lib, api = _handle._libs()
        if not lib.lib.mrcal_amd_valid_region_contains(_ptr(out), _ptr(qf), qf.shape[0], _ptr(r), r.shape[0]):
            raise Exception("is_within_valid_intrinsics_region() failed:" + api._last_error())
    return out.astype(bool).reshape(lead)


def valid_intrinsics_mask(model):
    """The (H,W) uint8 image of is_within_valid_intrinsics_region() at every pixel centre of the model's imager, in one
    launch; None if the model has no region"""
    r = _region_of(model)
    if r is None:
        return None
    W, H = (int(v) for v in model.imagersize())
    out = np.zeros((H, W), dtype=np.uint8)
    if r.shape[0] > 0:
        lib, api = _handle._libs()
        if not lib.lib.mrcal_amd_valid_region_image(_ptr(out), W, H, _ptr(r), r.shape[0]):
            raise Exception("valid_intrinsics_mask() failed:" + api._last_error())
    return out
