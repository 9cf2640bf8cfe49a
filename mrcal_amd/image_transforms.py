"""Reprojecting images from one camera model to another.

    model_pinhole = mrcal_amd.pinhole_model_for_reprojection(model, fit = 'corners')
    mapxy         = mrcal_amd.image_transformation_map(model, model_pinhole, intrinsics_only = True)
    undistorted   = mrcal_amd.transform_image(image, mapxy)

The names, keyword arguments, defaults and exception messages are those of the reference's
mrcal/image_transforms.py. The map and the remap are kernels (csrc/rectification.hip); the two pinhole helpers are
host code. Two deliberate departures from the reference:
  - its OpenCV special case (cv2.initUndistortRectifyMap for OPENCV -> PINHOLE) is not reproduced: the general path
    serves every model, as the reference says it may;
  - transform_image() interpolates exactly, in float32, where cv2.remap() rounds the map to 1/32 pixel first.
"""
import ctypes as C
import numpy as np

from ._cabi import _ptr
from ._images import _image_arguments, _remap_modes, _border_values, _output_array
from .poseutils import compose_Rt, invert_Rt
from .smoothing import antialias_params, antialias_sigma


_FIT_MESSAGE = "fit must be either None or a numpy array or one of ('corners','centers-horizontal','centers-vertical')"


def _unproject_host(q, lensmodel, intrinsics_data):
    """a few pixels through the host's mrcal_unproject(): no GPU needed"""
    from . import _lib, _api
    m = _lib.lensmodel(lensmodel)
    q = np.ascontiguousarray(q, dtype=np.float64)
    intrinsics_data = np.ascontiguousarray(intrinsics_data, dtype=np.float64)
    v = np.zeros(q.shape[:-1] + (3,))
    f = _lib.lib.mrcal_unproject
    if not f(_ptr(v), _ptr(q), q.size//2, C.byref(m), _ptr(intrinsics_data)):
        raise Exception("mrcal_unproject() failed:" + _api._last_error())
    return v


def scale_focal__best_pinhole_fit(model, fit):
    """The focal-length scale that makes a pinhole model with the core of this model just contain the given points

fit: None (the scale is 1); an array (N,2) of pixels of the model that must stay in view; 'corners': the four corners of
the imager; 'centers-horizontal', 'centers-vertical': the midpoints of the two vertical, horizontal edges.
The result goes to pinhole_model_for_reprojection(scale_focal = ...). Reference: mrcal.scale_focal__best_pinhole_fit()"""
    if fit is None: return 1.0
    size = np.array(model.imagersize(), dtype=float)
    last = size - 1.                       # the last pixel in x and in y
    named = {'corners':            ((0., 0.), (0., 1.), (1., 1.), (1., 0.)),
             'centers-horizontal': ((0., .5), (1., .5)),
             'centers-vertical':   ((.5, 0.), (.5, 1.))}
    if type(fit) is np.ndarray:                     pixels = np.asarray(fit, dtype=float).reshape(-1, 2)
    elif type(fit) is str and fit in named:         pixels = np.array(named[fit])*last
    else:                                           raise Exception(_FIT_MESSAGE)

    lensmodel, intrinsics_data = model.intrinsics()
    focal, centre = np.asarray(intrinsics_data[:2], dtype=float), np.asarray(intrinsics_data[2:4], dtype=float)
    v = _unproject_host(pixels, lensmodel, intrinsics_data)
    # A pinhole camera with k times this focal length puts the point at k focal xy/z + centre. It stays on the imager
    # while k xy/z lies between -centre/focal and (last - centre)/focal: each coordinate of each point bounds k by
    # the edge on ITS side of the centre, and the smallest bound is the fit (1e6 if nothing bounds it)
    xy = v[:, :2]/v[:, 2:]
    edge = np.where(xy > 0, (last - centre)/focal, -centre/focal)
    with np.errstate(divide="ignore", invalid="ignore"):
        bounds = edge/xy
    bounds = bounds[np.isfinite(bounds)]          # (a coordinate on the optical axis bounds nothing)
    return float(min(1e6, bounds.min())) if bounds.size else 1e6


def pinhole_model_for_reprojection(model_from, fit=None, *, scale_focal=None, scale_image=None):
    """A LENSMODEL_PINHOLE cameramodel with the core, the pose and the imager of model_from, to reproject its images to

fit: as in scale_focal__best_pinhole_fit(), which then gives the focal-length scale; or scale_focal directly (at most
one of the two). scale_image: scales the imager, the centre of the imager keeping its direction.
Reference: mrcal.pinhole_model_for_reprojection()"""
    from .cameramodel import cameramodel
    if scale_focal is None:
        if fit is not None:
            if isinstance(fit, np.ndarray):
                if fit.shape[-1] != 2:
                    raise Exception("'fit' is an array, so it must have shape (...,2)")
                fit = fit.reshape(-1, 2)
            elif isinstance(fit, str) and fit in ('corners', 'centers-horizontal', 'centers-vertical'):
                pass
            else:
                raise Exception("'fit' must be an array of shape (...,2) or one of ('corners','centers-horizontal','centers-vertical')")
        scale_focal = scale_focal__best_pinhole_fit(model_from, fit)
    else:
        if fit is not None:
            raise Exception("At most one of 'scale_focal' and 'fit' may be non-None")

    lensmodel, intrinsics_data = model_from.intrinsics()
    focal  = np.array(intrinsics_data[:2], dtype=float)*scale_focal
    centre = np.array(intrinsics_data[2:4], dtype=float)
    imagersize = [int(x) for x in model_from.imagersize()]
    if scale_image is not None:
        # Pixel q covers [q - 1/2, q + 1/2]: measured from the imager's corner a point is at q + 1/2, and that is what
        # scales with the image. So does the focal length
        imagersize = [round(n*scale_image) for n in imagersize]
        focal  = focal*scale_image
        centre = (centre + 0.5)*scale_image - 0.5
    return cameramodel(intrinsics=('LENSMODEL_PINHOLE', np.concatenate((focal, centre))), rt_cam_ref=model_from.rt_cam_ref(),
                       imagersize=imagersize)


def image_transformation_map(model_from, model_to, *, intrinsics_only=False, distance=None, plane_n=None, plane_d=None,
                             mask_valid_intrinsics_region_from=False):
    """float32 (H_to, W_to, 2): for every pixel of model_to's imager, where model_from sees the same thing: what
transform_image(image_from, mapxy) takes to produce the image model_to would have seen

Three modes. intrinsics_only: the poses are ignored. Otherwise the relative pose counts: by default only its rotation
(the scene is at infinity); distance: every pixel looks at a point that far from model_to; plane_n, plane_d: at the
plane {x: plane_n . x = plane_d} in model_from's coordinates (the homography of Faugeras and Lustman).
mask_valid_intrinsics_region_from: pixels that land outside model_from's valid-intrinsics region are -1.
Reference: mrcal.image_transformation_map()"""
    from . import _lib, _api
    if (plane_n is None and plane_d is not None) or (plane_n is not None and plane_d is None):
        raise Exception("plane_n and plane_d should both be None or neither should be None")
    if plane_n is not None and intrinsics_only:
        raise Exception("We're looking at remapping a plane (plane_d, plane_n are not None), so intrinsics_only should be False")
    if distance is not None and (plane_n is not None or intrinsics_only):
        raise Exception("'distance' makes sense only without plane_n/plane_d and without intrinsics_only")

    # p_from = A (v_to, or v_to/|v_to| distance) + t
    A, t, d = np.eye(3), np.zeros(3), 0.0
    if not intrinsics_only:
        Rt_to_from = compose_Rt(model_to.Rt_cam_ref(), model_from.Rt_ref_cam())
        if plane_n is not None:
            plane_n = np.asarray(plane_n, dtype=float)
            if plane_n.shape != (3,):
                raise Exception(f"plane_n must have shape (3,), got {plane_n.shape}")
            A = np.linalg.inv(float(plane_d)*Rt_to_from[:3, :] + np.outer(Rt_to_from[3, :], plane_n))
        elif distance is not None:
            if not float(distance) > 0:
                raise Exception("'distance' must be > 0")
            Rt_from_to = invert_Rt(Rt_to_from)
            A, t, d = Rt_from_to[:3, :], Rt_from_to[3, :], float(distance)
        else:
            A = Rt_to_from[:3, :].T

    region, Nregion = None, 0
    if mask_valid_intrinsics_region_from:
        region = model_from.valid_intrinsics_region()
        if region is None:
            raise Exception("mask_valid_intrinsics_region_from is True, but model_from has no valid-intrinsics region")
        region = np.ascontiguousarray(region, dtype=np.float64).reshape(-1, 2)
        Nregion = region.shape[0]
        if Nregion == 0: region = np.zeros((1, 2))      # valid nowhere

    lensmodel_from, intrinsics_from = model_from.intrinsics()
    lensmodel_to,   intrinsics_to   = model_to.intrinsics()
    m_from, m_to = _lib.lensmodel(lensmodel_from), _lib.lensmodel(lensmodel_to)
    intrinsics_from = np.ascontiguousarray(intrinsics_from, dtype=np.float64)
    intrinsics_to   = np.ascontiguousarray(intrinsics_to,   dtype=np.float64)
    W_to, H_to = (int(x) for x in model_to.imagersize())
    imagersize_to = (C.c_uint*2)(W_to, H_to)
    A, t = np.ascontiguousarray(A, dtype=np.float64), np.ascontiguousarray(t, dtype=np.float64)
    mapxy = np.zeros((H_to, W_to, 2), dtype=np.float32)
    f = _lib.lib.mrcal_amd_image_transformation_map
    if not f(_ptr(mapxy), C.addressof(m_from), _ptr(intrinsics_from), C.addressof(m_to), _ptr(intrinsics_to),
             C.addressof(imagersize_to), _ptr(A), _ptr(t), d, _ptr(region), Nregion):
        raise Exception("image_transformation_map() failed:" + _api._last_error())
    return mapxy


def transform_image(image, mapxy, *, out=None, borderMode=None, borderValue=0, interpolation=None, antialias=None):
    """out[i,j] = image at the pixel mapxy[i,j] = (x,y): (H,W) or (H,W,3), like the image

image: uint8, uint16 or float32, (H_in, W_in) or (H_in, W_in, 3). mapxy: float32 (H, W, 2), from
image_transformation_map() or rectification_maps(). interpolation: None, 'linear' or 1: bilinear; 'nearest' or 0.
borderMode: None, 'constant' or 0: a neighbour outside the image counts as borderValue (a scalar or a value per
channel), and so does a pixel whose map entry is not finite; 'transparent' or 5: a pixel with any neighbour outside
keeps what 'out' had (zeros if no 'out' is given). Integer images are rounded to nearest and saturate.
The interpolation is exact bilinear interpolation in float32: cv2.remap(), which the reference calls, rounds the map
to 1/32 pixel first, and that is not imitated. Reference: mrcal.transform_image()
antialias: None, 'auto', a sigma or (sigma_x, sigma_y): the image (grayscale, uint8 or uint16 then) is filtered on the
device between its upload and the remap (smooth_gaussian()), the same bits as filtering it first. 'auto':
antialias_sigma(mapxy); where that is 0, and for None, nothing of it runs"""
    from . import _lib, _api
    if not isinstance(image, np.ndarray): raise Exception("'image' must be a numpy array")
    if not isinstance(mapxy, np.ndarray): raise Exception("'mapxy' must be a numpy array")
    a, w, h, channels, dtype = _image_arguments(image)
    if mapxy.dtype != np.float32 or mapxy.ndim != 3 or mapxy.shape[2] != 2 or mapxy.size == 0:
        raise Exception(f"'mapxy' must be a float32 array of shape (H,W,2), got {mapxy.dtype} {mapxy.shape}")
    border, interp = _remap_modes(borderMode, interpolation)
    bv = _border_values(borderValue, channels)
    H, W = mapxy.shape[:2]
    o, ret = _output_array(out, (H, W) if channels == 1 else (H, W, 3), a.dtype, border == 5)
    m = np.ascontiguousarray(mapxy)
    smooth = antialias_params(antialias, lambda: antialias_sigma(mapxy), (image,))
    if smooth is None:
        ok = _lib.lib.mrcal_amd_transform_image(_ptr(o), _ptr(a), w, h, channels, dtype, _ptr(m), W, H, interp, border, _ptr(bv))
    else:
        ok = _lib.lib.mrcal_amd_transform_image_smoothed(_ptr(o), _ptr(a), w, h, channels, dtype, _ptr(m), W, H, interp, border,
                                                         _ptr(bv), C.addressof(smooth))
    if not ok:
        raise Exception("transform_image() failed:" + _api._last_error())
    if ret is not o: ret[...] = o
    return ret
