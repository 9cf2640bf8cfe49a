"""Stereo rectification: the rectified system, its maps, ranges from disparities.

    models_rectified = mrcal_amd.rectified_system(models, az_fov_deg = 90, el_fov_deg = 50)
    maps             = mrcal_amd.rectification_maps(models, models_rectified)
    images_rectified = [mrcal_amd.transform_image(i, m) for i, m in zip(images, maps)]
    ranges           = mrcal_amd.stereo_range(disparity, models_rectified, disparity_scale = 16)

    with mrcal_amd.Rectification(models, models_rectified) as r:       # the maps are made once and stay on the device
        for image0, image1 in frames:
            rect0, rect1 = r.rectify(image0, image1)
            ranges       = r.range(matcher(rect0, rect1), disparity_scale = 16)
            # or, the rectified images staying on the device:
            ranges       = r.range(r.disparity(image0, image1, disparity_max = 128), disparity_scale = 16)

    disparity = mrcal_amd.stereo_matching_sgm(rect0, rect1, disparity_max = 128)      # int16, scaled by 16

    with mrcal_amd.StereoMatcherSGM(rect0.shape, rect0.dtype, disparity_max = 128) as sgm:     # the buffers are made once
        disparity = sgm.match(rect0, rect1)

    # cv2's speckle filter, on request: as a stage of the matcher (also of StereoMatcherSGM and Rectification.disparity()) ...
    disparity = mrcal_amd.stereo_matching_sgm(rect0, rect1, disparity_max = 128, speckle_window_size = 200, speckle_range = 2)
    # ... or on a disparity image from anywhere
    disparity = mrcal_amd.filter_speckles(disparity, new_value = -16, max_speckle_size = 200, max_diff = 32)

    # the points themselves, compacted and coloured from camera 0: only the valid ones cross to the host
    points, color, index = mrcal_amd.stereo_point_cloud(disparity, models_rectified, models = models, image0 = image0,
                                                        disparity_scale = 16, dtype = np.float32)
    mrcal_amd.write_point_cloud_as_ply("points.ply", points, color = color)
    with mrcal_amd.Rectification(models, models_rectified) as r:       # ... from the image pair, everything in between on the device
        points, color, index = r.point_cloud_of_images(image0, image1, disparity_max = 128, dtype = np.float32)

    q1, diagnostics = mrcal_amd.match_feature(image0, image1, q0, H10 = H10, search_radius1 = 200, template_size1 = 41)

    with mrcal_amd.FeatureMatcher(image0, image1) as matcher:          # both images are uploaded once
        q1, status = matcher.match(q0, H10 = H10, search_radius1 = 200, template_size1 = 41)        # q0 (N,2)

The names, keyword arguments, defaults, return shapes and exception messages are those of the reference's
mrcal/stereo.py. rectified_system() and rectified_resolution() are host code (csrc/stereo_geometry.cpp) and need no
GPU; the maps, the remap and the ranges are kernels (csrc/rectification.hip), the template matching of match_feature()
is csrc/match_feature.hip, the dense matching of stereo_matching_sgm() is csrc/stereo_sgm.hip, the connected-component
labelling of filter_speckles() is csrc/speckle_filter.hip, the compaction of stereo_point_cloud() is
csrc/point_cloud.hip, and there is no CPU fallback for them.
Out of scope: image file I/O, cv2.StereoSGBM's and libelas's own pixel-for-pixel output, visualization, LONLAT rectification (which the reference's
rectified_system() refuses too).
"""
import ctypes as C
import numpy as np

from . import _handle
from ._cabi import _ptr
from ._handle import Handle, _failed
from ._images import MAX_PIXELS, _image_arguments, _output_array
from .poseutils import compose_Rt
from .equalization import equalization_params, _EqualizeParams
from .smoothing import antialias_params, antialias_sigma


class _Point2(C.Structure):
    _fields_ = [("x", C.c_double), ("y", C.c_double)]


def _rectification_model_type(lib, rectification_model):
    return lib.lensmodel(rectification_model).type


def rectified_resolution(model0, *, az_fov_deg, el_fov_deg, az0_deg, el0_deg, R_cam0_rect0,
                         pixels_per_deg_az=-1., pixels_per_deg_el=-1., rectification_model='LENSMODEL_LATLON'):
    """The resolution of the rectified system: (pixels_per_deg_az, pixels_per_deg_el)

A value > 0 is used as given. A value < 0 scales the resolution model0 has at the centre (az0_deg, el0_deg) of the
rectified view: -1 keeps it, -0.5 halves it. For LENSMODEL_LATLON and LENSMODEL_LONLAT the result is then adjusted so
that the field of view is a whole number of pixels; for LENSMODEL_PINHOLE it is the resolution at the centre.
Reference: mrcal.rectified_resolution(), mrcal_rectified_resolution()"""
    lib, api = _handle._libs()
    lensmodel, intrinsics = model0.intrinsics()
    m = lib.lensmodel(lensmodel)
    intrinsics = np.ascontiguousarray(intrinsics, dtype=np.float64)
    R = np.ascontiguousarray(R_cam0_rect0, dtype=np.float64)
    if R.shape != (3, 3):
        raise Exception(f"R_cam0_rect0 must have shape (3,3), got {R.shape}")
    az, el = C.c_double(pixels_per_deg_az), C.c_double(pixels_per_deg_el)
    fov, center = _Point2(az_fov_deg, el_fov_deg), _Point2(az0_deg, el0_deg)
    if not lib.lib.mrcal_rectified_resolution(C.addressof(az), C.addressof(el), C.addressof(m), _ptr(intrinsics), C.addressof(fov),
                                              C.addressof(center), _ptr(R), _rectification_model_type(lib, rectification_model)):
        raise _failed("mrcal_rectified_resolution()")
    return az.value, el.value


def rectified_system(models, *, az_fov_deg, el_fov_deg, az0_deg=None, el0_deg=0, az_edge_margin_deg=10.,
                     pixels_per_deg_az=-1., pixels_per_deg_el=-1., rectification_model='LENSMODEL_LATLON',
                     return_metadata=False):
    """The two rectified models of a stereo pair: LENSMODEL_LATLON (the default) or LENSMODEL_PINHOLE cameramodels with
identical intrinsics, the same orientation, and camera 1 a baseline away along the rectified +x

models: the two cameramodels. az_fov_deg, el_fov_deg: the field of view of the rectified images. az0_deg, el0_deg: its
centre; az0_deg = None: the mean forward direction of the two cameras, shifted if need be so that the view stays
az_edge_margin_deg away from the baseline. pixels_per_deg_az, pixels_per_deg_el: as for rectified_resolution().
return_metadata: also a dict with az_fov_deg, el_fov_deg, az0_deg, el0_deg, pixels_per_deg_az, pixels_per_deg_el,
baseline as they ended up. Runs on the host: no GPU is needed.
Reference: mrcal.rectified_system(), mrcal_rectified_system2()"""
    from .cameramodel import cameramodel
    lib, api = _handle._libs()
    if len(models) != 2:
        raise Exception("I need exactly 2 camera models")
    for m in models:
        lensmodel, intrinsics = m.intrinsics()
        # (the one noncentral model)
        if lensmodel.startswith("LENSMODEL_CAHVORE") and np.any(np.asarray(intrinsics)[-3:] != 0):
            raise Exception("Stereo rectification is only possible with a central projection. Please centralize your models. This is CAHVORE, so set E=0 to centralize. This will ignore all noncentral effects near the lens")

    lensmodel, intrinsics = models[0].intrinsics()
    m = lib.lensmodel(lensmodel)
    intrinsics = np.ascontiguousarray(intrinsics, dtype=np.float64)
    rt0 = np.ascontiguousarray(models[0].rt_cam_ref(), dtype=np.float64)
    rt1 = np.ascontiguousarray(models[1].rt_cam_ref(), dtype=np.float64)
    imagersize = (C.c_uint*2)()
    fxycxy, rt_rect0_ref = np.zeros(4), np.zeros(6)
    baseline = C.c_double(0)
    az, el = C.c_double(pixels_per_deg_az), C.c_double(pixels_per_deg_el)
    autodetect = az0_deg is None
    fov, center = _Point2(az_fov_deg, el_fov_deg), _Point2(0. if autodetect else az0_deg, el0_deg)
    if not lib.lib.mrcal_rectified_system2(
            C.addressof(imagersize), _ptr(fxycxy), _ptr(rt_rect0_ref), C.addressof(baseline),
            C.addressof(az), C.addressof(el), C.addressof(fov), C.addressof(center),
            float(az_edge_margin_deg), C.addressof(m), _ptr(intrinsics), _ptr(rt0), _ptr(rt1),
            _rectification_model_type(lib, rectification_model), autodetect, False, False, False):
        raise _failed("mrcal_rectified_system2()")

    # rect1 has the orientation of rect0, and its origin at camera 1: rt_rect0_rect1 = (0,0,0, baseline,0,0)
    rt_rect1_ref = rt_rect0_ref.copy()
    rt_rect1_ref[3] -= baseline.value
    Naz, Nel = int(imagersize[0]), int(imagersize[1])
    models_rectified = tuple(cameramodel(intrinsics=(rectification_model, fxycxy.copy()), imagersize=(Naz, Nel), rt_cam_ref=rt)
                             for rt in (rt_rect0_ref, rt_rect1_ref))
    if not return_metadata:
        return models_rectified
    return models_rectified, dict(az_fov_deg=fov.x, el_fov_deg=fov.y, az0_deg=center.x, el0_deg=center.y,
                                  pixels_per_deg_az=az.value, pixels_per_deg_el=el.value, baseline=baseline.value)


def _validate_models_rectified(models_rectified):
    """what rectified_system() returns: two LENSMODEL_LATLON or LENSMODEL_PINHOLE cameras with identical intrinsics and
    orientation, the second a translation along the rectified +x away"""
    if len(models_rectified) != 2:
        raise Exception(f"Must have received exactly two models. Got {len(models_rectified)} instead")
    intrinsics = [m.intrinsics() for m in models_rectified]
    Rt01 = compose_Rt(models_rectified[0].Rt_cam_ref(), models_rectified[1].Rt_ref_cam())
    if not ((intrinsics[0][0] == 'LENSMODEL_LATLON'  and intrinsics[1][0] == 'LENSMODEL_LATLON') or
            (intrinsics[0][0] == 'LENSMODEL_PINHOLE' and intrinsics[1][0] == 'LENSMODEL_PINHOLE')):
        raise Exception(f"Expected two models with the same  'LENSMODEL_LATLON' or 'LENSMODEL_PINHOLE' but got {intrinsics[0][0]} and {intrinsics[1][0]}")
    d = np.asarray(intrinsics[0][1]) - np.asarray(intrinsics[1][1])
    if np.dot(d, d) > 1e-6:
        raise Exception("The two rectified models MUST have the same intrinsics values")
    if tuple(int(x) for x in models_rectified[0].imagersize()) != tuple(int(x) for x in models_rectified[1].imagersize()):
        raise Exception("The two rectified models MUST have the same imager size")
    costh = (np.trace(Rt01[:3, :]) - 1.) / 2.
    if costh < 0.999999:
        raise Exception("The two rectified models MUST have the same relative rotation")
    if np.dot(Rt01[3, 1:], Rt01[3, 1:]) > 1e-9:
        raise Exception("The two rectified models MUST have a translation ONLY in the +x rectified direction")


def _baseline(models_rectified):
    Rt01 = compose_Rt(models_rectified[0].Rt_cam_ref(), models_rectified[1].Rt_ref_cam())
    return float(np.linalg.norm(Rt01[3, :]))


class Rectification(Handle):
    """The rectification of a stereo pair, resident: both maps are made on the device once and stay there.

    models: the two cameramodels; models_rectified: what rectified_system() returned for them.
      .maps()                          rectification_maps(): float32 (2, Nel, Naz, 2), the same bits
      .rectify(image0, image1)         the two rectified images; the maps do not cross to the host and back
      .disparity(image0, image1, ...)  stereo_matching_sgm() of the rectified images, which stay on the device
      .range(disparity, ...)           stereo_range() of a dense (Nel, Naz) disparity
      .point_cloud(disparity, ...)     stereo_point_cloud() of it: the kept points, their colours and pixel indices
      .point_cloud_of_images(image0, image1, ...)   the same from the image pair; the rectified images and the
                                       disparities stay on the device
      .point_cloud_stage_milliseconds()  how long the mask, the scan and the scatter of the last cloud took
    rectify(), disparity() and point_cloud_of_images() take equalization = None | 'clahe' | 'stretch',
    clahe_clip_limit = 8.0, clahe_tiles = (8,8): each raw image (grayscale, uint8 or uint16) is equalized on the device
    between its upload and the remap (equalize_clahe(), equalize_stretch()), the same bits as equalizing it first.
    With 'stretch' the rectified images are uint8. None: nothing of it runs.
    The same three take antialias = None | 'auto' | sigma | (sigma_x, sigma_y): each raw image (grayscale, uint8 or
    uint16) is filtered on the device (smooth_gaussian()) after its upload and its equalization and before the remap,
    the same bits as filtering it first. 'auto': antialias_sigma() of the two maps, the larger; where that is 0, and for
    None, nothing of it runs. The colours of a point cloud are not filtered"""

    _destroy = "mrcal_amd_rectification_destroy"

    def __init__(self, models, models_rectified):
        _validate_models_rectified(models_rectified)
        if len(models) != 2:
            raise Exception("I need exactly 2 camera models")
        lib, _ = _handle._libs()
        self._models, self._models_rectified = tuple(models), tuple(models_rectified)
        self.Naz, self.Nel = (int(x) for x in models_rectified[0].imagersize())
        args, keep = [], []
        for m in models:
            lensmodel, intrinsics = m.intrinsics()
            lm = lib.lensmodel(lensmodel)
            intrinsics = np.ascontiguousarray(intrinsics, dtype=np.float64)
            r = np.ascontiguousarray(m.rt_cam_ref()[:3], dtype=np.float64)
            keep += [lm, intrinsics, r]
            args += [C.addressof(lm), _ptr(intrinsics), _ptr(r)]
        rectification_model, fxycxy = models_rectified[0].intrinsics()
        fxycxy = np.ascontiguousarray(fxycxy, dtype=np.float64)
        imagersize = (C.c_uint*2)(self.Naz, self.Nel)
        r_rect0_ref = np.ascontiguousarray(models_rectified[0].rt_cam_ref()[:3], dtype=np.float64)
        self._create("rectification_maps()", "mrcal_amd_rectification_create", *args,
                     _rectification_model_type(lib, rectification_model), _ptr(fxycxy), C.addressof(imagersize),
                     _ptr(r_rect0_ref), _baseline(models_rectified))

    # what the handle last received of the two settings, as plain values; None: nothing, which a new handle does by itself
    _sent = (None, None)
    _antialias_auto_sigma = None

    def _antialias_auto(self):
        """antialias_sigma() of the two maps, the larger: computed once"""
        if self._antialias_auto_sigma is None:
            maps = self.maps()
            self._antialias_auto_sigma = max(antialias_sigma(maps[0]), antialias_sigma(maps[1]))
        return self._antialias_auto_sigma

    def _prepare(self, eq, smooth):
        """What the calls that follow do to their raw images between the upload and the remap: eq, smooth: what
        equalization_params() and antialias_params() made of the keywords, after every refusal; None: nothing of it.
        Each is sent only where it differs from what the handle last received"""
        settings = (None if eq is None else (eq.method, eq.clip_limit, eq.tiles_x, eq.tiles_y),
                    None if smooth is None else (smooth.sigma_x, smooth.sigma_y))
        if settings[0] != self._sent[0]:
            p = eq if eq is not None else _EqualizeParams(0, 8.0, 8, 8)
            self._call("equalize()", "mrcal_amd_rectification_set_equalization", C.addressof(p))
            self._sent = (settings[0], self._sent[1])
        if settings[1] != self._sent[1]:
            self._call("smooth()", "mrcal_amd_rectification_set_antialias", None if smooth is None else C.addressof(smooth))
            self._sent = settings

    @staticmethod
    def _matcher_pair(image0, image1):
        """a grayscale pair of one dtype for the matcher -> its dtype code"""
        for image in (image0, image1):
            if not isinstance(image, np.ndarray) or image.ndim != 2 or image.size == 0:
                raise Exception("stereo_matching_sgm() accepts ONLY grayscale images of shape (H,W)")
        if image0.dtype != image1.dtype:
            raise Exception(f"stereo_matching_sgm(): image0 and image1 must have the same dtype, got {image0.dtype} and {image1.dtype}")
        return _SGM_DTYPES[_sgm_dtype(image0.dtype)]

    def maps(self):
        self._open()
        maps = np.zeros((2, self.Nel, self.Naz, 2), dtype=np.float32)
        self._call("rectification_maps()", "mrcal_amd_rectification_maps", _ptr(maps))
        return maps

    def rectify(self, image0, image1, out=None, *, equalization=None, clahe_clip_limit=8.0, clahe_tiles=(8, 8), antialias=None):
        """(image0 rectified, image1 rectified): linear interpolation, 0 outside the images. out: the two arrays to fill.
        equalization, antialias: of the raw images, on the device, before the remap (grayscale, uint8 or uint16, then)"""
        self._open()
        eq, dtype_out = equalization_params(equalization, clahe_clip_limit, clahe_tiles, (image0, image1))
        a0, w0, h0, c0, t0 = _image_arguments(image0, "image0")
        a1, w1, h1, c1, t1 = _image_arguments(image1, "image1")
        if (c0, t0) != (c1, t1):
            raise Exception("image0 and image1 must have the same dtype and number of channels")
        shape = (self.Nel, self.Naz) if c0 == 1 else (self.Nel, self.Naz, 3)
        if out is not None and len(out) != 2:
            raise Exception("'out' must be a pair of arrays")
        (o0, r0), (o1, r1) = (_output_array(None if out is None else out[i], shape, a0.dtype if dtype_out is None else dtype_out, False)
                              for i in (0, 1))
        self._prepare(eq, antialias_params(antialias, self._antialias_auto, (image0, image1)))
        self._call("rectify()", "mrcal_amd_rectification_rectify", _ptr(o0), _ptr(o1), _ptr(a0), w0, h0, _ptr(a1), w1, h1,
                   c0, t0, 1, 0, None)
        if r0 is not o0: r0[...] = o0
        if r1 is not o1: r1[...] = o1
        return r0, r1

    def range(self, disparity, *, disparity_scale=1, disparity_min=None, disparity_max=None,
              disparity_scaled_min=None, disparity_scaled_max=None):
        """stereo_range(disparity, models_rectified, ...) of a dense (Nel, Naz) disparity"""
        self._open()
        return stereo_range(disparity, self._models_rectified, disparity_scale=disparity_scale,
                            disparity_min=disparity_min, disparity_max=disparity_max,
                            disparity_scaled_min=disparity_scaled_min, disparity_scaled_max=disparity_scaled_max,
                            _rectification=self)

    def disparity(self, image0, image1, *, speckle_window_size=0, speckle_range=0,
                  equalization=None, clahe_clip_limit=8.0, clahe_tiles=(8, 8), antialias=None, **params):
        """stereo_matching_sgm(*rectify(image0, image1), **params), the same bits: int16 (Nel, Naz). The rectified images
        are made and matched on the device and do not cross to the host. image0, image1: grayscale, uint8 or uint16.
        speckle_window_size > 0: the disparity image is filtered there too (filter_speckles()).
        equalization, antialias: of the raw images, there too, before the remap"""
        self._open()
        speckle = _speckle_keywords(speckle_window_size, speckle_range)
        p = _sgm_params(**params)
        dtype = self._matcher_pair(image0, image1)
        eq, _ = equalization_params(equalization, clahe_clip_limit, clahe_tiles, (image0, image1))
        self._prepare(eq, antialias_params(antialias, self._antialias_auto, (image0, image1)))
        a0, a1 = np.ascontiguousarray(image0), np.ascontiguousarray(image1)
        out = np.zeros((self.Nel, self.Naz), dtype=np.int16)
        images = (_ptr(a0), a0.shape[1], a0.shape[0], _ptr(a1), a1.shape[1], a1.shape[0], dtype, C.addressof(p))
        if speckle[0] == 0:             # (no filter: the entry point without it)
            self._call("stereo_matching_sgm()", "mrcal_amd_rectification_disparity", *images, _ptr(out))
        else:
            self._call("stereo_matching_sgm()", "mrcal_amd_rectification_disparity_filtered", *images, *speckle, _ptr(out))
        return out

    def point_cloud(self, disparity, *, image0=None, disparity_scale=1, disparity_min=None, disparity_max=None,
                        disparity_scaled_min=None, disparity_scaled_max=None, range_min=None, range_max=None,
                        frame='ref', dtype=np.float64):
        """stereo_point_cloud(disparity, models_rectified, models = models, ...) of a dense (Nel, Naz) disparity on the host:
        (points, color, index), the same bits. The map of camera 0 is the one that lies on the device"""
        self._open()
        image = _cloud_image(image0, "image0", self._models)
        d, scale, dmin, dmax = _cloud_disparity(disparity, (self.Nel, self.Naz), disparity_scale, disparity_min, disparity_max,
                                                disparity_scaled_min, disparity_scaled_max)
        rmin, rmax, Rt, float32 = _cloud_frame(self._models_rectified, self._models, range_min, range_max, frame, dtype)
        p, keep = _cloud_params(scale, dmin, dmax, rmin, rmax, Rt, float32, image)
        N = C.c_int(0)
        self._call("stereo_point_cloud()", "mrcal_amd_rectification_point_cloud", _ptr(d), C.addressof(p), C.addressof(N))
        return _cloud_read(self, "mrcal_amd_rectification_point_cloud_read", N.value, float32, image)

    def point_cloud_of_images(self, image0, image1, *, color_image=None, frame='ref', dtype=np.float64,
                                  range_min=None, range_max=None, speckle_window_size=0, speckle_range=0,
                                  equalization=None, clahe_clip_limit=8.0, clahe_tiles=(8, 8), antialias=None, **sgm_params):
        """point_cloud(disparity(image0, image1, ...), image0 = color_image or image0, disparity_scale = 16,
        disparity_min = disparity_min, ...), the same bits: (points, color, index). The pair is rectified, matched, on
        request filtered, and made a cloud of on the device: neither the rectified images nor the disparities cross to the
        host. image0, image1: grayscale, uint8 or uint16. color_image: the image of camera 0 the colours come from, gray or
        BGR, of its imager size; None: image0. A negative disparity_min is refused: stereo_range()'s cast to uint16 has no
        meaning for negative disparities. equalization: of the raw images, on the device, before the remap; the colours
        are then those of the EQUALIZED image0 (as in the reference's mrcal-stereo), unless a color_image is given,
        which is used as it is. antialias: of the raw images, after the equalization; the colours are NOT filtered: they
        are those of image0 as it was before the filter"""
        self._open()
        speckle = _speckle_keywords(speckle_window_size, speckle_range)
        p_sgm = _sgm_params(**sgm_params)
        if p_sgm.disparity_min < 0:
            raise Exception(f"stereo_point_cloud(): disparity_min must not be negative: the cast to uint16 of stereo_range() has no meaning for negative disparities. Got {p_sgm.disparity_min}")
        sgm_dtype = self._matcher_pair(image0, image1)
        eq, dtype_equalized = equalization_params(equalization, clahe_clip_limit, clahe_tiles, (image0, image1))
        smooth = antialias_params(antialias, self._antialias_auto, (image0, image1))
        a0, a1 = np.ascontiguousarray(image0), np.ascontiguousarray(image1)
        # (image0 as its own colour image: the SAME array, which the library then takes equalized, where it lies)
        image = _cloud_image(a0 if color_image is None else color_image, "image0" if color_image is None else "color_image", self._models)
        rmin, rmax, Rt, float32 = _cloud_frame(self._models_rectified, self._models, range_min, range_max, frame, dtype)
        if eq is not None and color_image is not None and image[0].ctypes.data == a0.ctypes.data:
            image = (image[0].copy(),) + tuple(image[1:])                           # (given: used as it is, also where it is image0)
        p, keep = _cloud_params(0, 0, 0, rmin, rmax, Rt, float32, image)       # (the disparity fields: the library's, from the matcher's)
        if eq is not None and color_image is None and dtype_equalized != a0.dtype:
            image = (np.zeros((0,), dtype=dtype_equalized),) + tuple(image[1:])      # (what the colours are read into: 'stretch' makes uint8)
        self._prepare(eq, smooth)           # (after every refusal)
        N = C.c_int(0)
        self._call("stereo_point_cloud()", "mrcal_amd_rectification_point_cloud_of_images", _ptr(a0), a0.shape[1], a0.shape[0],
                   _ptr(a1), a1.shape[1], a1.shape[0], sgm_dtype, C.addressof(p_sgm), *speckle, C.addressof(p), C.addressof(N))
        return _cloud_read(self, "mrcal_amd_rectification_point_cloud_read", N.value, float32, image)

    def point_cloud_stage_milliseconds(self):
        """how long the mask, the scan and the scatter of the last cloud took on the device"""
        self._open()
        return _cloud_stage_milliseconds(self, "mrcal_amd_rectification_point_cloud_stage_milliseconds")

    def _range_dense(self, disparity_scaled, disparity_scale, dmin, dmax):
        d = np.ascontiguousarray(disparity_scaled, dtype=np.uint16)
        r = np.zeros(d.shape, dtype=np.float64)
        self._call("stereo_range()", "mrcal_amd_rectification_range", _ptr(r), _ptr(d), int(disparity_scale), int(dmin), int(dmax))
        return r


def rectification_maps(models, models_rectified):
    """float32 (2, Nel, Naz, 2): for every pixel of the rectified images, where to look it up in the image of camera 0
and of camera 1: maps[i] is what transform_image(image_i, maps[i]) takes. The one-shot form of
Rectification(models, models_rectified).maps(). Reference: mrcal.rectification_maps(), mrcal_rectification_maps()"""
    with Rectification(models, models_rectified) as r:
        return r.maps()


class _Image(C.Structure):
    """mrcal_image_uint16_t, mrcal_image_double_t: the stride in bytes"""
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("stride", C.c_int), ("data", C.c_void_p)]


def stereo_range(disparity, models_rectified, *, disparity_scale=1, disparity_min=None, disparity_scaled_min=None,
                 disparity_max=None, disparity_scaled_max=None, qrect0=None, _rectification=None):
    """Ranges from disparities; 0 where the disparity is invalid (<= 0, below the minimum, above the maximum) or the
range is not finite

Dense form (qrect0 is None): disparity is an (Nel, Naz) image from a stereo matcher, cast to uint16 as the reference
does (an int16 image: the maximum defaults to 0x7FFF, so that its negative "invalid" marks stay invalid); the true
disparity in pixels is disparity / disparity_scale. Sparse form: qrect0 (...,2), the pixels in the rectified image of
camera 0 the disparities (...) belong to; they broadcast, and a scalar disparity gives a scalar.
disparity_min/max are in pixels, disparity_scaled_min/max in the units of the given disparity.
Reference: mrcal.stereo_range(), mrcal_stereo_range_dense(), mrcal_stereo_range_sparse()"""
    if _rectification is None: _validate_models_rectified(models_rectified)     # (a Rectification has)
    if disparity_min is not None and disparity_scaled_min is not None and disparity_min != disparity_scaled_min:
        raise Exception("disparity_min and disparity_scaled_min may not both be given")
    if disparity_max is not None and disparity_scaled_max is not None and disparity_max != disparity_scaled_max:
        raise Exception("disparity_max and disparity_scaled_max may not both be given")
    # an int16 image marks invalid pixels with negative values, which the cast to uint16 turns into large ones
    if disparity_max is None and disparity_scaled_max is None and isinstance(disparity, np.ndarray) and disparity.dtype == np.int16:
        disparity_scaled_max = 0x7FFF
    # Each bound may come in pixels or in the units of the given disparity; the dense kernel wants the latter, the
    # sparse one the former. Absent: 0, and the largest value the type holds
    dense = qrect0 is None
    def bound(pixels, scaled, absent):
        if dense: return scaled if scaled is not None else absent if pixels is None else pixels*disparity_scale
        return pixels if pixels is not None else absent if scaled is None else scaled/disparity_scale
    lowest  = bound(disparity_min, disparity_scaled_min, 0)
    highest = bound(disparity_max, disparity_scaled_max, 0xFFFF if dense else np.finfo(float).max)
    if dense: disparity_scaled_min, disparity_scaled_max = lowest, highest
    else:     disparity_min, disparity_max = lowest, highest

    is_scalar = np.ndim(disparity) == 0
    disparity = np.atleast_1d(np.asarray(disparity))
    lib, api = _handle._libs()
    rectification_model, fxycxy = models_rectified[0].intrinsics()
    fxycxy = np.ascontiguousarray(fxycxy, dtype=np.float64)
    model_type = _rectification_model_type(lib, rectification_model)
    baseline = _baseline(models_rectified)

    if qrect0 is None:
        W, H = (int(x) for x in models_rectified[0].imagersize())
        if disparity.shape != (H, W):
            raise Exception(f"qrect0 is None, so the given disparity and full rectified images MUST have the same dimensions. I have disparity.shape={disparity.shape} and models_rectified[0].imagersize()={(W, H)}")
        d = np.ascontiguousarray(disparity.astype(np.uint16))
        # (uint16 arguments: a bound beyond their range is the end of the range)
        scale, dmin, dmax = (int(min(max(x, 0), 0xFFFF)) for x in (disparity_scale, disparity_scaled_min, disparity_scaled_max))
        if _rectification is not None:
            return _rectification._range_dense(d, scale, dmin, dmax)
        r = np.zeros((H, W), dtype=np.float64)
        image_d = _Image(W, H, W*2, d.ctypes.data)
        image_r = _Image(W, H, W*8, r.ctypes.data)
        if not lib.lib.mrcal_stereo_range_dense(C.addressof(image_r), C.addressof(image_d), scale, dmin, dmax, model_type,
                                                _ptr(fxycxy), baseline):
            raise _failed("mrcal_stereo_range_dense()")
        return r

    r = _range_sparse(disparity.astype(float) / disparity_scale, qrect0, float(disparity_min), float(disparity_max),
                      model_type, fxycxy, baseline, False)
    return r[0] if is_scalar and r.shape == (1,) else r


def _range_sparse(disparity, qrect0, disparity_min, disparity_max, model_type, fxycxy, baseline, want_points):
    """the broadcast batch through mrcal_amd_stereo_range_sparse(): ranges (...), or the points (...,3)"""
    lib, api = _handle._libs()
    qrect0 = np.asarray(qrect0, dtype=np.float64)
    if qrect0.ndim < 1 or qrect0.shape[-1] != 2:
        raise Exception(f"qrect0 must have shape (...,2), got {qrect0.shape}")
    lead = np.broadcast_shapes(disparity.shape, qrect0.shape[:-1])
    d = np.ascontiguousarray(np.broadcast_to(disparity, lead), dtype=np.float64).ravel()
    q = np.ascontiguousarray(np.broadcast_to(qrect0, lead + (2,)), dtype=np.float64).reshape(-1, 2)
    N = d.shape[0]
    out = np.zeros((N, 3) if want_points else (N,))
    if not lib.lib.mrcal_amd_stereo_range_sparse(None if want_points else _ptr(out), _ptr(out) if want_points else None,
                                                 _ptr(d), _ptr(q), N, disparity_min, disparity_max, model_type, _ptr(fxycxy),
                                                 baseline):
        raise _failed("mrcal_stereo_range_sparse()")
    return out.reshape(lead + ((3,) if want_points else ()))


def stereo_unproject(disparity, models_rectified, *, ranges=None, disparity_scale=1, qrect0=None):
    """The points (...,3), in the coordinates of the rectified camera 0, that disparities (or ranges) see: (0,0,0) where
the disparity is invalid. Exactly one of disparity and ranges is given; qrect0 as in stereo_range().
Reference: mrcal.stereo_unproject()"""
    if (ranges is None) == (disparity is None):
        raise Exception("Exactly one of (disparity,ranges) must be non-None")
    lib, api = _handle._libs()
    if ranges is None and qrect0 is not None:
        # one launch: the range and the unit vector it scales
        _validate_models_rectified(models_rectified)
        rectification_model, fxycxy = models_rectified[0].intrinsics()
        is_scalar = np.ndim(disparity) == 0 and np.ndim(qrect0) == 1
        d = np.atleast_1d(np.asarray(disparity)).astype(float) / disparity_scale
        p = _range_sparse(d, qrect0, 0., np.finfo(float).max, _rectification_model_type(lib, rectification_model),
                          np.ascontiguousarray(fxycxy, dtype=np.float64), _baseline(models_rectified), True)
        return p[0] if is_scalar and p.shape == (1, 3) else p
    if ranges is None:
        ranges = stereo_range(disparity, models_rectified, disparity_scale=disparity_scale, qrect0=qrect0)
    if qrect0 is None:
        W, H = (int(x) for x in models_rectified[0].imagersize())
        qrect0 = np.ascontiguousarray(np.stack(np.meshgrid(np.arange(W, dtype=float), np.arange(H, dtype=float)), axis=-1))
    vrect0 = api.unproject(np.asarray(qrect0, dtype=float), *models_rectified[0].intrinsics(), normalize=True)
    return vrect0 * np.asarray(ranges)[..., np.newaxis]


# ---------------------------------------------------------------------------------------------------------------------
# match_feature(): template matching between two images (csrc/match_feature.hip)

# cv2's values: a caller's cv2.TM_* constants work unchanged
TM_SQDIFF, TM_SQDIFF_NORMED, TM_CCORR, TM_CCORR_NORMED, TM_CCOEFF, TM_CCOEFF_NORMED = range(6)

MATCH_OK, MATCH_OPTIMUM_ON_EDGE, MATCH_SUBPIXEL_DEGENERATE, MATCH_OUTSIDE_IMAGE1, MATCH_OUTSIDE_IMAGE0 = range(5)


def apply_homography(H, q):
    """The pixels q (...,2) mapped through the homography H (3,3), or (...,3,3) broadcasting with q: (...,2), in double

Each coordinate is ((h0*x + h1*y) + h2) / ((h20*x + h21*y) + h22), evaluated in exactly that order.
Reference: mrcal.apply_homography()"""
    H, q = np.asarray(H, dtype=np.float64), np.asarray(q, dtype=np.float64)
    if H.ndim < 2 or H.shape[-2:] != (3, 3):
        raise Exception(f"H must have shape (...,3,3), got {H.shape}")
    if q.ndim < 1 or q.shape[-1] != 2:
        raise Exception(f"q must have shape (...,2), got {q.shape}")
    x, y = q[..., 0], q[..., 1]
    d = (H[..., 2, 0]*x + H[..., 2, 1]*y) + H[..., 2, 2]
    return np.stack((((H[..., 0, 0]*x + H[..., 0, 1]*y) + H[..., 0, 2])/d,
                     ((H[..., 1, 0]*x + H[..., 1, 1]*y) + H[..., 1, 2])/d), axis=-1)


def _template_size(template_size1):
    """-> (width, height), with the reference's refusals"""
    try:
        n = len(template_size1)
    except TypeError:
        n, template_size1 = 2, (template_size1, template_size1)
    if n != 2:
        raise Exception(f"template_size1 must be an interable of length 2 OR a scalar. Got an iterable of length {n}")
    for t in template_size1:
        if not (isinstance(t, (int, np.integer)) and t > 0):
            raise Exception(f"Each element of template_size1 must be an integer > 0. Got {t}")
    return int(template_size1[0]), int(template_size1[1])


def _match_images(image0, image1):
    for image in (image0, image1):
        if not isinstance(image, np.ndarray) or image.ndim != 2:
            raise Exception("match_feature() accepts ONLY grayscale images of shape (H,W)")
    a0, w0, h0, _, t0 = _image_arguments(image0, "image0")
    a1, w1, h1, _, t1 = _image_arguments(image1, "image1")
    if t0 != t1:
        raise Exception(f"image0 and image1 must have the same dtype, got {image0.dtype} and {image1.dtype}")
    return (a0, w0, h0), (a1, w1, h1), t0


def _match_features(q0, q1_estimate, H10):
    """-> q0 (N,2), q1e (N,2), H01 (N,3,3), in double"""
    if (H10 is None) == (q1_estimate is None):
        raise Exception("Exactly one of (q1_estimate,H10) must be given")
    q0 = np.asarray(q0, dtype=np.float64)
    if q0.ndim != 2 or q0.shape[1] != 2:
        raise Exception(f"q0 must have shape (N,2), got {q0.shape}")
    N = q0.shape[0]
    if H10 is None:
        q1e = np.asarray(q1_estimate, dtype=np.float64)
        if q1e.shape not in ((2,), (N, 2)):
            raise Exception(f"q1_estimate must have shape (2,) or ({N},2), got {q1e.shape}")
        q1e = np.ascontiguousarray(np.broadcast_to(q1e, (N, 2)))
        H10 = np.tile(np.eye(3), (N, 1, 1))
        H10[:, :2, 2] = q1e - q0
    else:
        H10 = np.asarray(H10, dtype=np.float64)
        if H10.shape not in ((3, 3), (N, 3, 3)):
            raise Exception(f"H10 must have shape (3,3) or ({N},3,3), got {H10.shape}")
        H10 = np.ascontiguousarray(np.broadcast_to(H10, (N, 3, 3)))
        q1e = apply_homography(H10, q0)
    H01 = np.linalg.inv(H10) if N else np.zeros((0, 3, 3))
    return q0, np.ascontiguousarray(q1e), np.ascontiguousarray(H01)


def _match_method(method):
    if method is None: return TM_CCORR_NORMED
    if not (isinstance(method, (int, np.integer)) and TM_SQDIFF <= method <= TM_CCOEFF_NORMED):
        raise Exception(f"method must be one of TM_SQDIFF ... TM_CCOEFF_NORMED (0..5), not {method!r}")
    return int(method)


def _match_radius(search_radius1):
    if not (isinstance(search_radius1, (int, np.integer)) and search_radius1 >= 0):
        raise Exception(f"search_radius1 must be an integer >= 0. Got {search_radius1}")
    return int(min(search_radius1, 1 << 30))


def _checkdims(image_shape, what, *qall):
    """the reference's test of the template's corners, with its messages"""
    for q in qall:
        if q[0] < 0:                raise Exception(f"Too close to the left edge in {what}")
        if q[1] < 0:                raise Exception(f"Too close to the top edge in {what} ")
        if q[0] >= image_shape[1]:  raise Exception(f"Too close to the right edge in {what} ")
        if q[1] >= image_shape[0]:  raise Exception(f"Too close to the bottom edge in {what} ")


def _template_window(q1e, template_size):
    """(tmin, tmax): the template's first and last pixel in image1"""
    tmin = np.round(q1e - (np.array(template_size, dtype=float) - 1.)/2.)
    return tmin, tmin + np.array(template_size, dtype=float) - 1


class FeatureMatcher(Handle):
    """Template matching between two images, resident: both images are uploaded once, and every match() finds a batch
of features of image0 in image1.

    image0, image1: grayscale (H,W) arrays of the same dtype: uint8, uint16 or float32.
      .match(q0, *, search_radius1, template_size1, q1_estimate=None, H10=None, method=None, diagnostics=False)
          q0 (N,2); q1_estimate: None, (2,) or (N,2); H10: None, (3,3) or (N,3,3): exactly one of the two.
          -> q1 (N,2), status (N,): 0 ok; 1 the optimum is on the edge of the match surface; 2 the subpixel fit is
          degenerate; 3 the template is outside image1; 4 outside image0. A row whose status is not 0 is NaN. No
          status raises: only arguments that are wrong whatever the data do.
          diagnostics=True: a third value, a list of N dicts as match_feature() returns them
    equalization = None | 'clahe' | 'stretch', clahe_clip_limit = 8.0, clahe_tiles = (8,8): both images (uint8 or uint16
    then) are equalized on the device after the upload (equalize_clahe(), equalize_stretch()), the same bits as
    equalizing them first; with 'stretch' the templates are uint8. None: nothing of it runs.
    What a match is: match_feature()"""

    _destroy = "mrcal_amd_feature_matcher_destroy"

    def __init__(self, image0, image1, *, equalization=None, clahe_clip_limit=8.0, clahe_tiles=(8, 8)):
        (a0, w0, h0), (a1, w1, h1), dtype = _match_images(image0, image1)
        eq, dtype_equalized = equalization_params(equalization, clahe_clip_limit, clahe_tiles, (image0, image1))
        self._dtype = a0.dtype if eq is None else dtype_equalized
        if eq is None:
            self._create("match_feature()", "mrcal_amd_feature_matcher_create", _ptr(a0), w0, h0, _ptr(a1), w1, h1, dtype)
        else:
            self._create("match_feature()", "mrcal_amd_feature_matcher_create_equalized", _ptr(a0), w0, h0, _ptr(a1), w1, h1,
                         dtype, C.addressof(eq))

    def match(self, q0, *, search_radius1, template_size1, q1_estimate=None, H10=None, method=None, diagnostics=False):
        self._open()
        tw, th = _template_size(template_size1)
        q0, q1e, H01 = _match_features(q0, q1_estimate, H10)
        method, radius = _match_method(method), _match_radius(search_radius1)
        N = q0.shape[0]
        q1, status = np.full((N, 2), np.nan), np.zeros((N,), dtype=np.int32)
        at, value = np.full((N, 2), np.nan), np.full((N,), np.nan)
        qmin, size = np.zeros((N, 2), dtype=np.int32), np.zeros((N, 2), dtype=np.int32)
        self._call("match_feature()", "mrcal_amd_feature_matcher_match", N, _ptr(q1e), _ptr(H01), tw, th, radius, method,
                   _ptr(q1), _ptr(status), _ptr(at), _ptr(value), _ptr(qmin), _ptr(size))
        if not diagnostics:
            return q1, status
        out = []
        for i in range(N):
            d = dict()
            if status[i] not in (MATCH_OUTSIDE_IMAGE1, MATCH_OUTSIDE_IMAGE0):
                d['matchoutput_image'] = np.zeros((size[i, 1], size[i, 0]), dtype=np.float32)
                d['template']          = np.zeros((th, tw), dtype=self._dtype)
                self._call("match_feature()", "mrcal_amd_feature_matcher_matchoutput", i, _ptr(d['matchoutput_image']))
                self._call("match_feature()", "mrcal_amd_feature_matcher_template", i, _ptr(d['template']))
            if status[i] == MATCH_OK:
                d['matchoutput_optimum_subpixel_at'] = at[i].copy()
                d['matchoutput_optimum_subpixel']    = float(value[i])
                d['qshift_image1_matchoutput']       = qmin[i] + q1e[i] - _template_window(q1e[i], (tw, th))[0]
            out.append(d)
        return q1, status, out


def match_feature(image0, image1, q0, *, search_radius1, template_size1, q1_estimate=None, H10=None, method=None,
                  visualize=False, return_plot_args=False, equalization=None, clahe_clip_limit=8.0, clahe_tiles=(8, 8)):
    """Finds in image1 the pixel q1 that shows what the pixel q0 of image0 shows: (q1, diagnostics)

image0, image1: grayscale (H,W). q0 (2,). Exactly one of q1_estimate (2,), a guess of q1, and H10 (3,3), a homography
that maps image0 pixels near q0 to image1 pixels (it corrects for the geometric difference between the images; for its
construction from two camera models see the reference's docstring). template_size1: the size of the template in
image1 pixels, a scalar or (width, height). search_radius1: how far from the estimate, in image1 pixels, to look; the
search window is clipped to image1. method: one of TM_SQDIFF ... TM_CCOEFF_NORMED (cv2's values); None: TM_CCORR_NORMED.

A match. With q1e = q1_estimate, or apply_homography(H10, q0), and ts = (width, height) of the template:
  1. tmin = round(q1e - (ts-1)/2), tmax = tmin + ts - 1. Both must lie inside image1: "Too close to the ... edge in
     image1" is raised otherwise
  2. the template is transform_image(image0, map), map = float32(apply_homography(inv(H10), integer image1 pixels
     tmin..tmax)). Its four corners must map inside image0: "Too close to the ... edge in image0"
  3. image1 is cut to max(tmin - search_radius1, 0) .. min(tmin + search_radius1 + ts - 1, size - 1); the match
     surface has (cut - ts + 1) entries each way
  4. every entry gets the method's score of the template against the window of the cut that begins there, from the
     window's sums IT = sum(I T), SI = sum(I), SI2 = sum(I I) and the template's ST, ST2, N = width height: exact
     integers for integer images, double in a fixed order for float32; the formula in double, rounded to float32:
       SQDIFF SI2 - 2 IT + ST2; CCORR IT; CCOEFF IT - SI ST/N;
       SQDIFF_NORMED, CCORR_NORMED: those over sqrt(SI2 ST2);
       CCOEFF_NORMED: CCOEFF over sqrt(max(SI2 - SI SI/N, 0) max(ST2 - ST ST/N, 0)).
     A denominator that is not > 0 gives 0 (1 for SQDIFF_NORMED)
  5. the optimum is the minimum (SQDIFF, SQDIFF_NORMED) or the maximum of the surface, the first one in row-major
     order. If it lies on the edge of the surface there is no match: (None, diagnostics)
  6. a quadric is fit to the 3x3 entries around the optimum, and q1 is where it is stationary, moved to image1

diagnostics: matchoutput_image (the surface, float32), template (what was looked for), and for a match
matchoutput_optimum_subpixel_at (in surface coordinates), matchoutput_optimum_subpixel (the fit's value there) and
qshift_image1_matchoutput (q1 = matchoutput_optimum_subpixel_at + qshift_image1_matchoutput).
The N = 1 case of FeatureMatcher.match(): many features of one pair of images are faster through that.

Departures from the reference:
  - images are uint8, uint16 or float32 (cv2 takes the first and the last);
  - q0, H10 and q1_estimate are used in double; the reference rounds them to float32 first;
  - the correlation is summed exactly (cv2.matchTemplate() uses a float32 FFT), so the same call gives the same bits;
  - numpy.round rounds halves to even, and so does the library;
  - a subpixel fit with a zero determinant or a result that is not finite gives (None, diagnostics); the reference
    returns inf or nan there;
  - the subpixel fit is the closed form of the reference's 9-point least squares (on the -1,0,1 grid the normal
    equations are diagonal but for the coupling of c00, c20, c02);
  - visualize and return_plot_args are refused: gnuplotlib is not part of this project;
  - equalization = 'clahe' | 'stretch' (with clahe_clip_limit, clahe_tiles) equalizes both images on the device first, as
    the reference's mrcal-triangulate --clahe does on the host before it calls this: FeatureMatcher.
Reference: mrcal.match_feature()"""
    if visualize or return_plot_args:
        raise Exception("match_feature(visualize=True) is not available: gnuplotlib is not part of mrcal_amd")
    tw, th = _template_size(template_size1)
    _match_images(image0, image1)
    if equalization is not None:
        equalization_params(equalization, clahe_clip_limit, clahe_tiles, (image0, image1))
    if (H10 is None) == (q1_estimate is None):
        raise Exception("Exactly one of (q1_estimate,H10) must be given")
    q0 = np.asarray(q0, dtype=np.float64)
    if q0.shape != (2,):
        raise Exception(f"q0 must have shape (2,), got {q0.shape}")
    _match_method(method), _match_radius(search_radius1)
    if q1_estimate is not None:
        q1_estimate = np.asarray(q1_estimate, dtype=np.float64)
        if q1_estimate.shape != (2,):
            raise Exception(f"q1_estimate must have shape (2,), got {q1_estimate.shape}")
    elif np.shape(H10) != (3, 3):
        raise Exception(f"H10 must have shape (3,3), got {np.shape(H10)}")
    # The two "too close to the edge" refusals with the reference's messages, before anything goes to the device: the
    # library's tests (statuses 3 and 4), restated
    _, q1e, H01 = _match_features(q0[np.newaxis], q1_estimate, H10)
    tmin, tmax = _template_window(q1e[0], (tw, th))
    _checkdims(image1.shape, "image1", tmin, tmax)
    corners = np.array(((tmin[0], tmin[1]), (tmin[0], tmax[1]), (tmax[0], tmin[1]), (tmax[0], tmax[1])))
    _checkdims(image0.shape, "image0", *apply_homography(H01[0], corners).astype(np.float32))

    with FeatureMatcher(image0, image1, equalization=equalization, clahe_clip_limit=clahe_clip_limit, clahe_tiles=clahe_tiles) as matcher:
        q1, status, diagnostics = matcher.match(q0[np.newaxis], search_radius1=search_radius1, template_size1=(tw, th),
                                                q1_estimate=q1_estimate, H10=H10, method=method, diagnostics=True)
    if status[0] in (MATCH_OUTSIDE_IMAGE1, MATCH_OUTSIDE_IMAGE0):       # (a corner that is not a number)
        raise Exception(f"Too close to the edge in image{0 if status[0] == MATCH_OUTSIDE_IMAGE0 else 1}")
    if status[0] != MATCH_OK:
        return None, diagnostics[0]
    return q1[0], diagnostics[0]


# ---------------------------------------------------------------------------------------------------------------------
# stereo_matching_sgm(): dense disparities of a rectified pair (csrc/stereo_sgm.hip)

# cv2's scale of a StereoSGBM disparity image
STEREO_SGM_DISPARITY_SCALE = 16


class _SgmParams(C.Structure):
    """mrcal_amd_stereo_sgm_params_t"""
    _fields_ = [(n, C.c_int) for n in ("disparity_min", "disparity_max", "P1", "P2", "paths", "uniqueness_ratio",
                                       "disp12_max_diff")]


def _sgm_int(name, value):
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)):
        raise Exception(f"stereo_matching_sgm(): {name} must be an integer. Got {value!r}")
    return int(value)


def _sgm_params(*, disparity_min=0, disparity_max, P1=10, P2=120, paths=8, uniqueness_ratio=10, disp12_max_diff=1):
    """-> _SgmParams, with the refusals of csrc/sgm_plan.hpp (sgm_params_ok()) in its words, made before any device work"""
    dmin, dmax = _sgm_int("disparity_min", disparity_min), _sgm_int("disparity_max", disparity_max)
    P1, P2, paths = _sgm_int("P1", P1), _sgm_int("P2", P2), _sgm_int("paths", paths)
    ratio, diff = _sgm_int("uniqueness_ratio", uniqueness_ratio), _sgm_int("disp12_max_diff", disp12_max_diff)
    D = dmax - dmin
    if D <= 0 or D > 256 or D % 16 != 0:
        raise Exception(f"stereo_matching_sgm(): disparity_max - disparity_min must be a positive multiple of 16, at most 256. Got {D}")
    if not (0 <= P1 <= P2 <= 193):
        raise Exception(f"stereo_matching_sgm(): must have 0 <= P1 <= P2 <= 193. Got P1 = {P1}, P2 = {P2}")
    if paths not in (4, 8):
        raise Exception(f"stereo_matching_sgm(): paths must be 4 or 8. Got {paths}")
    if not (0 <= ratio <= 99):
        raise Exception(f"stereo_matching_sgm(): uniqueness_ratio must be in 0..99. Got {ratio}")
    if STEREO_SGM_DISPARITY_SCALE*(dmin - 1) < -32768 or STEREO_SGM_DISPARITY_SCALE*dmax > 32767:
        raise Exception(f"stereo_matching_sgm(): disparities {dmin}..{dmax} scaled by 16 leave int16 (at most -2047..2047)")
    return _SgmParams(dmin, dmax, P1, P2, paths, ratio, max(min(diff, 1 << 20), -1))


_SGM_DTYPES = {np.dtype(np.uint8): 0, np.dtype(np.uint16): 1}


def _sgm_dtype(dtype):
    try:    dtype = np.dtype(dtype)
    except TypeError: dtype = None
    if dtype not in _SGM_DTYPES:
        raise Exception(f"stereo_matching_sgm(): images must have dtype uint8 or uint16, not {dtype}")
    return dtype


def _sgm_images(image0, image1, shape=None, dtype=None):
    """-> the two dense arrays; the refusals before any device work"""
    for image in (image0, image1):
        if not isinstance(image, np.ndarray) or image.ndim != 2 or image.size == 0:
            raise Exception("stereo_matching_sgm() accepts ONLY grayscale images of shape (H,W)" +
                            (f", got {image.shape}" if isinstance(image, np.ndarray) else ""))
    if image0.shape != image1.shape:
        raise Exception(f"stereo_matching_sgm(): image0 and image1 must have the same shape, got {image0.shape} and {image1.shape}")
    if image0.dtype != image1.dtype:
        raise Exception(f"stereo_matching_sgm(): image0 and image1 must have the same dtype, got {image0.dtype} and {image1.dtype}")
    _sgm_dtype(image0.dtype)
    if shape is not None and (image0.shape != shape or image0.dtype != dtype):
        raise Exception(f"stereo_matching_sgm(): this matcher was made for images of shape {shape} and dtype {dtype}, "
                        f"got {image0.shape} and {image0.dtype}")
    return np.ascontiguousarray(image0), np.ascontiguousarray(image1)


class StereoMatcherSGM(Handle):
    """Dense stereo matching, resident: every device buffer a match of one image size needs is made once, and every
match() reuses them.

    shape: (H,W) of the rectified images; dtype: uint8 or uint16; the parameters: those of stereo_matching_sgm(),
    speckle_window_size and speckle_range among them.
      .match(image0, image1, out=None)   -> int16 (H,W); out: the array to fill
      .stage_milliseconds()              how long the census, the paths, the selection and the left-right check of the
                                         last match() took on the device
      .speckle_milliseconds()            ... and the speckle filter (0 without it)
    What a disparity image is: stereo_matching_sgm()"""

    _destroy = "mrcal_amd_stereo_sgm_destroy"

    def __init__(self, shape, dtype, *, speckle_window_size=0, speckle_range=0, **params):
        self._speckle = _speckle_keywords(speckle_window_size, speckle_range)
        self._params = _sgm_params(**params)
        self._dtype = _sgm_dtype(dtype)
        try:    shape = tuple(int(n) for n in shape)
        except TypeError: shape = ()
        if len(shape) != 2 or shape[0] <= 0 or shape[1] <= 0:
            raise Exception(f"stereo_matching_sgm(): shape must be (H,W), got {shape}")
        self.shape = shape
        self._create("stereo_matching_sgm()", "mrcal_amd_stereo_sgm_create", shape[1], shape[0], _SGM_DTYPES[self._dtype],
                     C.addressof(self._params))
        if self._speckle[0] > 0:        # (0: nothing of the filter is touched)
            try:
                self._call("stereo_matching_sgm()", "mrcal_amd_stereo_sgm_set_speckle_filter", *self._speckle)
            except Exception:
                self.close()
                raise

    def match(self, image0, image1, out=None):
        self._open()
        a0, a1 = _sgm_images(image0, image1, self.shape, self._dtype)
        o, r = _output_array(out, self.shape, np.int16, False)
        self._call("stereo_matching_sgm()", "mrcal_amd_stereo_sgm_match", _ptr(a0), _ptr(a1), _ptr(o))
        if r is not o: r[...] = o
        return r

    def stage_milliseconds(self):
        self._open()
        ms = np.zeros((4,), dtype=np.float32)
        self._call("stereo_matching_sgm()", "mrcal_amd_stereo_sgm_stage_milliseconds", _ptr(ms))
        return dict(zip(("census", "paths", "select", "check"), (float(x) for x in ms)))

    def speckle_milliseconds(self):
        """how long the speckle filter of the last match() took on the device; 0 without it"""
        self._open()
        ms = C.c_float(0)
        self._call("stereo_matching_sgm()", "mrcal_amd_stereo_sgm_speckle_milliseconds", C.addressof(ms))
        return float(ms.value)


def stereo_matching_sgm(image0, image1, *, disparity_min=0, disparity_max, P1=10, P2=120, paths=8, uniqueness_ratio=10,
                        disp12_max_diff=1, speckle_window_size=0, speckle_range=0):
    """The disparity image of a rectified pair, by semi-global matching on a census cost: int16 (H,W), the disparity in
pixels times STEREO_SGM_DISPARITY_SCALE = 16 (cv2's scale); an invalid pixel holds 16 (disparity_min - 1)

image0 (left), image1 (right): rectified, grayscale (H,W), the same shape and dtype, uint8 or uint16.
D = disparity_max - disparity_min must be a positive multiple of 16, at most 256; disparity_min may be negative;
0 <= P1 <= P2 <= 193; paths is 4 or 8; uniqueness_ratio is in 0..99 (0: no test); disp12_max_diff < 0: no left-right check.
The result goes straight into stereo_range(disparity, models_rectified, disparity_scale = 16, disparity_min = ...).

Everything is integer arithmetic, and the result is defined to the bit. The index i in [0,D) means d = disparity_min + i.
  1. census: per image and pixel 62 bits over the window 9 wide x 7 tall around the pixel, without the centre: a bit is
     (neighbour < centre); a neighbour outside the image is the nearest pixel inside
  2. C(y,x,i) = popcount(census0(y,x) XOR census1(y,x-d)); 62 where x-d is outside the image
  3. per path direction r: L_r(p,i) = C(p,i) + min(L_r(p-r,i), L_r(p-r,i-1) + P1, L_r(p-r,i+1) + P1, m + P2) - m,
     m = min_k L_r(p-r,k); an i-1, i+1 outside [0,D) takes no part; where p-r is outside the image L_r(p,.) = C(p,.).
     paths = 4: left, right, up, down; 8: the diagonals too. S = sum_r L_r
  4. i* = the first index of the minimum of S(p,.). Invalid if some i with |i - i*| > 1 has
     S(p,i) (100 - uniqueness_ratio) < S(p,i*) 100. Where 0 < i* < D-1, with a = S(i*-1), c = S(i*+1),
     den = max(a + c - 2 S(i*), 1): the scaled index is 16 i* + floor(((a - c) 16 + den)/(2 den)); elsewhere 16 i*
  5. the right image's i1(y,x1) = the smallest i that minimises S(y, x1 + d, i) over the i with x1 + d inside the image.
     A left pixel is invalid if x - d* is outside the image, or |i1(y, x - d*) - i*| > disp12_max_diff
  6. the result is 16 disparity_min + the scaled index
  7. on request only: speckle_window_size > 0 (cv2.StereoSGBM's speckleWindowSize and speckleRange) filters that result
     on the device before it is copied out: filter_speckles(result, new_value = 16 (disparity_min - 1),
     max_speckle_size = speckle_window_size, max_diff = 16 speckle_range). speckle_window_size = 0, the default:
     no filter, the result of steps 1-6 and nothing else runs

The N = 1 case of StereoMatcherSGM.match(): a sequence of pairs of one size is faster through that.
Shaped like the reference's mrcal.stereo_matching_libelas(). Not here: cv2.StereoSGBM's Birchfield-Tomasi cost on
Sobel-filtered images, its adaptive P2, colour input, and ELAS itself: nothing imitates either matcher pixel for pixel."""
    params = dict(disparity_min=disparity_min, disparity_max=disparity_max, P1=P1, P2=P2, paths=paths,
                  uniqueness_ratio=uniqueness_ratio, disp12_max_diff=disp12_max_diff)
    _speckle_keywords(speckle_window_size, speckle_range)
    _sgm_params(**params)
    a0, a1 = _sgm_images(image0, image1)
    with StereoMatcherSGM(a0.shape, a0.dtype, speckle_window_size=speckle_window_size, speckle_range=speckle_range,
                          **params) as matcher:
        return matcher.match(a0, a1)


# ---------------------------------------------------------------------------------------------------------------------
# filter_speckles(): small regions of a disparity image become invalid (csrc/speckle_filter.hip)

_INT32_MAX = (1 << 31) - 1


def _speckle_int(name, value):
    """the refusals of csrc/speckle_plan.hpp in its words, made before any device work"""
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)) or value < 0:
        raise Exception(f"filter_speckles(): {name} must be a non-negative integer. Got {value!r}")
    return int(value)


def _speckle_keywords(speckle_window_size, speckle_range):
    """-> (window size, range) as the library's two ints. Beyond 2^31 - 1 pixels no region is larger, and a range of
    4096 is already a max_diff above 65535"""
    return (min(_speckle_int("speckle_window_size", speckle_window_size), _INT32_MAX),
            min(_speckle_int("speckle_range", speckle_range), 4096))


def _speckle_params(new_value, max_speckle_size, max_diff):
    if isinstance(new_value, (bool, np.bool_)) or not isinstance(new_value, (int, np.integer)):
        raise Exception(f"filter_speckles(): new_value must be an integer. Got {new_value!r}")
    if not (-32768 <= new_value <= 32767):
        raise Exception(f"filter_speckles(): new_value must be in -32768..32767. Got {new_value}")
    return (int(new_value), min(_speckle_int("max_speckle_size", max_speckle_size), _INT32_MAX),
            min(_speckle_int("max_diff", max_diff), 65535))


def _speckle_shape(shape):
    try:    shape = tuple(int(n) for n in shape)
    except TypeError: shape = ()
    if len(shape) != 2:
        raise Exception(f"filter_speckles(): shape must be (H,W), got {shape}")
    if shape[0] <= 0 or shape[1] <= 0 or shape[0]*shape[1] > MAX_PIXELS:
        raise Exception(f"filter_speckles(): images of {shape[1]} x {shape[0]} pixels cannot be filtered")
    return shape


def _speckle_image(disparity, shape=None):
    if not isinstance(disparity, np.ndarray) or disparity.ndim != 2 or disparity.dtype != np.int16:
        raise Exception("filter_speckles(): the disparity image must be a 2-D int16 array" +
                        (f", got shape {disparity.shape} and dtype {disparity.dtype}" if isinstance(disparity, np.ndarray) else ""))
    _speckle_shape(disparity.shape)
    if shape is not None and disparity.shape != shape:
        raise Exception(f"filter_speckles(): this filter was made for images of shape {shape}, got {disparity.shape}")


def _speckle_out(out, shape):
    if out is not None and (not isinstance(out, np.ndarray) or out.shape != shape or out.dtype != np.int16):
        raise Exception(f"filter_speckles(): 'out' must be a numpy array of shape {shape} and dtype int16")


class SpeckleFilter(Handle):
    """filter_speckles(), resident: the device buffers for one image size are made once, and every filter() reuses them.

    shape: (H,W) of the disparity images.
      .filter(disparity, *, new_value, max_speckle_size, max_diff, out=None)   -> int16 (H,W); out: the array to
                                         fill, which may be disparity itself
      .milliseconds()                    how long the last filter() took on the device, without the copies
      .pass_milliseconds()               ... pass by pass: the tiles' labels, the joins across the tiles' borders, the
                                         roots and sizes, the result
    What the filter is: filter_speckles()"""

    _destroy = "mrcal_amd_speckle_filter_destroy"

    def __init__(self, shape):
        self.shape = _speckle_shape(shape)
        self._create("filter_speckles()", "mrcal_amd_speckle_filter_create", self.shape[1], self.shape[0])

    def filter(self, disparity, *, new_value, max_speckle_size, max_diff, out=None):
        self._open()
        _speckle_image(disparity, self.shape)
        params = _speckle_params(new_value, max_speckle_size, max_diff)
        _speckle_out(out, self.shape)
        a = np.ascontiguousarray(disparity)
        # (the library takes in == out: a dense `out` is filled straight away, disparity itself included)
        o, r = _output_array(out, self.shape, np.int16, False)
        self._call("filter_speckles()", "mrcal_amd_speckle_filter_apply", _ptr(a), _ptr(o), *params)
        if r is not o: r[...] = o
        return r

    def milliseconds(self):
        self._open()
        ms = C.c_float(0)
        self._call("filter_speckles()", "mrcal_amd_speckle_filter_milliseconds", C.addressof(ms))
        return float(ms.value)

    def pass_milliseconds(self):
        self._open()
        ms = np.zeros((4,), dtype=np.float32)
        self._call("filter_speckles()", "mrcal_amd_speckle_filter_pass_milliseconds", _ptr(ms))
        return dict(zip(("label", "merge", "count", "apply"), (float(x) for x in ms)))


def filter_speckles(disparity, *, new_value, max_speckle_size, max_diff, out=None):
    """A disparity image without its speckles: the connected regions of similar disparity that are too small to be a
surface become invalid. int16 (H,W) in, int16 (H,W) out: a new array, or `out`, which may be `disparity` itself.

  1. a pixel equal to new_value takes no part and is never changed
  2. two 4-neighbours (left/right, up/down) that both take part are joined if |a - b| <= max_diff; the difference is
     taken in 32 bits (-32768 beside 32767 differs by 65535), and a max_diff above 65535 means 65535
  3. the regions are the connected components of that graph
  4. every pixel of a region of size <= max_speckle_size becomes new_value; everything else is unchanged.
     max_speckle_size = 0 changes nothing

This is cv2.filterSpeckles(img, newVal, maxSpeckleSize, maxDiff) for CV_16S, the filter cv2.StereoSGBM applies with
newVal = 16 (minDisparity - 1), maxSpeckleSize = speckleWindowSize, maxDiff = 16 speckleRange, and the reference's
mrcal-stereo recommends (--sgbm-speckle-window-size 200 --sgbm-speckle-range 2). cv2's flood fill compares original
values only and the relation is symmetric, so the result does not depend on the order of the scan; "equal to cv2" rests
on a transcription of cv2's loop that the tests hold a graph formulation to (tests/speckle_checker.py), not on cv2
itself. Integer arithmetic on the device (csrc/speckle_filter.hip), the same bits on every call; no CPU fallback.
stereo_matching_sgm(..., speckle_window_size = ..., speckle_range = ...) applies it before the disparity image leaves
the device. The N = 1 case of SpeckleFilter.filter()."""
    _speckle_image(disparity)
    _speckle_params(new_value, max_speckle_size, max_diff)
    _speckle_out(out, disparity.shape)
    with SpeckleFilter(disparity.shape) as f:
        return f.filter(disparity, new_value=new_value, max_speckle_size=max_speckle_size, max_diff=max_diff, out=out)


# ---------------------------------------------------------------------------------------------------------------------
# stereo_point_cloud(): disparities to a compacted, coloured cloud of points (csrc/point_cloud.hip)

_CLOUD_FRAMES = ('ref', 'cam0', 'rect0')
_CLOUD_DTYPES = {np.dtype(np.uint8): 0, np.dtype(np.uint16): 1}


class _CloudParams(C.Structure):
    """mrcal_amd_point_cloud_params_t"""
    _fields_ = [("disparity_scale", C.c_uint16), ("disparity_scaled_min", C.c_uint16), ("disparity_scaled_max", C.c_uint16),
                ("range_min", C.c_double), ("range_max", C.c_double), ("Rt_out_rect0", C.c_void_p), ("points_float32", C.c_int),
                ("image", C.c_void_p), ("image_width", C.c_int), ("image_height", C.c_int), ("image_channels", C.c_int),
                ("image_dtype", C.c_int)]


def _cloud_disparity(disparity, shape, disparity_scale, disparity_min, disparity_max, disparity_scaled_min, disparity_scaled_max):
    """-> (the dense uint16 image, scale, scaled minimum, scaled maximum) as stereo_range()'s dense form makes them"""
    if not isinstance(disparity, np.ndarray) or disparity.ndim != 2 or disparity.dtype.kind not in 'iuf':
        raise Exception("stereo_point_cloud(): the disparity must be a 2-D numeric numpy array" +
                        (f", got shape {disparity.shape} and dtype {disparity.dtype}" if isinstance(disparity, np.ndarray) else ""))
    if disparity.shape != shape:
        raise Exception(f"stereo_point_cloud(): the disparity and the rectified images MUST have the same dimensions. I have disparity.shape={disparity.shape} and models_rectified[0].imagersize()={(shape[1], shape[0])}")
    if shape[0]*shape[1] > MAX_PIXELS:
        raise Exception(f"stereo_point_cloud(): a disparity image of {shape[1]} x {shape[0]} pixels cannot be made a cloud of: at most {MAX_PIXELS} pixels")
    if disparity_min is not None and disparity_scaled_min is not None and disparity_min != disparity_scaled_min:
        raise Exception("disparity_min and disparity_scaled_min may not both be given")
    if disparity_max is not None and disparity_scaled_max is not None and disparity_max != disparity_scaled_max:
        raise Exception("disparity_max and disparity_scaled_max may not both be given")
    if disparity_max is None and disparity_scaled_max is None and disparity.dtype == np.int16:
        disparity_scaled_max = 0x7FFF
    lowest  = disparity_scaled_min if disparity_scaled_min is not None else 0      if disparity_min is None else disparity_min*disparity_scale
    highest = disparity_scaled_max if disparity_scaled_max is not None else 0xFFFF if disparity_max is None else disparity_max*disparity_scale
    scale, dmin, dmax = (int(min(max(x, 0), 0xFFFF)) for x in (disparity_scale, lowest, highest))
    if dmin >= dmax:
        raise Exception(f"stereo_point_cloud(): must have disparity_scaled_max > disparity_scaled_min. Got {dmax} and {dmin}")
    return np.ascontiguousarray(disparity.astype(np.uint16)), scale, dmin, dmax


def _cloud_image_of_any_size(image, what):
    """-> (dense array, width, height, channels, dtype code) of a colour image"""
    if not isinstance(image, np.ndarray) or image.dtype not in _CLOUD_DTYPES:
        raise Exception(f"stereo_point_cloud(): '{what}' must be a numpy array of dtype uint8 or uint16" +
                        (f", not {image.dtype}" if isinstance(image, np.ndarray) else ""))
    if not (image.ndim == 2 or (image.ndim == 3 and image.shape[2] == 3)) or image.size == 0:
        raise Exception(f"stereo_point_cloud(): '{what}' must have shape (H,W) or (H,W,3), got {image.shape}")
    return np.ascontiguousarray(image), image.shape[1], image.shape[0], (1 if image.ndim == 2 else 3), _CLOUD_DTYPES[image.dtype]


def _cloud_image(image, what, models):
    """... of a colour image of camera 0, or None"""
    if image is None:
        return None
    if models is None:
        raise Exception(f"stereo_point_cloud(): '{what}' needs 'models': the colours are read through the rectification map of camera 0")
    arguments = _cloud_image_of_any_size(image, what)
    W, H = (int(x) for x in models[0].imagersize())
    if image.shape[:2] != (H, W):
        raise Exception(f"stereo_point_cloud(): '{what}' must have the imager size of camera 0, (H,W) = {(H, W)}, got {image.shape[:2]}")
    return arguments


def _cloud_frame(models_rectified, models, range_min, range_max, frame, dtype):
    """-> (range_min, range_max, Rt_out_rect0 (4,3) or None, the points are float32)"""
    if frame not in _CLOUD_FRAMES:
        raise Exception(f"stereo_point_cloud(): frame must be one of {_CLOUD_FRAMES}, not {frame!r}")
    if frame == 'cam0' and models is None:
        raise Exception("stereo_point_cloud(): frame='cam0' needs 'models'")
    try:    dtype = np.dtype(dtype)
    except TypeError: dtype = None
    if dtype is None or dtype not in (np.dtype(np.float64), np.dtype(np.float32)):      # (None == np.dtype(float) holds)
        raise Exception(f"stereo_point_cloud(): dtype must be float64 or float32, not {dtype}")
    rmin = 0. if range_min is None else float(range_min)
    rmax = np.inf if range_max is None else float(range_max)
    if not rmin <= rmax:
        raise Exception(f"stereo_point_cloud(): must have range_min <= range_max. Got {rmin:g} and {rmax:g}")
    if   frame == 'ref':  Rt = models_rectified[0].Rt_ref_cam()
    elif frame == 'cam0': Rt = compose_Rt(models[0].Rt_cam_ref(), models_rectified[0].Rt_ref_cam())
    else:                 Rt = None
    if Rt is not None: Rt = np.ascontiguousarray(Rt, dtype=np.float64)
    return rmin, rmax, Rt, dtype == np.float32


def _cloud_params(scale, dmin, dmax, rmin, rmax, Rt, float32, image):
    """-> (_CloudParams, what it points to)"""
    p = _CloudParams(scale, dmin, dmax, rmin, rmax, None if Rt is None else Rt.ctypes.data, int(float32), None, 0, 0, 0, 0)
    if image is not None:
        p.image, p.image_width, p.image_height, p.image_channels, p.image_dtype = image[0].ctypes.data, *image[1:]
    return p, (Rt, image)


def _cloud_read(owner, read, N, float32, image):
    """owner: the Rectification or StereoPointCloud that made the cloud; read: the name of its read function"""
    points = np.zeros((N, 3), dtype=np.float32 if float32 else np.float64)
    index  = np.zeros((N,), dtype=np.int32)
    color  = None if image is None else np.zeros((N,) if image[3] == 1 else (N, 3), dtype=image[0].dtype)
    owner._call("stereo_point_cloud()", read, _ptr(points), _ptr(color), _ptr(index))
    return points, color, index


def _cloud_stage_milliseconds(owner, name):
    ms = np.zeros((3,), dtype=np.float32)
    owner._call("stereo_point_cloud()", name, _ptr(ms))
    return dict(zip(("mask", "scan", "scatter"), (float(x) for x in ms)))


class StereoPointCloud(Handle):
    """stereo_point_cloud() without the camera models, resident: the device buffers for one size of disparity image are
made once, and every point_cloud() reuses them; the output buffers grow when a cloud outgrows them.

    models_rectified: what rectified_system() returned. map0: None, or the float32 (Nel,Naz,2) rectification map of
    camera 0, rectification_maps(...)[0], which a colour image is read through.
      .point_cloud(disparity, *, image0=None, ..., frame='ref' or 'rect0', dtype=np.float64)  -> (points, color, index)
      .stage_milliseconds()     how long the mask, the scan and the scatter of the last cloud took on the device
    What a cloud is: stereo_point_cloud(). A Rectification has its own: Rectification.point_cloud()"""

    _destroy = "mrcal_amd_point_cloud_destroy"

    def __init__(self, models_rectified, *, map0=None):
        _validate_models_rectified(models_rectified)
        self._models_rectified = tuple(models_rectified)
        self.Naz, self.Nel = (int(x) for x in models_rectified[0].imagersize())
        if map0 is not None:
            if not isinstance(map0, np.ndarray) or map0.dtype != np.float32 or map0.shape != (self.Nel, self.Naz, 2):
                raise Exception(f"stereo_point_cloud(): map0 must be a float32 numpy array of shape {(self.Nel, self.Naz, 2)}")
            map0 = np.ascontiguousarray(map0)
        if self.Nel*self.Naz > MAX_PIXELS:
            raise Exception(f"stereo_point_cloud(): a disparity image of {self.Naz} x {self.Nel} pixels cannot be made a cloud of: at most {MAX_PIXELS} pixels")
        lib, _ = _handle._libs()
        rectification_model, fxycxy = models_rectified[0].intrinsics()
        fxycxy = np.ascontiguousarray(fxycxy, dtype=np.float64)
        self._create("stereo_point_cloud()", "mrcal_amd_point_cloud_create", _rectification_model_type(lib, rectification_model),
                     _ptr(fxycxy), _baseline(models_rectified), self.Naz, self.Nel, None)
        self._has_map = map0 is not None
        if self._has_map:
            try:
                self._call("stereo_point_cloud()", "mrcal_amd_point_cloud_set_map", _ptr(map0))
            except Exception:
                self.close()
                raise

    def point_cloud(self, disparity, *, image0=None, disparity_scale=1, disparity_min=None, disparity_max=None,
                    disparity_scaled_min=None, disparity_scaled_max=None, range_min=None, range_max=None,
                    frame='ref', dtype=np.float64):
        self._open()
        if frame == 'cam0':
            raise Exception("stereo_point_cloud(): frame='cam0' needs 'models'")
        if image0 is not None:
            if not self._has_map:
                raise Exception("stereo_point_cloud(): 'image0' needs the rectification map of camera 0, and no map0 was given")
            image0 = _cloud_image_of_any_size(image0, "image0")       # (whatever image map0 leads into)
        d, scale, dmin, dmax = _cloud_disparity(disparity, (self.Nel, self.Naz), disparity_scale, disparity_min, disparity_max,
                                                disparity_scaled_min, disparity_scaled_max)
        rmin, rmax, Rt, float32 = _cloud_frame(self._models_rectified, None, range_min, range_max, frame, dtype)
        p, keep = _cloud_params(scale, dmin, dmax, rmin, rmax, Rt, float32, image0)
        N = C.c_int(0)
        self._call("stereo_point_cloud()", "mrcal_amd_point_cloud_compute", _ptr(d), C.addressof(p), C.addressof(N))
        return _cloud_read(self, "mrcal_amd_point_cloud_read", N.value, float32, image0)

    def stage_milliseconds(self):
        self._open()
        return _cloud_stage_milliseconds(self, "mrcal_amd_point_cloud_stage_milliseconds")


def stereo_point_cloud(disparity, models_rectified, *, models=None, image0=None, disparity_scale=1, disparity_min=None,
                       disparity_max=None, disparity_scaled_min=None, disparity_scaled_max=None, range_min=None,
                       range_max=None, frame='ref', dtype=np.float64):
    """The points a dense disparity image sees, compacted and coloured: (points (N,3), color, index (N,) int32)

What mrcal-stereo --write-point-cloud makes, on the device: only the N kept points cross to the host.
write_point_cloud_as_ply(filename, points, color = color) writes them.

disparity: the (Nel, Naz) image of a stereo matcher, in units of 1/disparity_scale pixels. models_rectified: what
rectified_system() returned. models: the two cameramodels: needed for image0 and for frame = 'cam0', and for nothing
else: without them no rectification map is made. image0: the image of camera 0 the colours come from, (H,W) gray or
(H,W,3) BGR, uint8 or uint16, of camera 0's imager size; None: color is None. frame: the coordinate system of the
points: 'ref' (the default: what mrcal-stereo writes), 'cam0', or 'rect0', the rectified camera 0. dtype: float64, or
float32, which is what a .ply holds.

A pixel (x,y) is KEPT when all of these hold:
  1. with d the disparity cast to uint16, as stereo_range() does: d > 0, d >= disparity_scaled_min,
     d <= disparity_scaled_max. disparity_min/max are the same bounds in pixels; an int16 image defaults the maximum
     to 0x7FFF, so that its negative "invalid" marks stay invalid
  2. its range, stereo_range()'s from the same device code, is finite and > 0. A negative LATLON range, which
     stereo_range() returns, is dropped here
  3. range_min <= range <= range_max, where given
  4. with image0: ix = floorf(mx + 0.5f), iy = floorf(my + 0.5f), additions in float32, of the float32 rectification
     map (mx,my) of camera 0 at (x,y), are finite and inside image0. The colour is image0[iy, ix]: the reference's
     nearest pixel of the original image, taken from the map instead of a projection of every point. A map entry of
     -0.5 exactly is inside here and outside in the reference
The point is range times the unit observation vector of (x,y), moved to `frame` by a transform made on the host, in
double and rounded once if dtype is float32; frame = 'rect0' makes no product and gives the bits of stereo_unproject(
disparity/disparity_scale, models_rectified, qrect0 = the pixel grid). The kept pixels come in ascending y Naz + x, which
is what index holds. Validity is decided once and stored a bit a pixel; an integer scan places every workgroup's
points: no atomics, the same bits on every call (csrc/point_cloud.hip). No CPU fallback.
The one-shot form of Rectification.point_cloud() (with models) and of StereoPointCloud.point_cloud() (without).
Reference: mrcal-stereo's --write-point-cloud; mrcal.stereo_unproject(), mrcal.write_point_cloud_as_ply()"""
    _validate_models_rectified(models_rectified)
    if models is not None and len(models) != 2:
        raise Exception("I need exactly 2 camera models")
    W, H = (int(x) for x in models_rectified[0].imagersize())
    _cloud_image(image0, "image0", models)
    _cloud_disparity(disparity, (H, W), disparity_scale, disparity_min, disparity_max, disparity_scaled_min, disparity_scaled_max)
    _cloud_frame(models_rectified, models, range_min, range_max, frame, dtype)
    kw = dict(disparity_scale=disparity_scale, disparity_min=disparity_min, disparity_max=disparity_max,
              disparity_scaled_min=disparity_scaled_min, disparity_scaled_max=disparity_scaled_max,
              range_min=range_min, range_max=range_max, frame=frame, dtype=dtype)
    if models is None:
        with StereoPointCloud(models_rectified) as c:
            return c.point_cloud(disparity, **kw)
    with Rectification(models, models_rectified) as r:
        return r.point_cloud(disparity, image0=image0, **kw)
