"""Image equalization: what the reference's tools do to a raw image before they rectify and match it.

    image = mrcal_amd.equalize_clahe(image)                          # cv2.createCLAHE(), setClipLimit(8), apply()
    image = mrcal_amd.equalize_stretch(image16)                      # uint16 -> uint8, mrcal_image_uint8_load()'s stretch

    with mrcal_amd.ImageEqualizer(image.shape, image.dtype, method = 'clahe') as e:    # the buffers are made once
        for image in images:
            equalized = e.apply(image)

    # or where the images go next, on the device, between the upload and the remap:
    with mrcal_amd.Rectification(models, models_rectified) as r:
        disparity = r.disparity(image0, image1, disparity_max = 128, equalization = 'clahe')
    q1, diagnostics = mrcal_amd.match_feature(image0, image1, q0, H10 = H10, search_radius1 = 200, template_size1 = 41,
                                              equalization = 'clahe')

The definition, to the bit, is in include/mrcal_amd.h ("equalization"); the kernels are csrc/equalize.hip, and there is
no CPU fallback for them. Out of scope: the reference's 'fieldscale' equalization, colour input.
"""
import ctypes as C
import numpy as np

from ._cabi import _ptr
from ._handle import Handle
from ._images import GREY_DTYPES, grey_shape, grey_dtype, grey_image, out_like, apply_resident


EQUALIZE_NONE, EQUALIZE_CLAHE, EQUALIZE_STRETCH = 0, 1, 2
_METHODS = {None: EQUALIZE_NONE, 'clahe': EQUALIZE_CLAHE, 'stretch': EQUALIZE_STRETCH}
_WORDS = ("equalize()", "equalized", "convert a colour image first", "equalizer")
_MAX_TILES = 4096


class _EqualizeParams(C.Structure):
    """mrcal_amd_equalize_params_t"""
    _fields_ = [("method", C.c_int), ("clip_limit", C.c_double), ("tiles_x", C.c_int), ("tiles_y", C.c_int)]


def _method(method, none_allowed):
    if isinstance(method, str) and method in _METHODS:
        return _METHODS[method]
    if method is None and none_allowed:
        return EQUALIZE_NONE
    raise Exception(f"equalize(): the method must be {'None, ' if none_allowed else ''}'clahe' or 'stretch', not {method!r}")


def _clahe_arguments(clip_limit, tiles):
    """-> (clip_limit, tiles_x, tiles_y): the refusals of csrc/equalize_plan.hpp that need no image"""
    if isinstance(clip_limit, (bool, np.bool_)) or not isinstance(clip_limit, (int, float, np.integer, np.floating)) or clip_limit != clip_limit:
        raise Exception(f"equalize(): clip_limit must be a number. Got {clip_limit!r}")
    try:    t = tuple(tiles)
    except TypeError: t = ()
    if len(t) != 2 or any(isinstance(n, (bool, np.bool_)) or not isinstance(n, (int, np.integer)) for n in t):
        raise Exception(f"equalize(): tiles must be two integers (tiles_x, tiles_y). Got {tiles!r}")
    if t[0] < 1 or t[1] < 1 or t[0]*t[1] > _MAX_TILES:
        raise Exception(f"equalize(): tiles must be at least (1,1) and at most {_MAX_TILES} in all. Got ({t[0]},{t[1]})")
    return float(clip_limit), int(t[0]), int(t[1])


def _tiles_fit(shape, tiles_x, tiles_y):
    H, W = shape
    if W % tiles_x == 0 and H % tiles_y == 0:
        return
    px, py = tiles_x - W % tiles_x, tiles_y - H % tiles_y
    if px > W - 1 or py > H - 1:
        raise Exception(f"equalize(): an image of {W} x {H} pixels is too small for ({tiles_x},{tiles_y}) tiles: it would be padded by "
                        f"({px},{py}) pixels, and a reflection reaches ({W - 1},{H - 1})")


def equalization_params(equalization, clahe_clip_limit, clahe_tiles, images=()):
    """The keywords equalization = None | 'clahe' | 'stretch', clahe_clip_limit, clahe_tiles that Rectification and
    FeatureMatcher take -> (mrcal_amd_equalize_params_t or None, the dtype the equalized images have or None). Every
    refusal is made here, before any device work"""
    method = _method(equalization, True)
    if method == EQUALIZE_NONE:
        return None, None
    clip_limit, tiles_x, tiles_y = _clahe_arguments(clahe_clip_limit, clahe_tiles)
    for i, image in enumerate(images):
        grey_image(_WORDS, image, f"image{i}")
        if method == EQUALIZE_CLAHE:
            _tiles_fit(image.shape, tiles_x, tiles_y)
    dtype = None
    if len(images) > 0:
        dtype = np.dtype(np.uint8) if method == EQUALIZE_STRETCH else images[0].dtype
    return _EqualizeParams(method, clip_limit, tiles_x, tiles_y), dtype


class ImageEqualizer(Handle):
    """equalize_clahe() and equalize_stretch(), resident: the device buffers for one image size and type are made once,
and every apply() reuses them.

    shape: (H,W); dtype: uint8 or uint16; method: 'clahe' (clip_limit = 8.0, tiles = (8,8)) or 'stretch'.
      .apply(image, out=None)       -> the equalized image: of the image's dtype for 'clahe', uint8 for 'stretch'
      .stage_milliseconds()         how long the histograms, the LUTs and the interpolation of the last apply() took on
                                    the device, without the copies ('stretch': the extremes, 0, the map)"""

    _destroy = "mrcal_amd_equalizer_destroy"

    def __init__(self, shape, dtype, method='clahe', *, clip_limit=8.0, tiles=(8, 8)):
        self.shape, self.dtype = grey_shape(_WORDS, shape), grey_dtype(_WORDS, dtype)
        m = _method(method, False)
        clip_limit, tiles_x, tiles_y = _clahe_arguments(clip_limit, tiles)
        if m == EQUALIZE_CLAHE:
            _tiles_fit(self.shape, tiles_x, tiles_y)
        self.dtype_out = np.dtype(np.uint8) if m == EQUALIZE_STRETCH else self.dtype
        p = _EqualizeParams(m, clip_limit, tiles_x, tiles_y)
        self._create("equalize()", "mrcal_amd_equalizer_create", self.shape[1], self.shape[0], GREY_DTYPES[self.dtype], C.addressof(p))

    def apply(self, image, out=None):
        self._open()
        grey_image(_WORDS, image, "image", self.shape, self.dtype)
        return apply_resident(_WORDS, lambda a, o: self._call("equalize()", "mrcal_amd_equalizer_apply", _ptr(a), _ptr(o)),
                              image, out, self.shape, self.dtype_out)

    def stage_milliseconds(self):
        self._open()
        ms = np.zeros((3,), dtype=np.float32)
        self._call("equalize()", "mrcal_amd_equalizer_stage_milliseconds", _ptr(ms))
        return dict(zip(("histogram", "lut", "apply"), (float(x) for x in ms)))


def equalize_clahe(image, *, clip_limit=8.0, tiles=(8, 8), out=None):
    """Contrast-limited adaptive histogram equalization of a grey image: what cv2.createCLAHE(clipLimit = clip_limit,
tileGridSize = tiles).apply(image) is published to compute (OpenCV's clahe.cpp), which the reference's mrcal-stereo
--clahe and mrcal-triangulate --clahe apply with a clip limit of 8 to every image before they rectify and match it.
uint8 or uint16 (H,W) in; the same shape and dtype out: a new array, or `out`.

  1. if W is no multiple of tiles[0] or H none of tiles[1], the image is padded on the right and at the bottom up to
     the next multiple, BOTH sides, the divisible one by a whole tiles[.], by reflection (numpy.pad(mode = 'reflect'))
  2. per tile: the histogram is clipped at max(int(clip_limit tile_pixels / histSize), 1), the excess is handed back
     evenly, the remainder to every step-th bin, and the LUT is the prefix sum scaled to the value range in float32
  3. per pixel: the LUTs of the four tiles around it, read at its value, interpolated bilinearly in float32

The exact arithmetic, operation by operation, is in include/mrcal_amd.h ("equalization"). cv2 is no part of this
project: the tests hold the kernels (csrc/equalize.hip) to two numpy transcriptions of that text
(tests/equalize_checker.py), EQUAL in every pixel, and not to cv2 itself. clip_limit <= 0: nothing is clipped. Integer
histograms, no floating-point atomics: the same bits on every call. The one-shot form of ImageEqualizer.apply()."""
    grey_image(_WORDS, image)
    clip_limit, tiles_x, tiles_y = _clahe_arguments(clip_limit, tiles)
    _tiles_fit(image.shape, tiles_x, tiles_y)
    out_like(_WORDS, out, image.shape, image.dtype)
    with ImageEqualizer(image.shape, image.dtype, 'clahe', clip_limit=clip_limit, tiles=(tiles_x, tiles_y)) as e:
        return e.apply(image, out=out)


def equalize_stretch(image, *, out=None):
    """The image's values stretched to 0..255: out = uint8(0.5 + (v - min) 255 / (max - min)) in float32, truncated, with
min and max over the whole image. uint8 or uint16 (H,W) in, uint8 out: a new array, or `out`. What the reference's
mrcal_image_uint8_load() does to a 16-bit image (image.c), and mrcal-stereo --equalization stretch; unlike it, the true
extremes are used (its loop misses a maximum that comes before the first smaller pixel) and a constant image, for which
it divides by zero, gives all zeros. The one-shot form of ImageEqualizer.apply()."""
    grey_image(_WORDS, image)
    out_like(_WORDS, out, image.shape, np.uint8)
    with ImageEqualizer(image.shape, image.dtype, 'stretch') as e:
        return e.apply(image, out=out)
