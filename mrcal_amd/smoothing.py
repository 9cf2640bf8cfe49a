"""The anti-aliasing Gaussian pre-filter: what an image wants before a remap makes it several times smaller.

    smoothed = mrcal_amd.smooth_gaussian(image, 2.0)                 # or (sigma_x, sigma_y); 0: that axis is left alone

    with mrcal_amd.ImageSmoother(image.shape, image.dtype, 2.0) as s:                  # the buffers are made once
        for image in images:
            smoothed = s.apply(image)

    # or where the images go next, on the device, between the upload (and the equalization) and the remap:
    small = mrcal_amd.transform_image(image, mapxy, antialias = 'auto')
    with mrcal_amd.Rectification(models, models_rectified) as r:
        disparity = r.disparity(image0, image1, disparity_max = 128, equalization = 'clahe', antialias = 'auto')

A bilinear remap reads 4 source pixels for an output pixel whatever the scale, so one that shrinks the image by 3-8 x,
as the rectification of a large pair down to the matcher's 256 disparities does, aliases. The reference has this on its
to-do list only (doc/news-3.0.org: "mrcal-stereo should have an anti-aliasing filter ... when I downsample, just before
mrcal.transform_image()", with cv2.GaussianBlur(sigmaX = 2)). The definition, to the bit, is in
include/mrcal_amd.h ("smoothing"); the kernel is csrc/smooth.hip, and there is no CPU fallback for it. Out of scope: colour
images, sigmas above 8 (halve the image first).
"""
import ctypes as C
import math
import numpy as np

from . import _handle
from ._cabi import _ptr
from ._handle import Handle
from ._images import GREY_DTYPES, grey_shape, grey_dtype, grey_image, out_like, apply_resident


_WORDS = ("smooth()", "smoothed", "an image that is filtered is grey", "smoother")
SIGMA_MIN, SIGMA_MAX, R_MAX = 0.5, 8.0, 24


class _SmoothParams(C.Structure):
    """mrcal_amd_smooth_params_t"""
    _fields_ = [("sigma_x", C.c_double), ("sigma_y", C.c_double)]


def _number(x):
    return isinstance(x, (int, float, np.integer, np.floating)) and not isinstance(x, (bool, np.bool_))


def _sigmas(sigma, what="sigma"):
    """a scalar or (sigma_x, sigma_y) -> (sigma_x, sigma_y), each 0 or in [0.5, 8]: the refusals of csrc/smooth_plan.hpp
    that need no image. Both 0 is NOT refused here: what that means is the caller's to say"""
    if _number(sigma):
        s = (float(sigma), float(sigma))
    else:
        try:    s = tuple(sigma)
        except TypeError: s = ()
        if len(s) != 2 or not all(_number(x) for x in s):
            raise Exception(f"smooth(): '{what}' must be a number or (sigma_x, sigma_y). Got {sigma!r}")
        s = (float(s[0]), float(s[1]))
    if not all(x == 0.0 or SIGMA_MIN <= x <= SIGMA_MAX for x in s):
        raise Exception(f"smooth(): a sigma is 0 (that axis is not filtered) or lies in [{SIGMA_MIN:g}, {SIGMA_MAX:g}]. Got ({s[0]:g},{s[1]:g})")
    return s


def _sigmas_to_run(sigma):
    s = _sigmas(sigma)
    if s == (0.0, 0.0):
        raise Exception("smooth(): both sigmas are 0: there is nothing to run")
    return s


def smooth_weights(sigma):
    """The integer taps w_0 .. w_R of one axis, int32 (R+1,), R = ceil(3 sigma); w_-k = w_k, and all of them sum to 256.
sigma: 0 (the one tap 256), or > 0 with R <= 24. Host code: no GPU is needed"""
    if not _number(sigma):
        raise Exception(f"smooth(): 'sigma' must be a number. Got {sigma!r}")
    lib, api = _handle._libs()
    R, w = C.c_int(0), np.zeros((R_MAX + 1,), dtype=np.int32)
    if not lib.lib.mrcal_amd_smooth_weights(float(sigma), C.byref(R), _ptr(w)):
        raise Exception("smooth() failed:" + api._last_error())
    return w[:R.value + 1].copy()


def antialias_sigma(mapxy):
    """The sigma that suits the remap through mapxy, float32 (H,W,2): half the decimation step's.

s: the larger of the two medians, over every 16th pixel in both directions, of |mapxy[y,x+1] - mapxy[y,x]| and of
|mapxy[y+1,x] - mapxy[y,x]| (the lengths of the differences: source pixels an output pixel; entries that are not finite
are skipped). The result is 0.5 sqrt(s^2 - 1), at most 8, and 0.0 where that is below 0.5: a remap that does not shrink
the image wants no filter. The factor 0.5 is a definition, not a measurement. Host numpy"""
    if not isinstance(mapxy, np.ndarray) or mapxy.ndim != 3 or mapxy.shape[2] != 2:
        raise Exception("smooth(): 'mapxy' must be an array of shape (H,W,2)")
    m = mapxy.astype(np.float64)

    def median_step(a, b):
        step = np.sqrt(((a - b)**2).sum(axis=-1))
        step = step[np.isfinite(step)]
        return float(np.median(step)) if step.size else 0.0
    s = max(median_step(m[::16, 1:][:, ::16], m[::16, :-1][:, ::16]),
            median_step(m[1:, ::16][::16], m[:-1, ::16][::16]))
    if s <= 1.0:
        return 0.0
    sigma = min(0.5*math.sqrt(s*s - 1.0), SIGMA_MAX)
    return sigma if sigma >= SIGMA_MIN else 0.0


def antialias_params(antialias, auto_sigma, images=()):
    """The keyword antialias = None | 'auto' | sigma | (sigma_x, sigma_y) that transform_image() and Rectification take
    -> mrcal_amd_smooth_params_t, or None: nothing runs. auto_sigma(): what 'auto' means there. Every refusal is made
    here, before any device work"""
    if antialias is None:
        return None
    if isinstance(antialias, str):
        if antialias != 'auto':
            raise Exception(f"smooth(): antialias must be None, 'auto', a sigma or (sigma_x, sigma_y), not {antialias!r}")
        s = auto_sigma()
        s = (s, s)
    else:
        s = _sigmas(antialias, "antialias")
    if s == (0.0, 0.0):
        return None
    for i, image in enumerate(images):
        grey_image(_WORDS, image, f"image{i}" if len(images) > 1 else "image")
    return _SmoothParams(*s)


class ImageSmoother(Handle):
    """smooth_gaussian(), resident: the device buffers for one image size and type are made once, and every apply() reuses
them.

    shape: (H,W); dtype: uint8 or uint16; sigma: a number or (sigma_x, sigma_y), each 0 or in [0.5, 8], not both 0.
      .apply(image, out=None)       -> the filtered image, of the image's shape and dtype
      .milliseconds()               how long the one launch of the last apply() took on the device, without the copies"""

    _destroy = "mrcal_amd_smoother_destroy"

    def __init__(self, shape, dtype, sigma):
        self.shape, self.dtype = grey_shape(_WORDS, shape), grey_dtype(_WORDS, dtype)
        self.sigma = _sigmas_to_run(sigma)
        p = _SmoothParams(*self.sigma)
        self._create("smooth()", "mrcal_amd_smoother_create", self.shape[1], self.shape[0], GREY_DTYPES[self.dtype], C.addressof(p))

    def apply(self, image, out=None):
        self._open()
        grey_image(_WORDS, image, "image", self.shape, self.dtype)
        return apply_resident(_WORDS, lambda a, o: self._call("smooth()", "mrcal_amd_smoother_apply", _ptr(a), _ptr(o)),
                              image, out, self.shape, self.dtype)

    def milliseconds(self):
        self._open()
        ms = C.c_float(0)
        self._call("smooth()", "mrcal_amd_smoother_milliseconds", C.addressof(ms))
        return float(ms.value)


def smooth_gaussian(image, sigma, out=None):
    """A separable Gaussian of a grey image in integers: uint8 or uint16 (H,W) in; the same shape and dtype out: a new
array, or `out`. sigma: a number or (sigma_x, sigma_y); each is 0 (that axis is not filtered) or lies in [0.5, 8].

  1. per axis: R = ceil(3 sigma) and the integer taps w_-R .. w_R of smooth_weights(sigma), which sum to 256
  2. T[y][x] = sum_k wx_k I[y][clamp(x + k)]; O[y][x] = (sum_k wy_k T[clamp(y + k)][x] + 32768) >> 16

The border is replicated; a constant image comes back unchanged. The exact definition is in include/mrcal_amd.h ("smoothing").
cv2 is no part of this project and no equality with cv2.GaussianBlur() is claimed: the tests hold the kernel
(csrc/smooth.hip) to two numpy transcriptions of that text (tests/smooth_checker.py), EQUAL in every pixel. Integers
only, no atomics: the same bits on every call. The one-shot form of ImageSmoother.apply()."""
    grey_image(_WORDS, image)
    sigma = _sigmas_to_run(sigma)
    out_like(_WORDS, out, image.shape, image.dtype)
    with ImageSmoother(image.shape, image.dtype, sigma) as s:
        return s.apply(image, out=out)
