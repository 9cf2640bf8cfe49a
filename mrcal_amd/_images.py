"""What the wrappers that take images check alike, before any device work: the arguments of a remap
(transform_image(), Rectification, the matchers) and the grey uint8 or uint16 image of the filters (smoothing.py,
equalization.py), whose refusals differ in a few words only. Private: no numerics happen here."""
import numpy as np


MAX_PIXELS = 1 << 28            # csrc/image_format.hpp: IMAGE_MAX_PIXELS
_DTYPES = {np.dtype(np.uint8): 0, np.dtype(np.uint16): 1, np.dtype(np.float32): 2}      # MRCAL_AMD_IMAGE_*
GREY_DTYPES = {np.dtype(np.uint8): 0, np.dtype(np.uint16): 1}


def _image_arguments(image, what="image"):
    """-> dense array, width, height, channels, dtype code"""
    if not isinstance(image, np.ndarray):
        raise Exception(f"'{what}' must be a numpy array")
    if image.dtype not in _DTYPES:
        raise Exception(f"'{what}' must have dtype uint8, uint16 or float32, not {image.dtype}")
    if not (image.ndim == 2 or (image.ndim == 3 and image.shape[2] == 3)) or image.size == 0:
        raise Exception(f"'{what}' must have shape (H,W) or (H,W,3), got {image.shape}")
    return np.ascontiguousarray(image), image.shape[1], image.shape[0], (1 if image.ndim == 2 else 3), _DTYPES[image.dtype]


def _remap_modes(borderMode, interpolation):
    if   borderMode is None or borderMode == 'constant'    or (not isinstance(borderMode, str) and borderMode == 0): border = 0
    elif                       borderMode == 'transparent' or (not isinstance(borderMode, str) and borderMode == 5): border = 5
    else: raise Exception(f"borderMode must be None, 'constant' (0) or 'transparent' (5), not {borderMode!r}")
    if   interpolation is None or interpolation == 'linear'  or (not isinstance(interpolation, str) and interpolation == 1): interp = 1
    elif                          interpolation == 'nearest' or (not isinstance(interpolation, str) and interpolation == 0): interp = 0
    else: raise Exception(f"interpolation must be None, 'linear' (1) or 'nearest' (0), not {interpolation!r}")
    return border, interp


def _border_values(borderValue, channels):
    b = np.atleast_1d(np.asarray(borderValue, dtype=np.float64)).ravel()
    if b.size == 1: b = np.repeat(b, channels)
    if b.size < channels:
        raise Exception(f"borderValue must be a scalar or have a value per channel ({channels}), got {b.size}")
    return np.ascontiguousarray(b[:channels])


def _output_array(out, shape, dtype, transparent):
    """-> (the dense array the library fills, the array to return)"""
    if out is None:
        o = np.zeros(shape, dtype=dtype)
        return o, o
    if not isinstance(out, np.ndarray) or out.shape != shape or out.dtype != dtype:
        raise Exception(f"'out' must be a numpy array of shape {shape} and dtype {np.dtype(dtype)}")
    if out.flags.c_contiguous:
        return out, out
    return (np.ascontiguousarray(out) if transparent else np.empty(shape, dtype=dtype)), out


# ---- a grey uint8 or uint16 image. words: what the caller's refusals say where they differ:
#      (the prefix "smooth()", what cannot be done "smoothed", what to tell about a colour image, the resident object)
def grey_shape(words, shape):
    try:    shape = tuple(int(n) for n in shape)
    except TypeError: shape = ()
    if len(shape) != 2:
        raise Exception(f"{words[0]}: shape must be (H,W), got {shape}")
    if shape[0] <= 0 or shape[1] <= 0 or shape[0]*shape[1] > MAX_PIXELS:
        raise Exception(f"{words[0]}: images of {shape[1]} x {shape[0]} pixels cannot be {words[1]}")
    return shape


def grey_dtype(words, dtype):
    try:    dtype = np.dtype(dtype)
    except TypeError: dtype = None
    if dtype is None or dtype not in GREY_DTYPES:
        raise Exception(f"{words[0]}: images are uint8 or uint16, not {dtype}")
    return dtype


def grey_image(words, image, what="image", shape=None, dtype=None):
    """the refusal of what is no grey uint8 or uint16 image; shape, dtype: those a resident object was made for"""
    if not isinstance(image, np.ndarray):
        raise Exception(f"{words[0]}: '{what}' must be a numpy array")
    if image.ndim == 3:
        raise Exception(f"{words[0]}: '{what}' must be a grayscale image of shape (H,W), got {image.shape}: {words[2]}")
    if image.ndim != 2:
        raise Exception(f"{words[0]}: '{what}' must be a grayscale image of shape (H,W), got {image.shape}")
    if image.dtype not in GREY_DTYPES:
        raise Exception(f"{words[0]}: '{what}' must have dtype uint8 or uint16, not {image.dtype}")
    grey_shape(words, image.shape)
    if shape is not None and (image.shape != shape or image.dtype != dtype):
        raise Exception(f"{words[0]}: this {words[3]} was made for images of shape {shape} and dtype {dtype}, got {image.shape} and {image.dtype}")


def out_like(words, out, shape, dtype):
    if out is not None and (not isinstance(out, np.ndarray) or out.shape != shape or out.dtype != dtype):
        raise Exception(f"{words[0]}: 'out' must be a numpy array of shape {shape} and dtype {np.dtype(dtype)}")


def apply_resident(words, call, image, out, shape, dtype_out):
    """What apply() of a resident filter does around its library call, call(dense image, dense result): -> the result,
    a new array or `out`. An `out` that is not dense, or overlaps the image, is filled afterwards"""
    out_like(words, out, shape, dtype_out)
    a = np.ascontiguousarray(image)
    overlaps = out is not None and (out is image or np.shares_memory(out, a))
    o, _ = _output_array(None if overlaps else out, shape, dtype_out, False)
    call(a, o)
    if out is None:
        return o
    if o is not out: out[...] = o
    return out
