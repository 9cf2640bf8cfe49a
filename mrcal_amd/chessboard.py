"""The calibration board detected on the GPU: from images to the corners a calibration starts from.

    corners = mrcal_amd.find_chessboard_corners(image, 10)                 # (10,10,2), or None: no whole board
    q, response, status = mrcal_amd.chessboard_corner_candidates(image)
    with mrcal_amd.ChessboardDetector(image.shape, image.dtype) as d:      # resident: the buffers are kept between images
        for image in images:
            corners = d.find_board(image, 10, 7)
    observations, indices_frame_camera, paths = \\
        mrcal_amd.compute_chessboard_corners(10, 10, globs_per_camera = ('frame*-cam0.pgm', 'frame*-cam1.pgm'),
                                             corners_cache_vnl = 'corners.vnl')

What a corner is is written once, in include/mrcal_amd.h ("chessboard corners"): an integer ChESS response of a blurred
image, its local maxima above a fraction of the largest, a cv2.cornerSubPix-style refinement in double, and the complete
W x H lattice among the refined points. The kernels are csrc/chessboard.hip and there is no CPU fallback for them; the
lattice is found on the host (csrc/chessboard_grid.cpp; chessboard_grid() here needs no GPU). The detector imitates
neither mrgingham nor cv2 pixel for pixel: it finds the same physical corners.
Reference: mrcal.compute_chessboard_corners() (mrcal/calibration.py), which runs mrgingham where this runs its own."""
import ctypes as C
import fnmatch
import glob
import io
import os
import re
import sys
import tempfile

import numpy as np

from . import _handle
from ._cabi import _ptr
from ._handle import Handle, _failed
from .utils import mapping_file_framenocameraindex

_CB_MIN_SIDE = 32
_CB_MAX_PIXELS = 1 << 28
_CB_NMS_RADIUS_MAX = 16
_CB_MAX_CANDIDATES = 65536
_CB_MAX_LEVELS = 8
_CB_DTYPES = {np.dtype(np.uint8): 1, np.dtype(np.uint16): 2}
_CB_STAGES = ("upload", "response", "candidates", "refine", "grid")
STATUS_OK, STATUS_SINGULAR, STATUS_LEFT_WINDOW = 0, 1, 2
_WHAT = "find_chessboard_corners()"        # what a failed call of the detector says it was


class _Params(C.Structure):
    """mrcal_amd_chessboard_params_t"""
    _fields_ = [("threshold_256", C.c_int), ("nms_radius", C.c_int), ("max_candidates", C.c_int)]


def _dtype(dtype):
    try:    dtype = np.dtype(dtype)
    except TypeError: dtype = None
    if dtype not in _CB_DTYPES:
        raise Exception(f"find_chessboard_corners(): images must have dtype uint8 or uint16, not {dtype}")
    return dtype


def _shape(shape):
    """the refusals of csrc/chessboard_plan.hpp, before any device work"""
    if len(shape) != 2:
        raise Exception(f"find_chessboard_corners() accepts ONLY grayscale images of shape (H,W), got {tuple(shape)}")
    H, W = (int(x) for x in shape)
    if W < _CB_MIN_SIDE or H < _CB_MIN_SIDE:
        raise Exception(f"find_chessboard_corners(): an image of {W} x {H} pixels is too small: at least {_CB_MIN_SIDE} x {_CB_MIN_SIDE}")
    if W*H > _CB_MAX_PIXELS:
        raise Exception(f"find_chessboard_corners(): an image of {W} x {H} pixels is too large: at most {_CB_MAX_PIXELS} pixels")
    return H, W


def _params(threshold_256, nms_radius, max_candidates):
    for name, value, lo, hi in (("threshold_256", threshold_256, 0, 255), ("nms_radius", nms_radius, 1, _CB_NMS_RADIUS_MAX),
                                ("max_candidates", max_candidates, 1, _CB_MAX_CANDIDATES)):
        if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not lo <= value <= hi:
            raise Exception(f"find_chessboard_corners(): {name} must be in {lo}..{hi}, got {value}")
    return _Params(int(threshold_256), int(nms_radius), int(max_candidates))


def _pyramid_levels(pyramid_levels, shape=None):
    """the refusals of chessboard_pyramid_plan(); shape: (H,W), already looked at by _shape()"""
    n = pyramid_levels
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 0 <= n <= _CB_MAX_LEVELS:
        raise Exception(f"find_chessboard_corners(): pyramid_levels must be in 0..{_CB_MAX_LEVELS}, got {n}")
    if shape is not None:
        H, W = shape
        most = 0
        while most < _CB_MAX_LEVELS and min(W >> (most + 1), H >> (most + 1)) >= _CB_MIN_SIDE: most += 1
        if n > most:
            raise Exception(f"find_chessboard_corners(): an image of {W} x {H} pixels is too small for pyramid_levels = {n}: "
                            f"level {most + 1} would have {W >> (most + 1)} x {H >> (most + 1)} pixels, at least "
                            f"{_CB_MIN_SIDE} x {_CB_MIN_SIDE}; at most pyramid_levels = {most}")
    return int(n)


def _image(image, shape=None, dtype=None):
    if not isinstance(image, np.ndarray) or image.ndim != 2:
        raise Exception("find_chessboard_corners() accepts ONLY grayscale images of shape (H,W)" +
                        (f", got {image.shape}" if isinstance(image, np.ndarray) else ""))
    _dtype(image.dtype)
    if shape is None:
        _shape(image.shape)
    elif image.shape != shape or image.dtype != dtype:
        raise Exception(f"find_chessboard_corners(): this detector was made for images of shape {shape} and dtype {dtype}, "
                        f"got {image.shape} and {image.dtype}")
    return np.ascontiguousarray(image)


def _board(W, H):
    if H is None: H = W
    for n in (W, H):
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 3 <= n <= 256:
            raise Exception(f"find_chessboard_corners(): a board has 3..256 corners a side, got {W} x {H}")
    return int(W), int(H)


class ChessboardDetector(Handle):
    """find_chessboard_corners() resident: the device buffers for one shape and dtype of image are made once and every
call reuses them.

    shape: (H,W) of the images; dtype: uint8 or uint16; threshold_256, nms_radius, max_candidates, pyramid_levels: as
    in find_chessboard_corners()
      .candidates(image)        -> (q (N,2) float64, response (N,) int32, status (N,) int32); .overflow: more than
                                   max_candidates were found, and the first in row-major order were kept. Level 0 alone
      .find_board(image, W, H=None, return_levels=False)  -> (H,W,2) float64, or None; with return_levels
                                   (corners, levels (H,W) int32) or (None, None). With pyramid_levels > 0 the board is
                                   looked for from the coarsest level down and each corner is refined as far down as
                                   the levels agree; .detection_level: where it was found (None: nowhere)
      .response()               -> (the int32 response image, its maximum, the pixels (N,2) int32 of the candidates)
                                   of the level the last call looked at last: (H,W) without a pyramid. After a
                                   find_board() through the levels the pixels are None: their number stays inside
      .level_image(level)       the image of a level of the last call, as the device holds it
      .stage_milliseconds()     how long the upload, the response, the candidates, the refinement (on the device) and
                                the lattice (on the host; 0 after candidates()) of the last call took; with a pyramid,
                                of the level it looked at last
      .pyramid_milliseconds()   of the last find_board() through the levels: dict(decimate, descent: on the device;
                                per_level: the host's clock around each level tried, 0 for the others)
      .close(); a context manager"""

    _destroy = "mrcal_amd_chessboard_detector_destroy"

    def __init__(self, shape, dtype=np.uint8, *, threshold_256=51, nms_radius=7, max_candidates=4096, pyramid_levels=0):
        self.overflow, self._N = False, 0
        self.detection_level, self._last_level = None, 0
        self.shape = _shape(shape)
        self.dtype = _dtype(dtype)
        p = _params(threshold_256, nms_radius, max_candidates)
        self.pyramid_levels = _pyramid_levels(pyramid_levels, self.shape)
        self.max_candidates = p.max_candidates
        if self.pyramid_levels == 0:
            self._create(_WHAT, "mrcal_amd_chessboard_detector_create", self.shape[1], self.shape[0], _CB_DTYPES[self.dtype],
                         C.addressof(p), 0)
        else:
            self._create(_WHAT, "mrcal_amd_chessboard_detector_create_pyramid", self.shape[1], self.shape[0],
                         _CB_DTYPES[self.dtype], C.addressof(p), self.pyramid_levels, 0)

    def candidates(self, image):
        self._open()
        image = _image(image, self.shape, self.dtype)
        q = np.zeros((self.max_candidates, 2), dtype=np.float64)
        response, status = (np.zeros((self.max_candidates,), dtype=np.int32) for _ in range(2))
        N, overflow = C.c_int(0), C.c_int(0)
        self._call(_WHAT, "mrcal_amd_chessboard_detector_candidates", _ptr(image), C.addressof(N), C.addressof(overflow),
                   _ptr(q), _ptr(response), _ptr(status))
        self.overflow, self._N = bool(overflow.value), N.value
        self.detection_level, self._last_level = None, 0
        return q[:N.value].copy(), response[:N.value].copy(), status[:N.value].copy()

    def find_board(self, image, W, H=None, return_levels=False):
        self._open()
        W, H = _board(W, H)
        image = _image(image, self.shape, self.dtype)
        corners = np.zeros((H, W, 2), dtype=np.float64)
        found = C.c_int(0)
        if self.pyramid_levels == 0 and not return_levels:
            self._call(_WHAT, "mrcal_amd_chessboard_detector_find_board", _ptr(image), W, H, C.addressof(found), _ptr(corners))
            self.detection_level, self._last_level = (0 if found.value else None), 0
            return corners if found.value else None
        levels = np.zeros((H, W), dtype=np.int32)
        detection_level = C.c_int(-1)
        self._call(_WHAT, "mrcal_amd_chessboard_detector_find_board_pyramid", _ptr(image), W, H, _ptr(corners), _ptr(levels),
                   C.addressof(detection_level), C.addressof(found))
        self.detection_level = detection_level.value if found.value else None
        self._last_level = detection_level.value if found.value else 0
        # (the candidates response() speaks of are the last level's; their number is not handed out by this call)
        self._N = None
        if not return_levels:
            return corners if found.value else None
        return (corners, levels) if found.value else (None, None)

    def level_shape(self, level):
        """(H,W) of a level of the pyramid"""
        return self.shape[0] >> level, self.shape[1] >> level

    def level_image(self, level):
        self._open()
        if isinstance(level, bool) or not isinstance(level, (int, np.integer)) or not 0 <= level <= self.pyramid_levels:
            raise Exception(f"find_chessboard_corners(): this detector has the levels 0..{self.pyramid_levels}, and level {level} was asked for")
        out = np.zeros(self.level_shape(int(level)), dtype=self.dtype)
        self._call(_WHAT, "mrcal_amd_chessboard_detector_read_level", int(level), _ptr(out))
        return out

    def pyramid_milliseconds(self):
        self._open()
        decimate, descent = C.c_float(0), C.c_float(0)
        per_level = np.zeros((self.pyramid_levels + 1,), dtype=np.float32)
        self._call(_WHAT, "mrcal_amd_chessboard_detector_pyramid_milliseconds", C.addressof(decimate), C.addressof(descent),
                   _ptr(per_level))
        return dict(decimate=float(decimate.value), descent=float(descent.value), per_level=[float(x) for x in per_level])

    def response(self):
        self._open()
        R = np.zeros(self.level_shape(self._last_level), dtype=np.int32)
        xy = np.zeros((self.max_candidates, 2), dtype=np.int32)
        Rmax = C.c_int32(0)
        self._call(_WHAT, "mrcal_amd_chessboard_detector_read_response", _ptr(R), C.addressof(Rmax), _ptr(xy))
        if self._N is None:
            return R, int(Rmax.value), None
        return R, int(Rmax.value), xy[:self._N].copy()

    def stage_milliseconds(self):
        self._open()
        ms = np.zeros((len(_CB_STAGES),), dtype=np.float32)
        self._call(_WHAT, "mrcal_amd_chessboard_detector_stage_milliseconds", _ptr(ms))
        return dict(zip(_CB_STAGES, (float(x) for x in ms)))


def chessboard_corner_candidates(image, *, threshold_256=51, nms_radius=7, max_candidates=4096):
    """The refined corner candidates of a grey image: (q (N,2) float64, response (N,) int32, status (N,) int32)

Parts a..d of the definition (include/mrcal_amd.h, "chessboard corners"), in row-major order of the pixels the
candidates were found at. status: 0, or 1 (the gradient matrix was singular) or 2 (the refinement left the +-3.5 px box
around its start), with NaN coordinates. The N = 1 case of ChessboardDetector.candidates()."""
    image = _image(image)
    _params(threshold_256, nms_radius, max_candidates)
    with ChessboardDetector(image.shape, image.dtype, threshold_256=threshold_256, nms_radius=nms_radius,
                            max_candidates=max_candidates) as d:
        return d.candidates(image)


def find_chessboard_corners(image, W, H=None, *, threshold_256=51, nms_radius=7, max_candidates=4096, pyramid_levels=0,
                            return_levels=False):
    """The W x H corners of the calibration board in a grey image: an (H,W,2) float64 array, or None

image: (height,width) uint8 or uint16; colour images are refused. W, H: the corners a row and a column of the board
(H = None: W). Only a WHOLE board is returned, like mrgingham. The order is row-major and proper: with the image's y
pointing down, +i (along a row of the board) cross +j is positive, and of the labellings that are, the one whose +i
points most along the image's +x is chosen.

A corner: a local maximum (window 2 nms_radius + 1) of the integer ChESS response of the [1 2 1] x [1 2 1] blurred
image, above threshold_256/256 of the largest response, refined in double by the fixed point of cv2.cornerSubPix (an
11 x 11 Gaussian window on the original image). At most max_candidates candidates are looked at. The definition, to the
bit: include/mrcal_amd.h, "chessboard corners". The image kernels run on the GPU (csrc/chessboard.hip; no CPU
fallback); the lattice among the candidates is found on the host. The one-shot form of ChessboardDetector.find_board().

pyramid_levels = n > 0 (0..8; every level keeps 32 pixels a side): for corners blurred over several pixels and boards
whose squares cover hundreds of pixels. The image is halved n times (2 x 2 means), the board is looked for from the
coarsest level down, and each of its corners is then refined level by level towards the image for as long as the
refinement agrees with where it started within 0.3 px ("chessboard corners", p1-p3). The corners are always in pixels
of the image. return_levels: (corners, levels) or (None, None); levels (H,W) int32: the level each corner's position
was taken at, what compute_chessboard_corners() writes as the level whose weight is 2^-level. All 0 without a pyramid."""
    image = _image(image)
    _params(threshold_256, nms_radius, max_candidates)
    _pyramid_levels(pyramid_levels, image.shape)
    _board(W, H)
    with ChessboardDetector(image.shape, image.dtype, threshold_256=threshold_256, nms_radius=nms_radius,
                            max_candidates=max_candidates, pyramid_levels=pyramid_levels) as d:
        return d.find_board(image, W, H, return_levels=return_levels)


def chessboard_grid(q, W, H=None, *, response=None, status=None):
    """The W x H board among the points q (N,2), in the order of find_chessboard_corners(), or None. Host code: no GPU"""
    W, H = _board(W, H)
    q = np.ascontiguousarray(q, dtype=np.float64)
    if q.ndim != 2 or q.shape[1] != 2:
        raise Exception(f"chessboard_grid(): q must have shape (N,2), got {q.shape}")
    N = q.shape[0]
    if response is not None: response = np.ascontiguousarray(response, dtype=np.int32).reshape(N)
    if status   is not None: status   = np.ascontiguousarray(status,   dtype=np.int32).reshape(N)
    lib, _ = _handle._libs()
    corners = np.zeros((H, W, 2), dtype=np.float64)
    found = C.c_int(0)
    if not lib.lib.mrcal_amd_chessboard_grid(N, _ptr(q), _ptr(response), _ptr(status), W, H, C.addressof(found), _ptr(corners)):
        raise _failed("chessboard_grid()")
    return corners if found.value else None


# ---------------------------------------------------------------------------------------------------------------------
# images from disk

def _read_pgm(filename):
    """binary PGM (P5), 8 or 16 bit (big-endian, as the format has it) -> (H,W) uint8 or uint16"""
    with open(filename, "rb") as f:
        data = f.read()
    # the header: magic, width, height, maxval, separated by whitespace and comments, then ONE whitespace byte
    fields, at = [], 0
    while len(fields) < 4:
        m = re.compile(rb"\s*(?:#[^\n]*\n\s*)*(\S+)").match(data, at)
        if m is None:
            raise Exception(f"Couldn't load image '{filename}': the PGM header is cut short")
        fields.append(m.group(1))
        at = m.end()
    try:    W, H, maxval = (int(x) for x in fields[1:])
    except ValueError: W = H = maxval = 0
    if fields[0] != b"P5" or W <= 0 or H <= 0 or not 0 < maxval < 65536:
        raise Exception(f"Couldn't load image '{filename}': not a binary PGM (P5) header")
    at += 1
    dtype = np.dtype(np.uint8) if maxval < 256 else np.dtype(">u2")
    if len(data) - at < W*H*dtype.itemsize:
        raise Exception(f"Couldn't load image '{filename}': {len(data) - at} bytes of pixels, {W*H*dtype.itemsize} expected")
    image = np.frombuffer(data, dtype=dtype, count=W*H, offset=at).reshape(H, W)
    return np.ascontiguousarray(image, dtype=np.uint8 if maxval < 256 else np.uint16)


def load_image_gray(filename):
    """An image file as an (H,W) uint8 or uint16 array. Binary PGM (P5) is read with numpy; every other format goes
through PIL, if that can be imported, and is converted to 8-bit grey unless it holds 16-bit grey"""
    with open(filename, "rb") as f:
        magic = f.read(2)
    if magic == b"P5":
        return _read_pgm(filename)
    try:
        from PIL import Image
    except ImportError:
        raise Exception(f"Couldn't load image '{filename}': only binary PGM (P5) is read without PIL, and PIL cannot be imported")
    with Image.open(filename) as im:
        if im.mode in ("I;16", "I;16L", "I;16B"):
            return np.ascontiguousarray(np.asarray(im), dtype=np.uint16)
        return np.ascontiguousarray(np.asarray(im.convert("L")), dtype=np.uint8)


# ---------------------------------------------------------------------------------------------------------------------
# compute_chessboard_corners()

def _parse_corner(out, fields, line, weight_column_kind):
    """the fields after the filename of a row of a corners file -> out (3,) = (x, y, weight); True: the point is
    valid. out comes in as (-1,-1,-1): invalid"""
    if fields[0] == '-' or fields[1] == '-':
        return False
    try:
        out[0], out[1] = float(fields[0]), float(fields[1])
    except Exception:
        raise Exception(f"'corners.vnl' data rows must lead with 'filename x y' with x and y being numerical or '-'. Instead got line '{line}'")
    if out[0] < 0 or out[1] < 0:
        return False
    if len(fields) == 2 or weight_column_kind is None:
        out[2] = 1.0
        return True
    if fields[2] == '-':
        return False
    try:
        w = float(fields[2])
    except Exception:
        raise Exception(f"'corners.vnl' data rows expected as 'filename x y {weight_column_kind}' with {weight_column_kind} being numerical or '-'. Instead got line '{line}'")
    if weight_column_kind == 'weight':
        if w <= 0.0:
            return False
        out[2] = w
    else:
        if w < 0.0:
            return False
        out[2] = 1. / (1 << int(w))         # the decimation level: the weight is 2^-level
    return True


def _detect_into_vnl(W, H, globs_per_camera, detector_params):
    """the lines of the corners file of the images the globs match, this detector in mrgingham's place"""
    yield "# filename x y level\n"
    detectors = {}
    try:
        for g in globs_per_camera:
            for filename in sorted(glob.glob(g)):
                image = load_image_gray(filename)
                key = (image.shape, image.dtype)
                if key not in detectors:
                    detectors[key] = ChessboardDetector(image.shape, image.dtype, **detector_params)
                d = detectors[key]
                if d.pyramid_levels == 0: corners = d.find_board(image, W, H)
                else:                     corners, levels = d.find_board(image, W, H, return_levels=True)
                if corners is None:
                    yield f"{filename} - - -\n"
                else:
                    if d.pyramid_levels == 0: levels = np.zeros(corners.shape[:2], dtype=np.int32)
                    for (x, y), level in zip(corners.reshape(-1, 2), levels.ravel()):
                        yield f"{filename} {float(x)!r} {float(y)!r} {int(level)}\n"        # (repr: the float64 comes back to the bit)
    finally:
        for d in detectors.values():
            d.close()


def compute_chessboard_corners(W, H, *, globs_per_camera=('*',), corners_cache_vnl=None, image_path_prefix=None,
                               image_directory=None, jobs=1, exclude_images=set(), weight_column_kind='level',
                               Npoint_observations_per_board_min=None, **detector_params):
    """The chessboard observations of a set of images, in the form a calibration takes

    observations, indices_frame_camera, paths = \\
        mrcal_amd.compute_chessboard_corners(10, 10, globs_per_camera = ('frame*-cam0.pgm', 'frame*-cam1.pgm'),
                                             corners_cache_vnl = "corners.vnl")

The signature, the messages and the returned values of the reference's mrcal.compute_chessboard_corners(). W, H: the
corners of the board. globs_per_camera: a glob of image filenames for each camera; the part of the names that varies
inside a camera is the frame number. corners_cache_vnl: a filename, or a file object to read from. If it exists (or is a
file object) the corners are READ from it and no image is opened: a vnlog of rows "filename x y" or "filename x y
level-or-weight", a board's W*H rows after each other, "-" for a point that was not seen. weight_column_kind: 'level'
(the weight is 2^-level; '-' or < 0: weight -1, the point is ignored), 'weight' (the column is the weight; '-' or <= 0:
ignored), None (weight 1). The paths of the file are used as follows: with image_path_prefix, prefixed with it;
else with image_directory, their directory replaced by it; else, when reading a file on disk and the path is relative
and does not exist relative to the current directory, prefixed with the file's directory; else as they are. Files in
exclude_images, files that match no glob and boards with no more than Npoint_observations_per_board_min (default
2 min(W,H)) valid points are dropped.

If the file does not exist, the reference runs mrgingham; here find_chessboard_corners() runs instead, on the GPU,
over the images the globs match, and the same vnlog is written ("# filename x y level", level 0; "filename - - -" for
an image without a whole board), atomically: to a temporary file that is renamed. jobs: jobs < 0 says that the file MUST
exist already; otherwise the number is not used: the images go through one device one after the other. The reference's
refusal of W != H ("mrgingham currently accepts ONLY square grids") does NOT apply: this detector finds rectangular
boards. Binary PGM images (P5, 8 and 16 bit) are read natively; other formats through PIL where it is installed.
detector_params: threshold_256, nms_radius, max_candidates, pyramid_levels of find_chessboard_corners(), each as a
keyword of its own or all in one dict, detector_params={'pyramid_levels': 3}. With pyramid_levels > 0 the level column holds the level each corner was refined at, which comes back as the weight 2^-level.

Returns (observations (N,H,W,3) of (x, y, weight), indices_frame_camera (N,2) int32, contiguous and sorted, the N
paths). Reference: mrcal/calibration.py, compute_chessboard_corners()"""
    if not (weight_column_kind == 'level' or weight_column_kind == 'weight' or weight_column_kind is None):
        raise Exception(f"weight_column_kind must be one of ('level','weight',None); got '{weight_column_kind}'")
    if Npoint_observations_per_board_min is None:
        Npoint_observations_per_board_min = 2*min(W, H)
    if isinstance(detector_params.get("detector_params"), dict):
        # (the detector's keywords given as ONE dict, detector_params={'pyramid_levels': 3}, or each on its own)
        detector_params = dict(detector_params.pop("detector_params"), **detector_params)

    globs_per_camera = [os.path.normpath(g) for g in globs_per_camera]
    Ncameras = len(globs_per_camera)
    files_per_camera = [[] for _ in range(Ncameras)]
    is_file_object = isinstance(corners_cache_vnl, io.IOBase)
    corners_dir = None
    if corners_cache_vnl is not None and not is_file_object:
        if os.path.isdir(corners_cache_vnl):
            raise Exception(f"Given cache path '{corners_cache_vnl}' is a directory. Must be a file or must not exist")
        corners_dir = os.path.dirname(corners_cache_vnl)

    write_fd, write_tmp, opened = None, None, None
    if corners_cache_vnl is not None and (is_file_object or os.path.exists(corners_cache_vnl)):
        lines = corners_cache_vnl if is_file_object else open(corners_cache_vnl, 'r', encoding='ascii')
        if not is_file_object: opened = lines
    else:
        if jobs < 0:
            raise Exception("I was asked to use an existing cache file, but it couldn't be read. jobs<0, so I do not recompute")
        if weight_column_kind == 'weight':
            raise Exception("Need to run the detector, so I will get a column of decimation levels, but weight_column_kind == 'weight'")
        checked = dict(dict(threshold_256=51, nms_radius=7, max_candidates=4096, pyramid_levels=0), **detector_params)
        _pyramid_levels(checked.pop("pyramid_levels"))
        _params(**checked)
        sys.stderr.write("Computing chessboard corners with find_chessboard_corners() of the images matching:\n   {}\n".format(' '.join(globs_per_camera)))
        if corners_cache_vnl is not None:
            # (in the cache's own directory, so that the rename is one)
            write_fd, write_tmp = tempfile.mkstemp('.vnl', dir=corners_dir or '.')
            sys.stderr.write(f"Will save corners to '{corners_cache_vnl}'\n")
        lines = _detect_into_vnl(W, H, globs_per_camera, detector_params)

    globs_matched = [g if g[0] == '/' else '*/' + g for g in globs_per_camera]
    mapping = {}

    def new_board():
        return dict(f='', igrid=0, Nvalid=0, grid=-np.ones((H*W, 3), dtype=float))

    def finish(board):
        if board['igrid'] <= 1:
            return
        if W*H != board['igrid']:
            raise Exception("File '{}' expected to have {} points, but got {}".format(board['f'], W*H, board['igrid']))
        if board['f'] in exclude_images or not board['Nvalid'] > Npoint_observations_per_board_min:
            return
        f = board['f']
        if image_path_prefix is not None:   path = f"{image_path_prefix}/{f}"
        elif image_directory is not None:   path = f"{image_directory}/{os.path.basename(f)}"
        elif corners_dir is not None and f[0] != '/' and not os.path.exists(f):
                                            path = f"{corners_dir}/{f}"
        else:                               path = os.path.normpath(f)
        for icam in range(Ncameras):
            if fnmatch.fnmatch(os.path.abspath(path), globs_matched[icam]):
                files_per_camera[icam].append(path)
                mapping[path] = board['grid'].reshape(H, W, 3)
                return

    try:
        board = new_board()
        for line in lines:
            if write_fd is not None:
                os.write(write_fd, line.encode())
            if re.match(r'\s*#', line):
                continue
            m = re.match(r'\s*(\S+)\s+(.*?)$', line)
            if m is None:
                raise Exception(f"Unexpected line in the corners output: '{line}'")
            if board['f'] != m.group(1):
                finish(board)
                board = new_board()
                board['f'] = m.group(1)
            fields = m.group(2).split()
            if not (len(fields) == 2 or len(fields) == 3):
                raise Exception(f"'corners.vnl' data rows must contain a filename and 2 or 3 values. Instead got line '{line}'")
            if board['igrid'] < H*W:
                if _parse_corner(board['grid'][board['igrid']], fields, line, weight_column_kind):
                    board['Nvalid'] += 1
            board['igrid'] += 1
        finish(board)
        if write_fd is not None:
            os.close(write_fd)
            write_fd = None
            os.replace(write_tmp, corners_cache_vnl)
            write_tmp = None
            sys.stderr.write("Done computing chessboard corners\n")
    finally:
        if opened is not None: opened.close()
        if write_fd is not None: os.close(write_fd)
        if write_tmp is not None and os.path.exists(write_tmp): os.remove(write_tmp)

    min_num_images = 2 if Ncameras > 1 else 1
    for icam in range(Ncameras):
        N = len(files_per_camera[icam])
        if N < min_num_images:
            raise Exception("Found too few ({}; need at least {}) images containing a calibration pattern in camera {}; glob '{}'".format(
                N, min_num_images, icam, globs_matched[icam]))

    file_framenocameraindex = mapping_file_framenocameraindex(*files_per_camera)
    files_sorted = sorted(mapping.keys(), key=lambda f: file_framenocameraindex[f][1])
    files_sorted = sorted(files_sorted,   key=lambda f: file_framenocameraindex[f][0])
    indices_frame_camera = np.zeros((len(files_sorted), 2), dtype=np.int32)
    observations = np.zeros((len(files_sorted), H, W, 3), dtype=float)
    index_frame, iframe_last = -1, None
    for i, f in enumerate(files_sorted):
        # (the frame indices are consecutive from 0, not the numbers in the names)
        iframe, icam = file_framenocameraindex[f]
        if iframe_last is None or iframe_last != iframe:
            index_frame += 1
            iframe_last = iframe
        indices_frame_camera[i] = (index_frame, icam)
        observations[i] = mapping[f]
    return observations, indices_frame_camera, files_sorted
