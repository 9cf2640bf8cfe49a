"""Sampling the imager on a grid (mrcal/utils.py:268-437): sample_imager() is host numpy, sample_imager_unproject()
runs over unproject() (the GPU). write_point_cloud_as_ply() (mrcal/utils.py:1578-1750) is host numpy."""
import numpy as np


def sample_imager(gridn_width, gridn_height, imager_width, imager_height):
    """Regularly-sampled pixel coordinates across the imager, (gridn_height,gridn_width,2): [0,0] = (0,0),
    [-1,-1] = (imager_width-1,imager_height-1). gridn_height=None: int(round(imager_height/imager_width*gridn_width))"""
    if gridn_height is None:
        gridn_height = int(round(imager_height/imager_width*gridn_width))
    w = np.linspace(0, imager_width  - 1, gridn_width)
    h = np.linspace(0, imager_height - 1, gridn_height)
    return np.ascontiguousarray(np.stack(np.meshgrid(w, h), axis=-1))


def sample_imager_unproject(gridn_width, gridn_height, imager_width, imager_height, lensmodel, intrinsics_data,
                            normalize=False):
    """(v, q): the grid q of sample_imager() and its unprojection v (gridn_height,gridn_width,3); with a list or tuple
    of lens models (and as many intrinsics) v is (Ncameras,gridn_height,gridn_width,3), all of the one grid"""
    from . import unproject
    grid = sample_imager(gridn_width, gridn_height, imager_width, imager_height)
    if isinstance(lensmodel, (list, tuple)):
        return np.array([unproject(grid, lensmodel[i], intrinsics_data[i], normalize=normalize)
                         for i in range(len(lensmodel))]), grid
    return unproject(grid, lensmodel, intrinsics_data, normalize=normalize), grid


def write_point_cloud_as_ply(filename, points, *, color=None, binary=True):
    """Writes a point cloud to a .ply file

points: (N,3); or (N,4), a grayscale intensity in the last column; or (N,6), a BGR colour in the last three. color: the
colours apart from the points, which are (N,3) then: (N,) grayscale or (N,3) BGR. The file holds float32 x y z and, per
point, `uchar intensity` or `uchar red green blue` (BGR in, RGB out). binary: little-endian binary (the default) or ascii.
The argument forms, the checks and their messages are the reference's. Departures:
  - ascii writes exactly the properties the header declares, the coordinates as %.9g, which a float32 survives. The
    reference writes %.1f and, for BGR, a seventh column that its header does not declare
  - uint16 colours, and colours of any type outside 0..255, are refused; the reference truncates them
  - N = 0 writes a valid file with no vertices
Host numpy: needs no GPU. Reference: mrcal.write_point_cloud_as_ply()"""
    points = np.asarray(points)
    if points.ndim != 2:
        raise Exception(f"points.shape must be (N,3) or (N,4) or (N,6), but points.ndim={points.ndim}")
    N, Ntrailing = points.shape
    if not (Ntrailing == 3 or Ntrailing == 4 or Ntrailing == 6):
        raise Exception(f"points.shape[-1] must be one of (3,4,6) to indicate no-color or grayscale or bgr colors respectively. Instead got points.shape[-1] = {points.shape[-1]}")
    if color is not None:
        color = np.asarray(color)
        if Ntrailing != 3:
            raise Exception("Both 'points' and 'color' are specifying color information. At most one of those should provide it")
        if color.ndim > 2:
            raise Exception(f"color.shape must be (N,) or (N,3), but color.ndim={color.ndim}")
        if color.ndim < 1 or N != color.shape[0]:
            raise Exception(f"Inconsistent point counts: len(points)={len(points)} but len(color)={len(color) if color.ndim else 0}")
        if not (color.shape == (N,) or color.shape == (N, 3)):
            raise Exception(f"color.shape must be (N,) or (N,3), but color.shape={color.shape}")
        if color.dtype == np.uint16:
            raise Exception("write_point_cloud_as_ply(): colours are written as uchar, and uint16 colours would be truncated: scale them to uint8 first")
    elif Ntrailing == 4:
        color, points = points[:, 3], points[:, :3]
    elif Ntrailing == 6:
        color, points = points[:, 3:], points[:, :3]

    # points (N,3); color None, (N,) or (N,3)
    if color is not None and color.size and not (np.all(color >= 0) and np.all(color <= 255)):
        raise Exception("write_point_cloud_as_ply(): colours are written as uchar and must lie in 0..255")
    if color is None:
        dtype, header_color = np.dtype([('xyz', '<f4', 3)]), ''
    elif color.ndim == 1:
        dtype, header_color = np.dtype([('xyz', '<f4', 3), ('i', np.uint8)]), 'property uchar intensity\n'
    else:
        dtype, header_color = np.dtype([('xyz', '<f4', 3), ('rgb', np.uint8, 3)]), 'property uchar red\nproperty uchar green\nproperty uchar blue\n'
    header = (f"ply\nformat {'binary_little_endian' if binary else 'ascii'} 1.0\nelement vertex {N}\n"
              f"property float x\nproperty float y\nproperty float z\n{header_color}end_header\n").encode()

    record = np.zeros((N,), dtype=dtype)
    record['xyz'] = points.astype(np.float32)
    if color is not None and color.ndim == 1: record['i']   = color.astype(np.uint8)
    if color is not None and color.ndim == 2: record['rgb'] = color[:, ::-1].astype(np.uint8)
    with open(filename, 'wb') as f:
        f.write(header)
        if binary:
            record.tofile(f)
        else:
            for r in record:
                fields = ["%.9g" % x for x in r['xyz']]
                if color is not None:
                    fields += ["%d" % c for c in np.atleast_1d(r['i'] if color.ndim == 1 else r['rgb'])]
                f.write((" ".join(fields) + "\n").encode())


def mapping_file_framenocameraindex(*files_per_camera):
    """Image filenames to frame numbers: a dict from filename to (framenumber, cameraindex)

    mapping_file_framenocameraindex(('img5-cam2.jpg', 'img6-cam2.jpg'), ('img6-cam3.jpg', 'img7-cam3.jpg'))
    -> {'img5-cam2.jpg': (5, 0), 'img6-cam2.jpg': (6, 0), 'img6-cam3.jpg': (6, 1), 'img7-cam3.jpg': (7, 1)}

One argument a camera: the filenames of its images; cameraindex counts the arguments. Within a camera the longest
leading and trailing strings common to all its filenames are removed; what varies in between, which must be numeric,
and the digits next to it are the frame number, which is neither sequential nor starts at 0. A camera with ONE image
gets frame number 0. A middle that is not numeric is an error with several cameras, and sequential numbers with one.
Host code. Reference: mrcal.mapping_file_framenocameraindex() (mrcal/utils.py)"""
    import re
    empty = [i for i in range(len(files_per_camera)) if len(files_per_camera[i]) == 0]
    if len(empty) > 0:
        raise Exception("These camera globs matched no files: {}".format(empty))

    def common(a, b, from_the_end):
        if from_the_end: a, b = a[::-1], b[::-1]
        n = 0
        while n < len(a) and n < len(b) and a[n] == b[n]: n += 1
        return a[:n][::-1] if from_the_end else a[:n]

    def framenumbers(files):
        if len(files) == 1:
            return [0]
        leading = trailing = files[0]
        for f in files[1:]:
            leading, trailing = common(leading, f, False), common(trailing, f, True)
        end = -len(trailing) if len(trailing) > 0 else None
        for f in files:
            if not re.match("^[0-9]+$", f[len(leading):end]):
                raise Exception(("Image filenames MUST be of the form 'something..number..something'\n" +
                                 "where the somethings are common to all the filenames. File '{}'\n" +
                                 "has a non-numeric middle: '{}'. The somethings are: '{}' and '{}'\n" +
                                 "Did you forget to pass globs for each camera separately?").format(f, f[len(leading):end], leading, trailing))
        before = re.match("^(.*?)([0-9]*)$", leading).group(2)
        after  = re.match("^([0-9]*)(.*?)$", trailing).group(1)
        return [int(before + f[len(leading):end] + after) for f in files]

    mapping = {}
    for icamera, files in enumerate(files_per_camera):
        try:
            numbers = framenumbers(files)
        except Exception:
            if len(files_per_camera) != 1: raise
            numbers = range(len(files))
        mapping.update(zip(files, [(n, icamera) for n in numbers]))
    return mapping


def hypothesis_board_corner_positions(icam_intrinsics=None, idx_inliers=None, **optimization_inputs):
    """The 3D chessboard corners a solve's state puts in front of its cameras, in each observing camera's coordinates:
    the board's geometry (with its warp) through rt_ref_frame and rt_cam_ref as
    indices_frame_camintrinsics_camextrinsics pairs them. Returns four arrays:
      (Nobservations,Nheight,Nwidth,3)  all observations
      (Nobservations of camera icam_intrinsics,Nheight,Nwidth,3)   (icam_intrinsics None: the same as the first)
      (N,3) the inliers among the second, (N,3) the outliers
    idx_inliers (Nobservations,Nheight,Nwidth) booleans: which corners count as inliers, instead of weight > 0 (to pick
    the inliers common to two solves). Host code. Reference: mrcal.hypothesis_board_corner_positions()"""
    from .calibration import ref_calibration_object
    from .poseutils import Rt_from_rt, compose_Rt, identity_Rt, transform_point_Rt
    observations_board = optimization_inputs.get('observations_board')
    if observations_board is None:
        raise Exception("No board observations available")
    observations_board = np.asarray(observations_board)
    ifce = np.asarray(optimization_inputs['indices_frame_camintrinsics_camextrinsics'])
    Nh, Nw = observations_board.shape[-3:-1]
    # (Nh,Nw,3)
    full_object = ref_calibration_object(Nw, Nh, optimization_inputs['calibration_object_spacing'],
                                         calobject_warp=optimization_inputs.get('calobject_warp'))
    Rt_ref_frame = Rt_from_rt(optimization_inputs['rt_ref_frame'])[ifce[:, 0]]
    rt_cam_ref = optimization_inputs.get('rt_cam_ref')
    rt_cam_ref = np.zeros((0, 6)) if rt_cam_ref is None else np.asarray(rt_cam_ref, dtype=float).reshape(-1, 6)
    Rt_cam_ref = np.concatenate((identity_Rt()[None], Rt_from_rt(rt_cam_ref)), axis=0)[ifce[:, 2] + 1]
    Rt_cam_frame = compose_Rt(Rt_cam_ref, Rt_ref_frame)
    p_cam = transform_point_Rt(Rt_cam_frame[:, None, None, :, :], full_object)
    if idx_inliers is None:
        idx_inliers = observations_board[..., 2] > 0
    idx_inliers  = np.array(idx_inliers, dtype=bool)
    idx_outliers = ~idx_inliers
    if icam_intrinsics is None:
        return p_cam, p_cam, p_cam[idx_inliers], p_cam[idx_outliers]
    idx_observations = ifce[:, 1] == icam_intrinsics
    idx_inliers [~idx_observations] = False
    idx_outliers[~idx_observations] = False
    return p_cam, p_cam[idx_observations], p_cam[idx_inliers], p_cam[idx_outliers]


def _all_measurements(optimization_inputs):
    from . import optimizer_callback
    return optimizer_callback(**optimization_inputs, no_jacobian=True, no_factorization=True)[1]


def measurements_board(optimization_inputs, *, icam_intrinsics=None, x=None, return_observations=False, i_cam=None):
    """The board measurements of a solve, (N,2): the WEIGHTED reprojection errors of every board corner that is not an
    outlier (weight > 0), of all cameras or of camera icam_intrinsics; x: the measurement vector if it is at hand,
    else optimizer_callback() evaluates it. return_observations: also the pixels (N,2) they were observed at. No board
    observations: (0,2) arrays. i_cam: the older name of icam_intrinsics. A numpy selection on the host.
    Reference: mrcal.measurements_board()"""
    from . import measurement_index_boards, num_measurements_boards
    observations_board = optimization_inputs.get('observations_board')
    if observations_board is None or np.size(observations_board) == 0:
        empty = np.zeros((0, 2), dtype=float)
        return (empty, np.zeros((0, 2), dtype=float)) if return_observations else empty
    observations_board = np.asarray(observations_board)
    if i_cam is not None:
        icam_intrinsics = i_cam
    if x is None:
        x = _all_measurements(optimization_inputs)
    imeas0 = measurement_index_boards(0, **optimization_inputs)
    Nmeas  = num_measurements_boards(**optimization_inputs)
    x_board = np.asarray(x)[imeas0:imeas0 + Nmeas].reshape(observations_board.shape[:-1] + (2,))
    keep = observations_board[..., 2] > 0.0
    if icam_intrinsics is not None:
        camera = np.asarray(optimization_inputs['indices_frame_camintrinsics_camextrinsics'])[:, 1]
        keep[camera != icam_intrinsics, ...] = False
    if return_observations:
        return x_board[keep], observations_board[keep][..., :2]
    return x_board[keep]


def residuals_board(*args, residuals=None, **kwargs):
    """measurements_board() under its older name, with x called residuals"""
    return measurements_board(*args, x=residuals, **kwargs)


def measurements_point(optimization_inputs, *, icam_intrinsics=None, x=None, return_observations=False):
    """The measurements of the discrete point observations of a solve, (N,2): the weighted reprojection errors of every
    point observation that is not an outlier, of all cameras or of camera icam_intrinsics. Otherwise as
    measurements_board(). Reference: mrcal.measurements_point()"""
    from . import measurement_index_points, num_measurements_points
    observations_point = optimization_inputs.get('observations_point')
    if observations_point is None or np.size(observations_point) == 0:
        empty = np.zeros((0, 2), dtype=float)
        return (empty, np.zeros((0, 2), dtype=float)) if return_observations else empty
    observations_point = np.asarray(observations_point)
    if x is None:
        x = _all_measurements(optimization_inputs)
    Nobservations = len(observations_point)
    imeas0 = measurement_index_points(0, **optimization_inputs)
    Nmeas  = num_measurements_points(**optimization_inputs)
    # (the reprojection error is the first two measurements of an observation)
    x_point = np.asarray(x)[imeas0:imeas0 + Nmeas].reshape(Nobservations, -1)[:, :2]
    keep = observations_point[..., 2] > 0.0
    if icam_intrinsics is not None:
        camera = np.asarray(optimization_inputs['indices_point_camintrinsics_camextrinsics'])[:, 1]
        keep[camera != icam_intrinsics] = False
    if return_observations:
        return x_point[keep], observations_point[keep][..., :2]
    return x_point[keep]


def residuals_point(*args, residuals=None, **kwargs):
    """measurements_point() under its older name, with x called residuals"""
    return measurements_point(*args, x=residuals, **kwargs)
