"""find_chessboard_corners(): the calibration board detected on the GPU (csrc/chessboard.hip; the definition:
include/mrcal_amd.h, "chessboard corners"), chessboard_corner_candidates(), ChessboardDetector, chessboard_grid() and
compute_chessboard_corners().

The checker (chessboard_checker.py) restates parts a-d of the definition in numpy. The response image and the candidates
are held to it pixel for pixel, with no tolerance; the refined positions to 1e-4 px (the two sum in different orders and
may stop an iteration apart, and a last step is below 1e-5 px by the stop rule). The checker itself is held to the
analytic corners of rendered boards.

What was measured, and is asserted below:
  the checker on the five pure-numpy renders of this file (800 x 600, 10 x 7 corners, squares of 14-40 px, rotation,
  perspective, k1 down to -0.5, noise of 1-3 grey levels): all 70 corners and no other candidate in every one; the worst
  error over the five 0.1042 px, the rms 0.0416 px
  the rms residual of tests/golden/real_opencv8-0.cameramodel at its stored optimum, from optimizer_callback() on the
  GPU, over the 18597 of 18600 corners that are not outliers: 0.551 px over the x and y residuals (0.780 px over the
  corners' residual vectors), as the solver weighs them. The smaller figure is the one used
  the checker with the board's lines along the pixel grid: test_checker_near_the_pixel_grid"""
import functools
import io
import os

import numpy as np
import pytest

import hostbuild
import chessboard_checker as chk

# measured once (the docstring above); the assertions use them as written here
RECORDED_WORST = 0.1042         # px: the checker's worst corner over the five renders
RECORDED_RMS   = 0.0416         # px: ... and its rms
REAL_DATA_RMS  = 0.551          # px: rms residual of real_opencv8-0.cameramodel at its stored optimum
BOUND = 2*RECORDED_WORST        # what is asserted: the rounding of the grey levels moves the worst corner from seed to seed

CONFIGS = (dict(square=30., angle=0.,   perspective=(0., 0.),      k1=0.,   noise=1., seed=1),
           dict(square=40., angle=25.,  perspective=(1e-4, -5e-5), k1=0.,   noise=2., seed=2),
           dict(square=14., angle=-40., perspective=(0., 0.),      k1=-0.5, noise=3., seed=3, centre=(250., 200.)),
           dict(square=24., angle=190., perspective=(4e-4, 2e-4),  k1=-0.3, noise=2., seed=4),
           dict(square=36., angle=40.,  perspective=(-2e-4, 3e-4), k1=-0.5, noise=3., seed=5))


# ------------------------------------------------------------------------------------------------ without a GPU ---
def test_host_code_under_the_host_sanitizers():
    """csrc/chessboard_plan.hpp and csrc/chessboard_grid.cpp driven by a stand-alone program with its own main, built
    with ASan and UBSan"""
    hostbuild.assert_prints_ok("chessboard_grid_check")


def board_points(W, H, step, degrees, perspective, k1, jitter, rng):
    """(H,W,2): the corners of a board in an 800 x 600 image, in the board's own labelling: turned about the image's
    centre, a perspective division, radial distortion (focal length 800), uniform jitter"""
    c, s = np.cos(np.radians(degrees)), np.sin(np.radians(degrees))
    u, v = np.meshgrid((np.arange(W) - (W - 1)/2.)*step, (np.arange(H) - (H - 1)/2.)*step)
    x, y = c*u - s*v, s*u + c*v
    w = 1. + perspective[0]*x + perspective[1]*y
    x, y = x/w, y/w
    r2 = (x*x + y*y)/800.**2
    p = np.stack((399.5 + x*(1. + k1*r2), 299.5 + y*(1. + k1*r2)), axis=-1)
    return p + rng.uniform(-jitter, jitter, p.shape)


def expected_labelling(native):
    """part e of the definition, by trying all eight labellings of the native one"""
    H, W = native.shape[:2]
    best = None
    for transposed in (False, True):
        a = native.transpose(1, 0, 2) if transposed else native
        for b in (a, a[::-1], a[:, ::-1], a[::-1, ::-1]):
            if b.shape[:2] != (H, W): continue
            ei, ej = (b[:, 1:] - b[:, :-1]).sum((0, 1)), (b[1:] - b[:-1]).sum((0, 1))
            if not ei[0]*ej[1] - ei[1]*ej[0] > 0: continue
            x = ei[0]/np.linalg.norm(ei)
            if best is None or x > best[0]: best = (x, b)
    return best[1]


def clutter_around(native, step, n, rng):
    """n points anywhere in the image, but not within half a step of a corner, where they would BE the corner"""
    out = []
    while len(out) < n:
        p = rng.uniform((0., 0.), (800., 600.))
        if np.linalg.norm(native.reshape(-1, 2) - p, axis=-1).min() >= 0.5*step: out.append(p)
    return np.array(out)


@pytest.mark.parametrize("degrees", (0., 40., -40., 180.))
@pytest.mark.parametrize("board", ((10, 10), (10, 7), (4, 3)), ids=lambda b: f"{b[0]}x{b[1]}")
def test_grid_finder_through_the_c_abi(amd, board, degrees):
    W, H = board
    rng = np.random.default_rng(int(1000 + degrees) + 7*W + H)
    for step, perspective, k1 in ((31., (0., 0.), 0.), (38., (3e-4, -2e-4), 0.), (26., (3e-4, -2e-4), -0.5)):
        native = board_points(W, H, step, degrees, perspective, k1, 0.1, rng)
        expected = expected_labelling(native)
        if W != H:      # (the two rules agree: this is the native labelling, or the one turned by 180 degrees)
            assert np.array_equal(expected, native[::-1, ::-1] if degrees == 180. else native)
        clutter = clutter_around(native, step, 30, rng)
        q = np.concatenate((native.reshape(-1, 2), clutter))
        order = rng.permutation(len(q))
        for points in (q, q[order]):
            found = amd.chessboard_grid(points, W, H)
            assert found is not None and found.shape == (H, W, 2) and np.array_equal(found, expected)
        # the response orders the seeds and changes nothing else; a status that is not 0 takes a point out
        response = rng.integers(1, 1000, size=len(q))
        assert np.array_equal(amd.chessboard_grid(q, W, H, response=response, status=np.zeros(len(q))), expected)
        status = np.zeros(len(q)); status[W + 1] = 2
        assert amd.chessboard_grid(q, W, H, response=response, status=status) is None
        # one corner removed: at a corner of the board, on its rim, inside
        for gone in (0, W*H - 1, W//2, (H//2)*W + W//2):
            assert amd.chessboard_grid(np.delete(q, gone, axis=0), W, H) is None
        # a corner duplicated 0.4 of a step away is not taken
        for which in (0, (H//2)*W + W//2):
            for sign in (1., -1.):
                double = q[which] + sign*0.4*(q[which + 1] - q[which])
                found = amd.chessboard_grid(np.concatenate((double[None], q)), W, H)
                assert found is not None and np.array_equal(found, expected)
        # only clutter; another board
        assert amd.chessboard_grid(clutter, W, H) is None
        assert amd.chessboard_grid(q, W + 1, H) is None
        if W != H:
            found = amd.chessboard_grid(q, H, W)        # the other way round: the same corners, +i along the other side
            assert found is not None and np.array_equal(found, expected_labelling(native.transpose(1, 0, 2)))


@functools.lru_cache(maxsize=None)
def render(k):
    """pure-numpy render k of the five, its true corners, and what the checker makes of it; made once"""
    image, truth = chk.render_numpy(10, 7, **CONFIGS[k])
    return (image, truth) + chk.detect(image)


def test_checker_against_truth(amd):
    """every corner found, no other candidate, the positions within twice the recorded worst error of the analytic
    corners; and the lattice finder puts them in the order of the truth"""
    worst, squares = 0., []
    for k, config in enumerate(CONFIGS):
        image, truth, q, response, status, overflow, R = render(k)
        assert len(q) == 70 and not overflow and np.all(status == chk.STATUS_OK), config
        d = np.linalg.norm(q[:, None] - truth.reshape(-1, 2)[None], axis=-1)
        assert np.array_equal(np.sort(d.argmin(1)), np.arange(70)), config          # (a corner each)
        error = d.min(1)
        print(f"square {config['square']:g} angle {config['angle']:g} k1 {config['k1']:g}: worst {error.max():.4f} rms {np.sqrt((error**2).mean()):.4f} px")
        worst = max(worst, error.max()); squares.append(error**2)
        board = amd.chessboard_grid(q, 10, 7, response=response, status=status)
        expected = truth[::-1, ::-1] if config["angle"] == 190. else truth
        assert board is not None and np.abs(board - expected).max() <= BOUND, config
    rms = np.sqrt(np.concatenate(squares).mean())
    print(f"all five: worst {worst:.4f} rms {rms:.4f} px")
    assert worst <= BOUND
    assert abs(worst - RECORDED_WORST) < 1e-3 and abs(rms - RECORDED_RMS) < 1e-3       # (what is recorded is what is)
    # a detector noisier than the data the project already calibrates from is not good enough
    assert RECORDED_WORST < REAL_DATA_RMS


def test_checker_near_the_pixel_grid():
    """What the five renders do not show: with the board's lines along the pixel grid, or within a few degrees of it,
    and no blur in the image, the refinement of part d is off by up to 0.3 px, whatever the size of the squares. The
    sums of part d weigh a point by its SQUARED gradient; across a line one pixel wide that lies along a pixel column
    the squared gradient's centroid is pulled towards the pixel that holds more of the step, by an amount that depends
    on where in the pixel the line is. Turned by 10 degrees or more the phases average out along the window (the
    renders above). cv2.cornerSubPix has the same property; a lens's blur, which these renders lack, reduces it.
    Measured (400 x 300, 10 x 7 corners, no noise; printed below): squares of 28.3 px at 0, 0.6 and 3 degrees: worst
    0.217, 0.290, 0.147 px, rms 0.137, 0.135, 0.093; squares of 40.3 px at 1 degree: worst 0.225, rms 0.143.
    Asserted: every corner is found and the worst stays below the rms residual of the real data the project calibrates
    from, the issue's measure of a detector that is good enough; the recorded bound of the rotated boards is NOT met"""
    for square, angle in ((28.3, 0.), (28.3, 0.6), (28.3, 3.), (40.3, 1.)):
        image, truth = chk.render_numpy(10, 7, width=520 if square > 40 else 400, height=400 if square > 40 else 300, square=square, angle=angle)
        q, _, status, _, _ = chk.detect(image)
        assert len(q) == 70 and np.all(status == chk.STATUS_OK)
        d = np.linalg.norm(q[:, None] - truth.reshape(-1, 2)[None], axis=-1)
        assert np.array_equal(np.sort(d.argmin(1)), np.arange(70))
        error = d.min(1)
        print(f"square {square:g} angle {angle:g}: worst {error.max():.4f} rms {np.sqrt((error**2).mean()):.4f} px")
        assert error.max() < REAL_DATA_RMS


def test_mapping_file_framenocameraindex(amd):
    f = amd.mapping_file_framenocameraindex
    assert f(('img5-cam2.jpg', 'img6-cam2.jpg'), ('img6-cam3.jpg', 'img7-cam3.jpg')) == \
        {'img5-cam2.jpg': (5, 0), 'img6-cam2.jpg': (6, 0), 'img6-cam3.jpg': (6, 1), 'img7-cam3.jpg': (7, 1)}
    assert f(('a/frame009.png', 'a/frame010.png', 'a/frame011.png')) == {'a/frame009.png': (9, 0), 'a/frame010.png': (10, 0), 'a/frame011.png': (11, 0)}
    assert f(('only.png',), ('x1.png', 'x2.png')) == {'only.png': (0, 0), 'x1.png': (1, 1), 'x2.png': (2, 1)}
    assert f(('left.png', 'right.png')) == {'left.png': (0, 0), 'right.png': (1, 0)}       # (one camera: in sequence)
    with pytest.raises(Exception, match="has a non-numeric middle: 'lef'"):
        f(('left.png', 'right.png'), ('x1.png', 'x2.png'))
    with pytest.raises(Exception, match="^These camera globs matched no files: \\[1\\]$"):
        f(('x1.png',), ())


def vnl_of(boards, columns=4):
    """the corners file of {filename: rows of (x, y, level) or None}"""
    lines = ["# filename x y level\n" if columns == 4 else "# filename x y\n"]
    for name, rows in boards.items():
        if rows is None:
            lines.append(f"{name} - - -\n" if columns == 4 else f"{name} - -\n")
            continue
        for row in rows:
            lines.append(" ".join([name] + [str(x) for x in row[:columns - 1]]) + "\n")
    return "".join(lines)


def test_compute_chessboard_corners_reads_a_cache(amd, tmp_path, monkeypatch):
    """the corner-cache reading of the reference; a 3 x 3 board, the expected arrays written out by hand"""
    f = amd.compute_chessboard_corners
    def no_device(*a, **k): raise AssertionError("a cache is read without the detector")
    monkeypatch.setattr(amd.chessboard, "ChessboardDetector", no_device)
    grid = [(10*i + 1.5, 10*j + 2.25) for j in range(3) for i in range(3)]
    def rows(levels): return [(x, y, l) for (x, y), l in zip(grid, levels)]
    boards = {"frame5-cam0.pgm": rows([0, 1, 2, 0, 0, 0, 0, 0, 0]),
              "frame6-cam0.pgm": None,
              "frame7-cam0.pgm": rows([0, 0, 0, 0, "-", 0, 0, -1, 0]),
              "frame5-cam1.pgm": rows([0]*9),
              "frame7-cam1.pgm": rows([0]*9),
              "notes.txt":       rows([0]*9)}                   # (matches no glob: silently ignored)
    globs = ("frame*-cam0.pgm", "frame*-cam1.pgm")
    xy = np.array(grid).reshape(3, 3, 2)
    def board(weights): return np.concatenate((xy, np.array(weights, dtype=float).reshape(3, 3, 1)), axis=-1)

    # 4 columns, levels: two cameras, frames 5 and 7 become 0 and 1
    obs, idx, paths = f(3, 3, globs_per_camera=globs, corners_cache_vnl=io.StringIO(vnl_of(boards)))
    assert paths == ["frame5-cam0.pgm", "frame5-cam1.pgm", "frame7-cam0.pgm", "frame7-cam1.pgm"]
    assert idx.dtype == np.int32 and np.array_equal(idx, ((0, 0), (0, 1), (1, 0), (1, 1)))
    assert obs.shape == (4, 3, 3, 3)
    assert np.array_equal(obs[0], board([1, 0.5, 0.25, 1, 1, 1, 1, 1, 1]))
    assert np.array_equal(obs[1], board([1]*9)) and np.array_equal(obs[3], board([1]*9))
    assert np.array_equal(obs[2], board([1, 1, 1, 1, -1, 1, 1, -1, 1]))        # (x and y are read; the weight says "ignore")

    # the column as a weight: copied; <= 0 and '-' are "ignore"
    weights = {"frame5-cam0.pgm": rows([0.5, 2, 1, 1, 1, 1, 1, 0, 1]), "frame6-cam0.pgm": rows([1]*9)}
    obs, idx, paths = f(3, 3, globs_per_camera=globs[:1], corners_cache_vnl=io.StringIO(vnl_of(weights)), weight_column_kind='weight')
    assert np.array_equal(obs[0][..., 2].ravel(), (0.5, 2, 1, 1, 1, 1, 1, -1, 1)) and np.array_equal(idx, ((0, 0), (1, 0)))
    # no kind: the column is not read, the weight is 1
    obs, _, _ = f(3, 3, globs_per_camera=globs[:1], corners_cache_vnl=io.StringIO(vnl_of(weights)), weight_column_kind=None)
    assert np.array_equal(obs[0][..., 2].ravel(), [1]*9)
    # 3 columns: weight 1; a '-' row is a point that was not seen
    three = {"frame5-cam0.pgm": rows([0]*9), "frame6-cam0.pgm": rows([0]*9)[:4] + [("-", "-", 0)] + rows([0]*9)[5:]}
    obs, idx, paths = f(3, 3, globs_per_camera=globs[:1], corners_cache_vnl=io.StringIO(vnl_of(three, columns=3)))
    assert np.array_equal(obs[0], board([1]*9)) and np.array_equal(obs[1][1, 1], (-1, -1, -1)) and np.array_equal(obs[1][..., 2].ravel(), (1, 1, 1, 1, -1, 1, 1, 1, 1))
    with pytest.raises(Exception, match="^weight_column_kind must be one of \\('level','weight',None\\); got 'levels'$"):
        f(3, 3, corners_cache_vnl=io.StringIO(""), weight_column_kind='levels')

    # exclude_images; Npoint_observations_per_board_min (more than that many valid points are needed: default 2 min(W,H) = 6)
    obs, idx, paths = f(3, 3, globs_per_camera=globs[:1], corners_cache_vnl=io.StringIO(vnl_of(boards)), exclude_images={"frame5-cam0.pgm"})
    assert paths == ["frame7-cam0.pgm"] and np.array_equal(idx, ((0, 0),))
    obs, idx, paths = f(3, 3, globs_per_camera=globs[:1], corners_cache_vnl=io.StringIO(vnl_of(boards)), Npoint_observations_per_board_min=7)
    assert paths == ["frame5-cam0.pgm"]                        # (frame 7 has exactly 7 valid points: not MORE than 7)

    # the path rules: a prefix; a directory in place of the paths' own; as they are, normalised
    deep = {"./data//frame5-cam0.pgm": rows([0]*9), "data/frame6-cam0.pgm": rows([0]*9)}
    _, _, paths = f(3, 3, globs_per_camera=("frame*-cam0.pgm",), corners_cache_vnl=io.StringIO(vnl_of(deep)), image_path_prefix="/mnt/images")
    assert paths == ["/mnt/images/./data//frame5-cam0.pgm", "/mnt/images/data/frame6-cam0.pgm"]
    _, _, paths = f(3, 3, globs_per_camera=("frame*-cam0.pgm",), corners_cache_vnl=io.StringIO(vnl_of(deep)), image_directory="/elsewhere")
    assert paths == ["/elsewhere/frame5-cam0.pgm", "/elsewhere/frame6-cam0.pgm"]
    _, _, paths = f(3, 3, globs_per_camera=("frame*-cam0.pgm",), corners_cache_vnl=io.StringIO(vnl_of(deep)))
    assert paths == ["data/frame5-cam0.pgm", "data/frame6-cam0.pgm"]
    # ... and a file on disk: a relative path that does not exist from here is relative to the file's directory
    (tmp_path / "there").mkdir()
    cache = tmp_path / "there" / "corners.vnl"
    cache.write_text(vnl_of({"frame5-cam0.pgm": rows([0]*9), "/abs/frame6-cam0.pgm": rows([0]*9)}))
    _, _, paths = f(3, 3, globs_per_camera=("frame*-cam0.pgm",), corners_cache_vnl=str(cache))
    assert paths == [f"{tmp_path}/there/frame5-cam0.pgm", "/abs/frame6-cam0.pgm"]
    monkeypatch.chdir(tmp_path / "there")
    (tmp_path / "there" / "frame5-cam0.pgm").write_text("")     # (it exists from here now: as it is)
    _, _, paths = f(3, 3, globs_per_camera=("frame*-cam0.pgm",), corners_cache_vnl=str(cache))
    assert paths == ["frame5-cam0.pgm", "/abs/frame6-cam0.pgm"]
    with pytest.raises(Exception, match="is a directory. Must be a file or must not exist"):
        f(3, 3, corners_cache_vnl=str(tmp_path / "there"))

    # what is refused
    short = dict(boards); short["frame5-cam0.pgm"] = rows([0]*9)[:8]
    with pytest.raises(Exception, match="^File 'frame5-cam0.pgm' expected to have 9 points, but got 8$"):
        f(3, 3, globs_per_camera=globs, corners_cache_vnl=io.StringIO(vnl_of(short)))
    long = {"frame5-cam0.pgm": rows([0]*9) + rows([0])}
    with pytest.raises(Exception, match="^File 'frame5-cam0.pgm' expected to have 9 points, but got 10$"):
        f(3, 3, globs_per_camera=globs[:1], corners_cache_vnl=io.StringIO(vnl_of(long)))
    with pytest.raises(Exception, match="^Found too few \\(1; need at least 2\\) images containing a calibration pattern in camera 1; glob '\\*/frame\\*-cam1.pgm'$"):
        f(3, 3, globs_per_camera=globs, corners_cache_vnl=io.StringIO(vnl_of(boards)), exclude_images={"frame5-cam1.pgm"})
    with pytest.raises(Exception, match="^Found too few \\(0; need at least 1\\)"):
        f(3, 3, globs_per_camera=("nothing*.pgm",), corners_cache_vnl=io.StringIO(vnl_of(boards)))
    with pytest.raises(Exception, match="data rows must contain a filename and 2 or 3 values"):
        f(3, 3, corners_cache_vnl=io.StringIO("a.pgm 1 2 3 4\n"))
    with pytest.raises(Exception, match="with x and y being numerical or '-'"):
        f(3, 3, corners_cache_vnl=io.StringIO("a.pgm 1 two 0\n"))
    with pytest.raises(Exception, match="expected as 'filename x y level' with level being numerical or '-'"):
        f(3, 3, corners_cache_vnl=io.StringIO("a.pgm 1 2 high\n"))
    # jobs < 0: the cache MUST be there
    for cache in (None, str(tmp_path / "no-such.vnl")):
        with pytest.raises(Exception, match="^I was asked to use an existing cache file, but it couldn't be read. jobs<0, so I do not recompute$"):
            f(3, 3, globs_per_camera=globs, corners_cache_vnl=cache, jobs=-1)
    assert not (tmp_path / "no-such.vnl").exists()
    with pytest.raises(Exception, match="weight_column_kind == 'weight'"):
        f(3, 3, globs_per_camera=globs, corners_cache_vnl=str(tmp_path / "no-such.vnl"), weight_column_kind='weight')


def write_pgm(path, image):
    maxval = 255 if image.dtype == np.uint8 else 65535
    with open(path, "wb") as f:
        f.write(f"P5\n# a comment\n{image.shape[1]} {image.shape[0]}\n{maxval}\n".encode())
        f.write(image.astype(image.dtype.newbyteorder(">")).tobytes())


def test_images_are_read(amd, tmp_path):
    rng = np.random.default_rng(0)
    for dtype in (np.uint8, np.uint16):
        image = rng.integers(0, np.iinfo(dtype).max + 1, size=(33, 47)).astype(dtype)
        image[0, :4] = (10, 32, 9, 13)                          # (whitespace bytes right after the header)
        write_pgm(tmp_path / "a.pgm", image)
        back = amd.load_image_gray(str(tmp_path / "a.pgm"))
        assert back.dtype == dtype and back.flags.c_contiguous and np.array_equal(back, image)
    (tmp_path / "cut.pgm").write_bytes(b"P5\n47 33\n255\n" + bytes(100))
    with pytest.raises(Exception, match="^Couldn't load image '.*cut.pgm': 100 bytes of pixels, 1551 expected$"):
        amd.load_image_gray(str(tmp_path / "cut.pgm"))
    (tmp_path / "not-an-image.png").write_bytes(b"no image at all")
    with pytest.raises(Exception, match="not-an-image.png"):
        amd.load_image_gray(str(tmp_path / "not-an-image.png"))


def test_refusals_before_any_device_work(amd, monkeypatch):
    def no_device(*a, **k): raise AssertionError("device work before the refusal")
    monkeypatch.setattr(amd._handle, "_libs", no_device)
    u8 = np.zeros((48, 64), dtype=np.uint8)
    find, candidates, Detector = amd.find_chessboard_corners, amd.chessboard_corner_candidates, amd.ChessboardDetector
    for bad in (np.zeros((48, 64, 3), dtype=np.uint8), np.zeros((48,), dtype=np.uint8), [[0]*64]*48):
        with pytest.raises(Exception, match="^find_chessboard_corners\\(\\) accepts ONLY grayscale images of shape \\(H,W\\)"):
            find(bad, 10)
        with pytest.raises(Exception, match="^find_chessboard_corners\\(\\) accepts ONLY grayscale images of shape \\(H,W\\)"):
            candidates(bad)
    for bad in (np.float32, np.int16, np.uint32, bool):
        with pytest.raises(Exception, match=f"^find_chessboard_corners\\(\\): images must have dtype uint8 or uint16, not {np.dtype(bad)}$"):
            find(u8.astype(bad), 10)
        with pytest.raises(Exception, match="^find_chessboard_corners\\(\\): images must have dtype uint8 or uint16"):
            Detector((48, 64), bad)
    with pytest.raises(Exception, match="^find_chessboard_corners\\(\\): images must have dtype uint8 or uint16, not None$"):
        Detector((48, 64), "no dtype")
    with pytest.raises(Exception, match="^find_chessboard_corners\\(\\): an image of 64 x 31 pixels is too small: at least 32 x 32$"):
        find(u8[:31], 10)
    with pytest.raises(Exception, match="^find_chessboard_corners\\(\\): an image of 31 x 48 pixels is too small"):
        Detector((48, 31), np.uint16)
    # more than 2^28 pixels (a view: no memory behind it)
    huge = np.lib.stride_tricks.as_strided(np.zeros((1,), dtype=np.uint8), shape=(1 << 14, (1 << 14) + 1), strides=(0, 0))
    with pytest.raises(Exception, match="^find_chessboard_corners\\(\\): an image of 16385 x 16384 pixels is too large: at most 268435456 pixels$"):
        find(huge, 10)
    with pytest.raises(Exception, match="^find_chessboard_corners\\(\\) accepts ONLY grayscale images"):
        Detector((48, 64, 3))
    for kw, words in ((dict(threshold_256=256), "threshold_256 must be in 0..255, got 256"), (dict(threshold_256=-1), "threshold_256 must be in 0..255, got -1"),
                      (dict(threshold_256=51.), "threshold_256 must be in 0..255, got 51.0"),
                      (dict(nms_radius=0), "nms_radius must be in 1..16, got 0"), (dict(nms_radius=17), "nms_radius must be in 1..16, got 17"),
                      (dict(max_candidates=0), "max_candidates must be in 1..65536, got 0"), (dict(max_candidates=65537), "max_candidates must be in 1..65536, got 65537")):
        for call in (lambda: find(u8, 10, **kw), lambda: candidates(u8, **kw), lambda: Detector(u8.shape, u8.dtype, **kw)):
            with pytest.raises(Exception, match="^find_chessboard_corners\\(\\): " + words + "$"):
                call()
    for W, H in ((2, 7), (10, 257), (10., 7), (True, 7)):
        with pytest.raises(Exception, match="^find_chessboard_corners\\(\\): a board has 3..256 corners a side, got"):
            find(u8, W, H)
    # a detector is for one shape and dtype; a closed one says so (no device: the object is not initialised)
    d = Detector.__new__(Detector)
    d.handle, d.shape, d.dtype, d.max_candidates = 1, (48, 64), np.dtype(np.uint8), 4096
    with pytest.raises(Exception, match="^find_chessboard_corners\\(\\): this detector was made for images of shape \\(48, 64\\) and dtype uint8, got \\(48, 65\\) and uint8$"):
        d.find_board(np.zeros((48, 65), dtype=np.uint8), 10)
    with pytest.raises(Exception, match="this detector was made for images of shape \\(48, 64\\) and dtype uint8, got \\(48, 64\\) and uint16$"):
        d.candidates(u8.astype(np.uint16))
    with pytest.raises(Exception, match="a board has 3..256 corners a side"):
        d.find_board(u8, 1)
    d.handle = None
    for call in (lambda: d.candidates(u8), lambda: d.find_board(u8, 10), d.response, d.stage_milliseconds):
        with pytest.raises(Exception, match="^this ChessboardDetector has been closed$"):
            call()


# --------------------------------------------------------------------------------------------------- on the GPU ---
def corner_image(cx, cy, width=48, height=40):
    """ONE corner, at (cx,cy): the middle of a board of 2 x 2 squares of 20 pixels, no noise"""
    return chk.render_numpy(1, 1, width=width, height=height, square=20., centre=(cx, cy))[0]


def gpu_cases():
    """name -> (uint8 image, detector keywords): the smallest images at which the kernels can still go wrong"""
    rng = np.random.default_rng(11)
    cases = {}
    # the smallest image: R is defined on 20 x 20 pixels of it (corners 8 px apart: a window of 11)
    cases["32x32"] = (chk.render_numpy(3, 3, width=32, height=32, square=8., angle=3., noise=1., seed=1)[0], dict(nms_radius=5))
    # narrower than one tile; neither a multiple of the tile nor of 4: several tiles, the last ones partly outside
    cases["45x39"] = (chk.render_numpy(3, 3, width=45, height=39, square=9., angle=-20., noise=2., seed=2)[0], {})
    cases["131x97"] = (chk.render_numpy(5, 4, width=131, height=97, square=16., angle=30., perspective=(5e-4, 0.), noise=2., seed=3)[0], {})
    # noise: candidates everywhere, at every place of a mask word and of a chunk, many to a tile
    cases["131x97 noise"] = (rng.integers(0, 256, size=(97, 131)).astype(np.uint8), dict(nms_radius=2, threshold_256=13))
    # 5 x 4 corners of 14-px squares: a column of corners at x = 63.5 and a row at y = 31.5, on the seams of the tiles
    # (x = 64 k, y = 16 k): its neighbours lie on either side
    cases["seam"] = (chk.render_numpy(5, 4, width=150, height=80, square=14., centre=(63.5 + 14., 31.5 + 7.), noise=1., seed=4)[0], {})
    # the first column that has a response, and the last that has none
    cases["corner at x=6"] = (corner_image(6., 20.), {})
    cases["corner at x=5"] = (corner_image(5., 20.), {})
    cases["corner at y=6, x=W-7"] = (corner_image(41., 6.), {})
    cases["constant"] = (np.full((40, 70), 131, dtype=np.uint8), {})
    # a corner half-way between two pixels: two (four) equal maxima inside one window
    cases["tie along x"] = (corner_image(24.5, 20.), {})
    cases["tie along y"] = (corner_image(24., 20.5), {})
    cases["tie of four"] = (corner_image(24.5, 20.5), {})
    cases["other radius"] = (cases["131x97"][0], dict(nms_radius=16, threshold_256=0))
    cases["max_candidates=8"] = (cases["131x97"][0], dict(max_candidates=8))
    return cases


GPU_CASES = gpu_cases()
STRUCTURED = [name for name in GPU_CASES if "noise" not in name]


def as_dtype(image, dtype):
    return image if dtype == np.uint8 else image.astype(np.uint16)*257


@pytest.fixture(scope="module")
def expected():
    """the checker's view of every case, computed once: (dtype name, case) -> (q, response, status, overflow, R, xy)"""
    out = {}
    for name, (image, kw) in GPU_CASES.items():
        for dtype in (np.uint8, np.uint16):
            im = as_dtype(image, dtype)
            R = chk.response(im)
            xy, overflow = chk.candidates(R, **kw)
            q, status, _ = chk.refine(im, xy)
            out[np.dtype(dtype).name, name] = (q, R[xy[:, 1], xy[:, 0]], status, overflow, R, xy)
    return out


def test_the_cases_are_about_something(expected):
    """(no GPU) each case has the property it is there for"""
    for dtype in ("uint8", "uint16"):
        def xy(name): return expected[dtype, name][5]
        def R(name): return expected[dtype, name][4]
        assert len(xy("32x32")) == 9 and len(xy("45x39")) == 9 and len(xy("131x97")) == 20 and len(xy("seam")) == 20
        assert len(xy("131x97 noise")) > 100 and len(set(expected[dtype, "131x97 noise"][2])) >= 1
        seam = xy("seam")
        assert {63, 64} & set(seam[:, 0]) and set(seam[:, 0]) & set(range(45, 63)) and set(seam[:, 0]) & set(range(65, 80))
        assert {31, 32} & set(seam[:, 1]) and set(seam[:, 1]) & set(range(16, 31)) and set(seam[:, 1]) & set(range(33, 48))
        # (x = 5 has no response: what is found of that corner is found a pixel beside it, and refined from there)
        assert np.array_equal(xy("corner at x=6"), ((6, 20),)) and np.array_equal(xy("corner at x=5"), ((6, 20),))
        assert np.all(R("corner at x=5")[:, :6] == 0) and R("corner at x=6")[20, 6] > R("corner at x=5")[20, 6] > 0
        assert np.array_equal(xy("corner at y=6, x=W-7"), ((41, 6),))
        assert len(xy("constant")) == 0 and R("constant").max() == 0
        r = R("tie along x"); assert r[20, 24] == r[20, 25] == r.max() and np.array_equal(xy("tie along x"), ((24, 20),))
        r = R("tie along y"); assert r[20, 24] == r[21, 24] == r.max() and np.array_equal(xy("tie along y"), ((24, 20),))
        r = R("tie of four"); assert r[20, 24] == r[20, 25] == r[21, 24] == r[21, 25] == r.max() and np.array_equal(xy("tie of four"), ((24, 20),))
        assert 1 <= len(xy("other radius")) < 20 and set(expected[dtype, "other radius"][2]) == {chk.STATUS_OK, chk.STATUS_LEFT}
        assert len(xy("max_candidates=8")) == 8 and expected[dtype, "max_candidates=8"][3] and np.array_equal(xy("max_candidates=8"), xy("131x97")[:8])
    # uint16 at full range: every intermediate below 2^27 (asserted inside), and something to find
    full = np.random.default_rng(5).integers(0, 65536, size=(40, 50)).astype(np.uint16)
    assert chk.response(full).max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", (np.uint8, np.uint16), ids=("uint8", "uint16"))
@pytest.mark.parametrize("name", list(GPU_CASES))
def test_response_and_candidates_equal_the_checker(amd, expected, name, dtype):
    """every pixel of R, Rmax, the candidates' pixels in their order, the overflow flag: no tolerance"""
    image, kw = GPU_CASES[name]
    image = as_dtype(image, dtype)
    q_c, response_c, status_c, overflow_c, R_c, xy_c = expected[np.dtype(dtype).name, name]
    with amd.ChessboardDetector(image.shape, image.dtype, **kw) as d:
        q, response, status = d.candidates(image)
        R, Rmax, xy = d.response()
        assert R.dtype == np.int32 and R.shape == R_c.shape
        bad = np.argwhere(R != R_c)
        assert len(bad) == 0, f"{len(bad)} of {R.size} pixels differ; the first at (y,x) = {tuple(bad[0])}: {R[tuple(bad[0])]} for {R_c[tuple(bad[0])]}"
        assert Rmax == R_c.max()
        assert np.array_equal(xy, xy_c), (len(xy), len(xy_c))
        assert np.array_equal(response, response_c) and d.overflow == overflow_c
        assert q.shape == (len(xy_c), 2) and status.shape == (len(xy_c),)


@pytest.mark.gpu
def test_full_range_uint16_equals_the_checker(amd):
    image = np.random.default_rng(5).integers(0, 65536, size=(40, 50)).astype(np.uint16)
    R_c = chk.response(image)
    xy_c, _ = chk.candidates(R_c, nms_radius=3)
    with amd.ChessboardDetector(image.shape, image.dtype, nms_radius=3) as d:
        d.candidates(image)
        R, Rmax, xy = d.response()
    assert np.array_equal(R, R_c) and Rmax == R_c.max() and np.array_equal(xy, xy_c)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", (np.uint8, np.uint16), ids=("uint8", "uint16"))
@pytest.mark.parametrize("name", STRUCTURED)
def test_refined_positions(amd, expected, name, dtype):
    """the statuses equal to the checker's, the positions within 1e-4 px. (Not on the noise image: an iteration on
    noise amplifies the last bits, and there is nothing two implementations would have to agree on)"""
    image, kw = GPU_CASES[name]
    image = as_dtype(image, dtype)
    q_c, _, status_c, _, _, xy_c = expected[np.dtype(dtype).name, name]
    q, response, status = amd.chessboard_corner_candidates(image, **kw)
    assert np.array_equal(status, status_c)
    ok = status_c == chk.STATUS_OK
    assert np.all(np.isnan(q[~ok])) and np.all(np.isfinite(q[ok]))
    if ok.any():
        worst = np.abs(q[ok] - q_c[ok]).max()
        print(f"{name}: {int(ok.sum())} of {len(ok)} refined; worst difference to the checker {worst:.3g} px")
        assert worst < 1e-4
        assert np.abs(q[ok] - xy_c[ok]).max() <= 3.5


@pytest.mark.gpu
def test_the_renders_equal_the_checker_and_find_the_board(amd):
    """two of the 800 x 600 renders through the GPU: the checker's candidates, and the board where the truth has it"""
    for k in (2, 3):
        config = CONFIGS[k]
        image, truth, q_c, response_c, status_c, overflow_c, R_c = render(k)
        with amd.ChessboardDetector(image.shape, image.dtype) as d:
            with pytest.raises(Exception, match="no image has been looked at yet"):
                d.stage_milliseconds()
            q, response, status = d.candidates(image)
            assert np.array_equal(d.response()[0], R_c) and np.array_equal(response, response_c) and np.array_equal(status, status_c)
            assert np.abs(q - q_c).max() < 1e-4
            board = d.find_board(image, 10, 7)
            ms = d.stage_milliseconds()
            assert set(ms) == {"upload", "response", "candidates", "refine", "grid"} and all(v >= 0 for v in ms.values())
            assert d.find_board(image, 10, 8) is None and d.find_board(image, 7, 10) is not None
        expected = truth[::-1, ::-1] if config["angle"] == 190. else truth
        assert board is not None and np.abs(board - expected).max() <= BOUND


@pytest.mark.gpu
def test_same_bits_on_repeated_calls(amd):
    image = GPU_CASES["131x97 noise"][0]
    kw = GPU_CASES["131x97 noise"][1]
    board = GPU_CASES["131x97"][0]
    with amd.ChessboardDetector(image.shape, image.dtype, **kw) as d0, amd.ChessboardDetector(image.shape, image.dtype, **kw) as d1:
        first = d0.candidates(image)
        assert len(first[0]) > 100
        d0.candidates(board)                                    # (another image in between: nothing of it stays)
        for again in (d0.candidates(image), d1.candidates(image), d1.candidates(image)):
            for a, b in zip(first, again):
                assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    with amd.ChessboardDetector(board.shape, board.dtype) as d0, amd.ChessboardDetector(board.shape, board.dtype) as d1:
        boards = [d.find_board(board, 5, 4) for d in (d0, d1, d0)]
        assert boards[0] is not None and all(b.tobytes() == boards[0].tobytes() for b in boards)


@pytest.mark.gpu
def test_buffer_bookkeeping(amd):
    live = amd.device_buffers_live()
    image = GPU_CASES["131x97"][0]
    d = amd.ChessboardDetector(image.shape, image.dtype)
    assert amd.device_buffers_live() == live + 1                # (ONE pooled allocation a detector)
    d.find_board(image, 5, 4)
    d.candidates(image)
    assert amd.device_buffers_live() == live + 1
    d.close()
    assert amd.device_buffers_live() == live
    d.close()
    with amd.ChessboardDetector(image.shape, image.dtype) as d:
        d.candidates(image)
    assert amd.device_buffers_live() == live
    assert amd.find_chessboard_corners(image, 5, 4) is not None and amd.device_buffers_live() == live


@pytest.mark.gpu
def test_end_to_end_from_images_to_a_calibration(amd, tmp_path):
    """six views of a 10 x 10 board rendered through an OPENCV4 lens, written as PGM: compute_chessboard_corners()
    detects them and writes the cache, reads the cache the second time, the corners are where project() puts the
    board's points, and seed_stereographic() + optimize() from the detections end with a residual below the bound.

    The views are of the kind the bound was recorded on: tilted by up to 22 degrees and, each of them, turned by 14 to 40
    degrees off the pixel grid (the last by 166: the board comes back in the labelling turned by 180). A first choice
    of views with the board's lines within 2 degrees of the pixel grid measured worst 0.255, rms 0.108 px here and
    missed the bound: that is the refinement's known weakness on lines along the grid of an image with no blur
    (test_checker_near_the_pixel_grid records it), not what this test is about"""
    from mrcal_amd.calibration import seed_stereographic
    W = H = 10
    spacing, imagersize = 0.05, (640, 480)
    lensmodel, intrinsics = "LENSMODEL_OPENCV4", np.array((520., 515., 322.3, 236.8, -0.12, 0.03, 1e-3, -5e-4))
    # (the rotation board -> camera as a Rodrigues vector, where the board's centre is in the camera's coordinates)
    views = (((0.05, 0.03, 0.30), (0.01, -0.01, 1.05)), ((0.35, -0.02, -0.50), (0.03, 0.02, 1.10)), ((-0.33, 0.05, 0.70), (-0.04, 0.03, 1.12)),
             ((0.03, 0.38, -0.25), (0.05, -0.02, 1.08)), ((-0.04, -0.36, 0.45), (-0.03, -0.02, 1.15)), ((0.22, 0.25, 2.90), (0.02, 0.01, 1.20)))
    Rt = np.array([amd.Rt_from_rt(np.array(r + (0., 0., 0.))) for r, _ in views])
    for M, (_, centre) in zip(Rt, views):
        M[3] = np.array(centre) - M[:3] @ np.array(((W - 1)*spacing/2., (H - 1)*spacing/2., 0.))
    images = chk.render_through_lens(amd.unproject, lensmodel, intrinsics, imagersize, Rt, W, H, spacing, noise=2., seed=20)
    board = np.zeros((H, W, 3)); board[..., 0], board[..., 1] = np.meshgrid(np.arange(W)*spacing, np.arange(H)*spacing)
    truth = np.array([amd.project(amd.transform_point_Rt(M, board), lensmodel, intrinsics) for M in Rt])
    truth[5] = truth[5, ::-1, ::-1].copy()                      # (the view turned by 166 degrees: +i points along +x this way round)
    assert truth[..., 0].min() > 20 and truth[..., 0].max() < 620 and truth[..., 1].min() > 20 and truth[..., 1].max() < 460
    for k, image in enumerate(images):
        write_pgm(tmp_path / f"frame{k:02d}-cam0.pgm", image)
    write_pgm(tmp_path / "frame06-cam0.pgm", np.full((480, 640), 90, dtype=np.uint8))          # (no board in this one)

    cache = tmp_path / "corners.vnl"
    kw = dict(globs_per_camera=(str(tmp_path / "frame*-cam0.pgm"),), corners_cache_vnl=str(cache))
    live = amd.device_buffers_live()
    observations, indices_frame_camera, paths = amd.compute_chessboard_corners(W, H, **kw)
    assert amd.device_buffers_live() == live
    assert cache.exists() and [p for p in os.listdir(tmp_path) if p.endswith(".vnl")] == ["corners.vnl"]
    text = cache.read_text().splitlines()
    assert text[0] == "# filename x y level" and text[-1] == f"{tmp_path}/frame06-cam0.pgm - - -" and len(text) == 1 + 6*W*H + 1
    assert paths == [str(tmp_path / f"frame{k:02d}-cam0.pgm") for k in range(6)]
    assert np.array_equal(indices_frame_camera, [(k, 0) for k in range(6)]) and observations.shape == (6, H, W, 3)
    assert np.all(observations[..., 2] == 1.)
    # the second call reads the cache: no detector, the same arrays to the bit
    class Forbidden:
        def __init__(self, *a, **k): raise AssertionError("the cache is there: nothing is detected")
    real, amd.chessboard.ChessboardDetector = amd.chessboard.ChessboardDetector, Forbidden
    try:
        again = amd.compute_chessboard_corners(W, H, jobs=-1, **kw)
    finally:
        amd.chessboard.ChessboardDetector = real
    assert again[0].tobytes() == observations.tobytes() and np.array_equal(again[1], indices_frame_camera) and again[2] == paths

    error = np.linalg.norm(observations[..., :2] - truth, axis=-1)
    print(f"detected corners against project(): worst {error.max():.4f} rms {np.sqrt((error**2).mean()):.4f} px")
    assert error.max() <= BOUND

    # detections -> seed -> calibration, stage by stage as the tool does it
    imagersizes = np.array((imagersize,), dtype=np.int32)
    core, rt_cam_ref, rt_ref_frame = seed_stereographic(imagersizes, 600., indices_frame_camera, observations, spacing)
    idx = np.ascontiguousarray(np.concatenate((indices_frame_camera, indices_frame_camera[:, 1:] - 1), -1).astype(np.int32))
    oi = dict(intrinsics=core, rt_cam_ref=rt_cam_ref, rt_ref_frame=rt_ref_frame, observations_board=observations.copy(),
              indices_frame_camintrinsics_camextrinsics=idx, lensmodel="LENSMODEL_STEREOGRAPHIC", imagersizes=imagersizes,
              do_optimize_intrinsics_core=False, do_optimize_intrinsics_distortions=False, do_optimize_calobject_warp=False,
              calibration_object_spacing=spacing, do_apply_outlier_rejection=False, do_apply_regularization=False)
    amd.optimize(**oi)
    oi["do_optimize_intrinsics_core"] = True
    amd.optimize(**oi)
    oi.update(intrinsics=np.ascontiguousarray(np.concatenate((oi["intrinsics"], np.full((1, 4), 1e-6)), -1)), lensmodel=lensmodel,
              do_optimize_intrinsics_distortions=True, do_apply_regularization=True)
    stats = amd.optimize(**oi)
    print(f"calibrated from the detections: rms {stats['rms_reproj_error__pixels']:.4f} px; intrinsics {oi['intrinsics'][0]}")
    assert stats["rms_reproj_error__pixels"] < BOUND
    assert np.abs(oi["intrinsics"][0, :4] - intrinsics[:4]).max() < 5.
