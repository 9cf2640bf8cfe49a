"""The image pyramid of find_chessboard_corners() (include/mrcal_amd.h, "chessboard corners", p1-p3; csrc/chessboard.hip,
planned by csrc/chessboard_plan.hpp): pyramid_levels, return_levels, ChessboardDetector.level_image(),
.detection_level, .pyramid_milliseconds(), and the level column of compute_chessboard_corners().

The checker (chessboard_pyramid_checker.py) restates p1-p3 in numpy on top of chessboard_checker.py. The level images,
the response and the candidates of every level tried are held to it pixel for pixel; the detection level and the
corners' levels are equal; the positions agree to 1e-4 px, the tolerance of the existing refinement test. The checker
itself is held to the analytic corners of blurred renders: 7 x 5 boards of 30, 60 and 110 px squares turned by 17
degrees with a slight perspective, noise of 1 grey level, then a Gaussian blur of sigma px, rounded to the dtype.

What was measured with the checker alone (pyramid_levels = 3, tau = 0.3 px), and is asserted below:
  sigma <= 3 (0, 1.5, 3 at 30 and 60 px; 0 at 110 px): found at level 1, 2 and 3 for the three sizes; every step of
    every corner disagrees with its start by at most 0.200 px, every corner reaches level 0, and the positions are
    those of the level-0 detector (to 1.4e-4 px: another start). Worst error against the analytic corners 0.0864 px
    (sigma = 3, 60 px); the bound is 0.10 px
    Over render seeds 1..8 the level-0 refinement's worst corner at sigma = 3 lies between 0.056 and 0.107 px (0.121 with
    one more seed tried): the 11 x 11 window of part d is small for that blur, with or without a pyramid. The bound
    holds with the seeds of the sweep (a case's place in it); it is not a bound for every seed at sigma = 3
  sigma = 4: the steps to level 0 disagree by 0.003 .. 0.66 px with no gap between good and bad; 18 and 17 of 35
    corners reach level 0. Worst error 0.3227 px (30 px), 0.2953 px (60 px). The level-0 detector alone "finds" all 35
    with errors of 1.09 and 0.87 px
  sigma = 6: every level-0 refinement leaves its +-3.5 px box (35 candidates, none of status 0: no board at level 0); the
    corners stay at level 1. Worst error 0.2025, 0.1987, 0.1892 px at 30, 60, 110 px
  the bound for sigma in {4, 6}: the worst of these, 0.3227 px, plus 25 %: 0.4034 px, for render seeds that are not in
    the sweep
  no step of the sweep lies within 1e-6 px of tau"""
import functools

import numpy as np
import pytest

import hostbuild
import chessboard_checker as chk
import chessboard_pyramid_checker as pc

LEVELS = 3
BOUND_SHARP = 0.10              # px, sigma <= 3: what the issue holds the level-0 detector to
# measured once with the checker (the docstring above): the worst |error| along x or y, in px
RECORDED_SHARP = 0.0864
RECORDED_BLURRED = {(4., 30): 0.3227, (4., 60): 0.2953, (6., 30): 0.2025, (6., 60): 0.1987, (6., 110): 0.1892}
BOUND_BLURRED = 1.25*max(RECORDED_BLURRED.values())
NEAR_TAU = 1e-6


def grid(*a, **k):
    import mrcal_amd
    return mrcal_amd.chessboard_grid(*a, **k)


@functools.lru_cache(maxsize=None)
def case(sigma, square, dtype="uint8"):
    """a render of the sweep, its true corners and what the checker makes of it with pyramid_levels = 3; made once"""
    image, truth = pc.blurred_render(sigma, square, dtype=np.dtype(dtype).type)
    return image, truth, pc.detect_pyramid(image, *pc.BOARD, LEVELS, grid)


@functools.lru_cache(maxsize=None)
def cluttered():
    image, truth = pc.cluttered_render()
    return image, truth, pc.detect_pyramid(image, *pc.BOARD, LEVELS, grid)


def worst_error(result, truth):
    return float(np.abs(result["corners"] - truth).max())


# ------------------------------------------------------------------------------------------------ without a GPU ---
def test_levels_and_refusals_before_any_device_work(amd, monkeypatch):
    def no_device(*a, **k): raise AssertionError("device work before the refusal")
    monkeypatch.setattr(amd._handle, "_libs", no_device)
    find, Detector = amd.find_chessboard_corners, amd.ChessboardDetector
    # the sizes of the levels: an odd last row or column is dropped at every step
    d = Detector.__new__(Detector)
    d.shape = (67, 65)
    assert [d.level_shape(l) for l in range(3)] == [(67, 65), (33, 32), (16, 16)] == [pc.level_shape((67, 65), l) for l in range(3)]
    d.shape = (640, 800)
    assert [d.level_shape(l) for l in range(5)] == [(640, 800), (320, 400), (160, 200), (80, 100), (40, 50)]
    d.shape = (97, 130)
    assert [d.level_shape(l) for l in (1, 2)] == [(48, 65), (24, 32)]
    # the largest pyramid_levels of a size, as the refusal names it
    for (H, W), most, next_level in (((32, 32), 0, "16 x 16"), ((65, 64), 1, "16 x 16"), ((64, 65), 1, "16 x 16"), ((640, 800), 4, "25 x 20")):
        assert pc.max_levels((H, W)) == most
        words = f"^find_chessboard_corners\\(\\): an image of {W} x {H} pixels is too small for pyramid_levels = {most + 1}: " \
                f"level {most + 1} would have {next_level} pixels, at least 32 x 32; at most pyramid_levels = {most}$"
        with pytest.raises(Exception, match=words):
            Detector((H, W), np.uint8, pyramid_levels=most + 1)
        with pytest.raises(Exception, match=words):
            find(np.zeros((H, W), dtype=np.uint16), 7, 5, pyramid_levels=most + 1)
        with pytest.raises(AssertionError, match="device work"):        # (the largest one is not refused)
            Detector((H, W), np.uint8, pyramid_levels=most)
    for bad in (-1, 9, 2., True, None):
        with pytest.raises(Exception, match="^find_chessboard_corners\\(\\): pyramid_levels must be in 0..8, got"):
            Detector((640, 800), np.uint8, pyramid_levels=bad)
        with pytest.raises(Exception, match="^find_chessboard_corners\\(\\): pyramid_levels must be in 0..8, got"):
            find(np.zeros((640, 800), dtype=np.uint8), 7, 5, pyramid_levels=bad)
        with pytest.raises(Exception, match="^find_chessboard_corners\\(\\): pyramid_levels must be in 0..8, got"):
            amd.compute_chessboard_corners(7, 5, globs_per_camera=("no-such-*.pgm",), pyramid_levels=bad)
        with pytest.raises(Exception, match="^find_chessboard_corners\\(\\): pyramid_levels must be in 0..8, got"):
            amd.compute_chessboard_corners(7, 5, globs_per_camera=("no-such-*.pgm",), detector_params={"pyramid_levels": bad})
    # the refusals that were there come first
    with pytest.raises(Exception, match="is too small: at least 32 x 32$"):
        Detector((31, 800), np.uint8, pyramid_levels=1)
    with pytest.raises(Exception, match="nms_radius must be in 1..16, got 0$"):
        find(np.zeros((640, 800), dtype=np.uint8), 7, 5, nms_radius=0, pyramid_levels=9)
    # a closed detector says so
    d = Detector.__new__(Detector)
    d.handle, d.shape, d.dtype, d.max_candidates, d.pyramid_levels = None, (640, 800), np.dtype(np.uint8), 4096, 3
    for call in (lambda: d.level_image(1), d.pyramid_milliseconds, lambda: d.find_board(np.zeros((640, 800), dtype=np.uint8), 7, 5, return_levels=True)):
        with pytest.raises(Exception, match="^this ChessboardDetector has been closed$"):
            call()
    d.handle = 1
    for bad in (-1, 4, 1.):
        with pytest.raises(Exception, match=f"^find_chessboard_corners\\(\\): this detector has the levels 0..3, and level {bad} was asked for$"):
            d.level_image(bad)


def test_pyramid_plan_under_the_host_sanitizers():
    """csrc/chessboard_plan.hpp's pyramid plan driven by a stand-alone program with its own main, built with ASan and
    UBSan: the level geometry, the refusals, and pyramid_levels = 0 giving the plan there was, field for field"""
    hostbuild.assert_prints_ok("chessboard_pyramid_plan_check")


def test_decimation_of_the_checker():
    """p1 by hand on a 5 x 7 image: rounding to nearest with .5 up, the odd row and column dropped, both dtypes alike"""
    I = np.array(((0, 1, 2, 3, 4, 5, 6), (1, 1, 1, 1, 255, 255, 9), (255, 255, 0, 0, 10, 11, 9), (255, 254, 0, 1, 12, 13, 9), (7, 7, 7, 7, 7, 7, 7)))
    expected = ((1, 2, 130), (255, 0, 12))       # (3/4 -> 1, 7/4 -> 2, 519/4 -> 130; 1019/4 -> 255, 1/4 -> 0, 46/4 -> 12)
    for dtype in (np.uint8, np.uint16):
        out = pc.decimate(I.astype(dtype))
        assert out.dtype == dtype and np.array_equal(out, expected)
    full = np.full((4, 4), 65535, dtype=np.uint16)
    assert np.array_equal(pc.decimate(full), np.full((2, 2), 65535))


def test_the_checker_is_about_something(amd):
    """at sigma = 6 on the 60 px render the level-0 detector has no candidate that survives its refinement, so no board;
    the pyramid finds it within the bound. At sigma = 0 every corner reaches level 0, and its position is that of a
    level-0 refinement started from the float start"""
    image, truth, result = case(6., 60)
    R = chk.response(image)
    xy, _ = chk.candidates(R)
    q, status, _ = chk.refine(image, xy)
    print(f"sigma 6, level 0: {len(xy)} candidates, statuses {np.bincount(status, minlength=3)}")
    assert not np.any(status == chk.STATUS_OK) and np.all(np.isnan(q))
    assert amd.chessboard_grid(q, *pc.BOARD, response=R[xy[:, 1], xy[:, 0]], status=status) is None
    assert result is not None and result["detection_level"] == 2 and np.all(result["levels"] == 1)
    assert worst_error(result, truth) <= BOUND_BLURRED

    image, truth, result = case(0., 60)
    assert result is not None and result["detection_level"] == 2 and np.all(result["levels"] == 0)
    # the last step of every corner: from up() of its level-1 position
    last = {c: d for l, c, d in result["disagreement"] if l == 0}
    assert sorted(last) == list(range(35)) and max(last.values()) <= pc.TAU
    level1 = pc.detect_pyramid(result["images"][1], *pc.BOARD, 1, grid)       # (the same descent, stopped a level above)
    assert level1["detection_level"] == 1 and np.all(level1["levels"] == 0)
    start = pc.up(level1["corners"].reshape(-1, 2))
    refined, status, _ = chk.refine(image, start)
    assert np.all(status == chk.STATUS_OK) and np.array_equal(refined.reshape(5, 7, 2), result["corners"])
    assert np.array_equal(np.abs(refined - start).max(-1), [last[c] for c in range(35)])


def test_checker_against_truth():
    """the sweep: the errors against the analytic corners, the bounds and what is recorded (the docstring of this file)"""
    steps = near = 0
    sharp, blurred = 0., {}
    for sigma, square in pc.SWEEP:
        image, truth, result = case(sigma, square)
        assert result is not None, (sigma, square)
        error = worst_error(result, truth)
        d = np.array([x for _, _, x in result["disagreement"]])
        steps += len(d)
        with np.errstate(invalid="ignore"):
            near += int((np.abs(d - pc.TAU) <= NEAR_TAU).sum())
        print(f"sigma {sigma:g} square {square}: found at level {result['detection_level']}, corners at levels "
              f"{np.bincount(result['levels'].ravel(), minlength=4)}, worst error {error:.4f} px, steps disagree by "
              f"{np.min(d[np.isfinite(d)], initial=np.inf):.3f} .. {np.max(d[np.isfinite(d)], initial=-np.inf):.3f} px ({int(np.isnan(d).sum())} failed)")
        assert result["detection_level"] == {30: 1, 60: 2, 110: 3}[square]
        if sigma <= 3.:
            assert np.all(result["levels"] == 0) and d.max() <= pc.TAU
            # ... and that IS the level-0 detector, where it finds the board
            board = pc.detect_level(image, grid, *pc.BOARD)[0]
            # (two refinements that stop at a step below 1e-5 px, from starts up to 0.7 px apart: the iteration closes
            # in on its fixed point by a factor of about 0.9 a step, so each is within 1e-4 px of it; 1.4e-4 is measured)
            assert board is not None and np.abs(board - result["corners"]).max() < 1e-3
            assert error <= BOUND_SHARP
            sharp = max(sharp, error)
        else:
            assert error <= BOUND_BLURRED
            blurred[sigma, square] = error
            if sigma == 6.: assert np.all(result["levels"] == 1)
            else:           assert 0 < (result["levels"] == 0).sum() < 35 and result["levels"].max() == 1
    print(f"sigma <= 3: worst {sharp:.4f} px; sigma in (4, 6): {blurred}; {near} of {steps} steps within {NEAR_TAU} px of tau")
    assert abs(sharp - RECORDED_SHARP) < 1e-3                                      # (what is recorded is what is)
    assert set(blurred) == set(RECORDED_BLURRED) and all(abs(blurred[k] - RECORDED_BLURRED[k]) < 1e-3 for k in blurred)
    # corners within 1e-6 px of tau may be left out of the GPU's level comparison: at most 2 % of the sweep's
    assert near <= 0.02*35*len(pc.SWEEP)
    # a seed that is not in the sweep
    for sigma, square in ((4., 30), (6., 60)):
        image, truth = pc.blurred_render(sigma, square, seed=77)
        result = pc.detect_pyramid(image, *pc.BOARD, LEVELS, grid)
        print(f"sigma {sigma:g} square {square}, another seed: worst error {worst_error(result, truth):.4f} px")
        assert result is not None and worst_error(result, truth) <= BOUND_BLURRED


def test_the_cluttered_render_is_about_something():
    image, truth, result = cluttered()
    assert result is not None and result["detection_level"] == 2 and np.all(result["levels"] == 0)
    assert worst_error(result, truth) <= BOUND_SHARP
    for level, (R, xy) in result["tried"].items():
        print(f"clutter: level {level}: {len(xy)} candidates")
    assert len(result["tried"][3][1]) > 0 and len(result["tried"][2][1]) > 35       # (more than the board's own)


# --------------------------------------------------------------------------------------------------- on the GPU ---
def decimation_images():
    rng = np.random.default_rng(3)
    return {"65x67": rng.integers(0, 256, size=(67, 65)).astype(np.uint8),
            "130x97": rng.integers(0, 256, size=(97, 130)).astype(np.uint8),
            "800x640 render": case(0., 60)[0],
            "full-range uint16": rng.integers(0, 65536, size=(200, 264)).astype(np.uint16)}


@pytest.mark.gpu
@pytest.mark.parametrize("name,dtype", [(name, dtype) for name in ("65x67", "130x97", "800x640 render") for dtype in (np.uint8, np.uint16)] +
                                       [("full-range uint16", np.uint16)],
                         ids=lambda x: x if isinstance(x, str) else np.dtype(x).name)
def test_decimation_equals_the_checker(amd, name, dtype):
    """every pixel of every level the size allows. 65 x 67 and 130 x 97 have rows that are no whole 16-byte words (a
    lane an output pixel) and the smallest legal levels; 800 x 640 takes the wide kernel down to the level whose rows
    are 200 (uint8) or 400 (uint16) bytes"""
    image = decimation_images()[name]
    if dtype == np.uint16 and image.dtype == np.uint8:
        image = image.astype(np.uint16)*257
    n = min(pc.max_levels(image.shape), 8)
    assert n >= 1
    expected = pc.pyramid(image, n)
    with amd.ChessboardDetector(image.shape, image.dtype, pyramid_levels=n) as d:
        d.find_board(image, *pc.BOARD)
        for l in range(n + 1):
            level = d.level_image(l)
            assert level.dtype == image.dtype and level.shape == expected[l].shape
            bad = np.argwhere(level != expected[l])
            assert len(bad) == 0, f"level {l}: {len(bad)} of {level.size} pixels differ; the first at (y,x) = {tuple(bad[0])}"


SWEEP_IDS = [f"sigma{sigma:g}-{square}px" for sigma, square in pc.SWEEP]


def compare_with_the_checker(amd, image, result):
    """-> (corners compared, corners left out of the level comparison)"""
    with amd.ChessboardDetector(image.shape, image.dtype, pyramid_levels=LEVELS) as d:
        with pytest.raises(Exception, match="no image has been looked at through the pyramid yet"):
            d.pyramid_milliseconds()
        corners, levels = d.find_board(image, *pc.BOARD, return_levels=True)
        assert (corners is not None) == (result is not None)
        if result is None:
            assert levels is None and d.detection_level is None
            return 0, 0
        assert d.detection_level == result["detection_level"]
        assert corners.shape == (5, 7, 2) and levels.shape == (5, 7) and levels.dtype == np.int32
        ms = d.pyramid_milliseconds()
        assert set(ms) == {"decimate", "descent", "per_level"} and len(ms["per_level"]) == LEVELS + 1
        assert all((ms["per_level"][l] > 0) == (l in result["tried"]) for l in range(LEVELS + 1))
        assert set(d.stage_milliseconds()) == {"upload", "response", "candidates", "refine", "grid"}
        R_last = d.response()[0]
        assert np.array_equal(R_last, result["tried"][result["detection_level"]][0])
        images = [d.level_image(l) for l in range(LEVELS + 1)]
    for l in range(LEVELS + 1):
        assert np.array_equal(images[l], result["images"][l]), f"level {l}"
    # the response and the candidates of every level tried: a single-level call on the level's image
    for l, (R_c, xy_c) in result["tried"].items():
        with amd.ChessboardDetector(images[l].shape, images[l].dtype) as one_level:
            one_level.candidates(images[l])
            R, Rmax, xy = one_level.response()
        assert np.array_equal(R, R_c) and Rmax == R_c.max() and np.array_equal(xy, xy_c), f"level {l}"
    # a corner whose step lies within 1e-6 px of tau may go either way
    unsure = {c for _, c, delta in result["disagreement"] if abs(delta - pc.TAU) <= NEAR_TAU}
    sure = np.array([c not in unsure for c in range(35)])
    assert np.array_equal(levels.ravel()[sure], result["levels"].ravel()[sure])
    worst = np.abs(corners.reshape(-1, 2)[sure] - result["corners"].reshape(-1, 2)[sure]).max()
    print(f"found at level {d.detection_level}; corners at levels {np.bincount(levels.ravel(), minlength=4)}; worst difference to the checker {worst:.3g} px")
    assert worst < 1e-4
    return int(sure.sum()), len(unsure)


@pytest.mark.gpu
@pytest.mark.parametrize("which", range(len(pc.SWEEP)), ids=SWEEP_IDS)
def test_pyramid_equals_the_checker(amd, which):
    sigma, square = pc.SWEEP[which]
    image, truth, result = case(sigma, square)
    compared, left_out = compare_with_the_checker(amd, image, result)
    assert compared == 35 and left_out == 0         # (test_checker_against_truth: no step of the sweep is near tau)


@pytest.mark.gpu
def test_pyramid_equals_the_checker_with_clutter_and_uint16(amd):
    image, truth, result = cluttered()
    assert compare_with_the_checker(amd, image, result) == (35, 0)
    image, truth, result = case(4., 60, "uint16")
    # (at 16 bits the rounding of the grey levels is out of the way, and every corner reaches level 0 at sigma = 4)
    assert result is not None and result["detection_level"] == 2 and np.all(result["levels"] == 0)
    assert compare_with_the_checker(amd, image, result) == (35, 0)
    # nothing to find at any level
    with amd.ChessboardDetector((400, 480), np.uint8, pyramid_levels=LEVELS) as d:
        flat = np.full((400, 480), 90, dtype=np.uint8)
        assert d.find_board(flat, *pc.BOARD) is None and d.find_board(flat, *pc.BOARD, return_levels=True) == (None, None)
        assert d.detection_level is None and d.response()[0].shape == (400, 480)
        assert all(ms > 0 for ms in d.pyramid_milliseconds()["per_level"])       # (every level was tried)


@pytest.mark.gpu
def test_nothing_changed_at_the_default(amd):
    """pyramid_levels = 0 through the old and the new entry points: the corners of find_board() to the bit, levels 0"""
    import test_chessboard as tc
    images = [(chk.render_numpy(10, 7, **tc.CONFIGS[k])[0], (10, 7)) for k in (2, 3)] + [(tc.GPU_CASES["131x97"][0], (5, 4)), (case(0., 30)[0], pc.BOARD),
                                                            (case(6., 30)[0], pc.BOARD)]
    for image, (W, H) in images:
        with amd.ChessboardDetector(image.shape, image.dtype) as d:
            old = d.find_board(image, W, H)
            candidates = d.candidates(image)
            new, levels = d.find_board(image, W, H, return_levels=True)
            assert d.detection_level == (None if old is None else 0)
        one_shot = amd.find_chessboard_corners(image, W, H)
        keyword, levels_keyword = amd.find_chessboard_corners(image, W, H, pyramid_levels=0, return_levels=True)
        if old is None:
            assert new is None and levels is None and one_shot is None and keyword is None and levels_keyword is None
            continue
        for other in (new, one_shot, keyword):
            assert other.dtype == old.dtype and other.tobytes() == old.tobytes()
        assert levels.dtype == np.int32 and levels.shape == (H, W) and not levels.any() and not levels_keyword.any()
        # level 0 of a detector WITH levels is the detector without: candidates() looks at it alone
        with amd.ChessboardDetector(image.shape, image.dtype, pyramid_levels=1) as d:
            for a, b in zip(candidates, d.candidates(image)):
                assert a.tobytes() == b.tobytes()
            assert d.find_board(image, W, H, return_levels=True)[0] is not None
            assert np.array_equal(d.level_image(0), image)
    assert images[-1][0] is case(6., 30)[0] and old is None        # (the blurred one: today's detector finds nothing)


@pytest.mark.gpu
def test_same_bits_and_one_detector_for_images_of_other_levels(amd):
    live = amd.device_buffers_live()
    blurred, sharp = case(6., 30)[0], case(0., 30)[0]
    small, _ = pc.blurred_render(0., 30, seed=50, size=(480, 400))
    small_squares, _ = chk.render_numpy(*pc.BOARD, width=480, height=400, square=14., angle=17., noise=1., seed=51)
    flat = np.full((400, 480), 90, dtype=np.uint8)
    expected = {id(im): pc.detect_pyramid(im, *pc.BOARD, LEVELS, grid) for im in (small, small_squares)}
    assert expected[id(small)]["detection_level"] == 1 and expected[id(small_squares)]["detection_level"] == 0
    d0 = amd.ChessboardDetector((400, 480), np.uint8, pyramid_levels=LEVELS)
    assert amd.device_buffers_live() == live + 1                # (ONE pooled allocation a detector, levels and all)
    with amd.ChessboardDetector((400, 480), np.uint8, pyramid_levels=LEVELS) as d1:
        assert amd.device_buffers_live() == live + 2
        first = {id(im): d0.find_board(im, *pc.BOARD, return_levels=True) for im in (blurred, sharp, small_squares)}
        assert np.all(first[id(blurred)][1] == 1) and not first[id(sharp)][1].any() and not first[id(small_squares)][1].any()
        # images found at other levels, and none, in between: nothing of them stays
        for d, im, level in ((d0, small_squares, 0), (d0, flat, None), (d0, blurred, 1), (d1, blurred, 1), (d0, small, 1), (d1, sharp, 1),
                             (d0, sharp, 1), (d1, small_squares, 0), (d0, small_squares, 0), (d1, blurred, 1)):
            corners, levels = d.find_board(im, *pc.BOARD, return_levels=True)
            assert d.detection_level == level
            if id(im) in first:
                assert corners.tobytes() == first[id(im)][0].tobytes() and levels.tobytes() == first[id(im)][1].tobytes()
            if id(im) in expected:
                assert np.array_equal(levels, expected[id(im)]["levels"]) and np.abs(corners - expected[id(im)]["corners"]).max() < 1e-4
    assert amd.device_buffers_live() == live + 1
    d0.close()
    assert amd.device_buffers_live() == live
    d0.close()
    assert amd.find_chessboard_corners(blurred, *pc.BOARD, pyramid_levels=LEVELS) is not None and amd.device_buffers_live() == live


@pytest.mark.gpu
def test_end_to_end_levels_into_the_corners_file(amd, tmp_path):
    """six 480 x 400 renders as PGM, frames 2 and 4 blurred by 6 px. With pyramid_levels = 3 all six boards are there,
    the level column is non-zero exactly for the blurred ones and comes back as the weight 2^-level; without the key the
    blurred ones are not found, as before"""
    from test_chessboard import write_pgm, BOUND
    W, H = pc.BOARD
    frames = [(0., 17.), (0., 28.), (6., 17.), (1.5, -24.), (6., 35.), (0., 200.)]
    for k, (sigma, angle) in enumerate(frames):
        write_pgm(tmp_path / f"frame{k}-cam0.pgm", pc.blurred_render(sigma, 30, seed=60 + k, angle=angle)[0])
    glob = (str(tmp_path / "frame*-cam0.pgm"),)
    live = amd.device_buffers_live()
    cache = tmp_path / "levels.vnl"
    observations, indices, paths = amd.compute_chessboard_corners(W, H, globs_per_camera=glob, corners_cache_vnl=str(cache),
                                                                     detector_params={'pyramid_levels': LEVELS})
    assert amd.device_buffers_live() == live
    assert paths == [str(tmp_path / f"frame{k}-cam0.pgm") for k in range(6)] and observations.shape == (6, H, W, 3)
    rows = [line.split() for line in cache.read_text().splitlines()[1:]]
    assert len(rows) == 6*W*H and all(len(r) == 4 for r in rows)
    for k, (sigma, _) in enumerate(frames):
        column = np.array([int(r[3]) for r in rows[k*W*H:(k + 1)*W*H]])
        assert np.all(column == 1) if sigma == 6. else not column.any(), k
        assert np.array_equal(observations[k, ..., 2].ravel(), 0.5**column)
        truth = pc.blurred_render(0., 30, seed=60 + k, angle=frames[k][1])[1]
        if frames[k][1] == 200.: truth = truth[::-1, ::-1]
        assert np.abs(observations[k, ..., :2] - truth).max() <= (BOUND_BLURRED if sigma == 6. else BOUND), k
    # the cache read back: the same arrays to the bit, no detector
    again = amd.compute_chessboard_corners(W, H, globs_per_camera=glob, corners_cache_vnl=str(cache), jobs=-1)
    assert again[0].tobytes() == observations.tobytes() and again[2] == paths
    # without the key: today's file
    plain = tmp_path / "plain.vnl"
    observations0, _, paths0 = amd.compute_chessboard_corners(W, H, globs_per_camera=glob, corners_cache_vnl=str(plain))
    assert paths0 == [str(tmp_path / f"frame{k}-cam0.pgm") for k in (0, 1, 3, 5)] and np.all(observations0[..., 2] == 1.)
    text = plain.read_text().splitlines()
    assert text[0] == "# filename x y level" and len(text) == 1 + 4*W*H + 2
    assert [t for t in text if t.endswith(" - - -")] == [f"{tmp_path}/frame{k}-cam0.pgm - - -" for k in (2, 4)]
    # (sharp boards: the same corners, refined from another start)
    assert np.abs(observations0 - observations[[0, 1, 3, 5]]).max() < 1e-3
