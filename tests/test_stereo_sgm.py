"""stereo_matching_sgm(): dense disparities of a rectified pair by semi-global matching on a census cost.

Without a GPU: the checker (tests/stereo_sgm_checker.py: the definition in numpy on int64) against plain per-pixel,
per-disparity loops, its accuracy on a slanted plane, every refusal before any device work, and the host planning
(csrc/sgm_plan.hpp) as a stand-alone program under the host sanitizers. On the GPU: EQUALITY with the checker, every
pixel, over the sizes, disparity ranges and parameters at which a kernel takes another path; ties, the floor of a
negative subpixel numerator, uint16, the resident object, and image pair -> rectification -> disparity -> range."""
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR
import hostbuild
import stereo_sgm_checker as chk


@pytest.fixture(scope="module")
def image():
    return np.load(os.path.join(GOLDEN_DIR, "match_feature_image.npz"))["image"]


def slanted_pair(image):
    """image0: a cut of the fixture; image1(y,x1) = its row at 250 + x1 + 6 + 0.03 x1: the left disparity is
    (6 + 0.03 x)/1.03"""
    image0 = np.ascontiguousarray(image[180:276, 250:410])
    x1 = np.arange(160)
    at = 250 + x1 + 6 + 0.03*x1
    x0 = np.floor(at).astype(int)
    f  = at - x0
    rows = image[180:276].astype(np.float64)
    image1 = np.rint(rows[:, x0]*(1 - f) + rows[:, x0 + 1]*f).astype(np.uint8)
    return image0, image1, (6 + 0.03*np.arange(160))/1.03


def piecewise_pair(image, H, W, disparity_min):
    """a cut of the fixture and the same cut seen disparity_min + 3 (the left half) and disparity_min + 9 (the right
    half) pixels further on"""
    r0, c0 = 180, 250
    image0 = np.ascontiguousarray(image[r0:r0 + H, c0:c0 + W])
    x1 = np.arange(W)
    shift = np.where(x1 < W//2, disparity_min + 3, disparity_min + 9)
    image1 = np.ascontiguousarray(image[r0:r0 + H][:, c0 + x1 + shift])
    return image0, image1


def noise_pair(H, W, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, size=(H, W), dtype=np.uint8), rng.integers(0, 256, size=(H, W), dtype=np.uint8)


SIZES = ((7, 9), (8, 63), (9, 64), (10, 65), (64, 17), (65, 130), (130, 131))      # (H,W)
DS    = (16, 48, 64, 80, 128, 256)
DMINS = (-20, 0, 5)
PS    = ((0, 0), (10, 120), (193, 193))
RATIOS, DIFFS = (0, 10, 99), (-1, 0, 1)


def equality_cases():
    """42 of the product. 7 sizes and 6 ranges: c -> (c % 7, c % 6) meets every pair of them once. A D (which is a
    kernel instantiation) is met by k = c // 6 = 0..6, and every other parameter steps with k, from an offset that
    depends on D (or, disp12_max_diff, at another pace): each D meets every value of every parameter, both path counts
    and both kinds of image, and no two parameters move together over the whole list"""
    out = []
    for c in range(42):
        k, j = c // 6, c % 6
        out.append(dict(size=SIZES[c % 7], D=DS[j], disparity_min=DMINS[k % 3], P=PS[(k + j) % 3], paths=(4, 8)[(k + j) % 2],
                        uniqueness_ratio=RATIOS[(k + 2*j) % 3], disp12_max_diff=DIFFS[(k + k//3) % 3],
                        noise=bool((k + j//2) % 2)))
    return out


def case_id(case):
    return "{}x{}-D{}-min{}-P{}_{}-paths{}-u{}-lr{}-{}".format(*case["size"], case["D"], case["disparity_min"], *case["P"], case["paths"],
                                                               case["uniqueness_ratio"], case["disp12_max_diff"],
                                                               "noise" if case["noise"] else "texture")


def case_keywords(case):
    return dict(disparity_min=case["disparity_min"], disparity_max=case["disparity_min"] + case["D"], P1=case["P"][0], P2=case["P"][1],
                paths=case["paths"], uniqueness_ratio=case["uniqueness_ratio"], disp12_max_diff=case["disp12_max_diff"])


# ------------------------------------------------------------------------------------------------ without a GPU ---
def test_the_cases_cover_what_they_claim():
    cases = equality_cases()
    assert len(cases) == 42 and len({(c["size"], c["D"]) for c in cases}) == 42
    for D in DS:
        mine = [c for c in cases if c["D"] == D]
        assert {c["disparity_min"] for c in mine} == set(DMINS) and {c["P"] for c in mine} == set(PS)
        assert {c["uniqueness_ratio"] for c in mine} == set(RATIOS) and {c["disp12_max_diff"] for c in mine} == set(DIFFS)
        assert {c["paths"] for c in mine} == {4, 8} and {c["noise"] for c in mine} == {False, True}
    assert any(c["size"][1] < c["D"] for c in cases)


@pytest.mark.parametrize("uniqueness_ratio", (0, 15))
@pytest.mark.parametrize("disparity_min", (-3, 2))
@pytest.mark.parametrize("paths", (4, 8))
def test_checker_against_plain_loops(paths, disparity_min, uniqueness_ratio):
    rng = np.random.default_rng(100*paths + 10*(disparity_min + 3) + uniqueness_ratio)
    image0 = rng.integers(0, 256, size=(7, 11), dtype=np.uint8)
    image1 = np.roll(image0, -(disparity_min + 5), axis=1)
    image1[2] = rng.integers(0, 256, size=11)
    kw = dict(disparity_min=disparity_min, disparity_max=disparity_min + 16, paths=paths, uniqueness_ratio=uniqueness_ratio)
    d = chk.stereo_matching_sgm(image0, image1, **kw)
    assert d.shape == (7, 11) and d.dtype == np.int16
    assert np.array_equal(d, chk.stereo_matching_sgm_loops(image0, image1, **kw))
    # both kinds of pixel are there
    invalid = d == 16*(disparity_min - 1)
    assert invalid.any() and not invalid.all()


def test_checker_on_a_slanted_plane(image):
    """measured: 0.9986 of the pixels valid, 0.9996 of those within 1 px, the median error 0.154 px"""
    image0, image1, truth = slanted_pair(image)
    d = chk.stereo_matching_sgm(image0, image1, disparity_min=0, disparity_max=32)
    d, truth = d[:, 16:], truth[16:]
    valid = d >= 0
    err = np.abs(d/16. - truth)
    print(f"valid {valid.mean():.4f}, within 1 px {(err[valid] <= 1).mean():.4f}, median error {np.median(err[valid]):.3f} px")
    assert valid.mean() >= 0.99
    assert (err[valid] <= 1).mean() >= 0.99


def test_refusals_before_any_device_work(amd, monkeypatch):
    def no_device(*a, **k): raise AssertionError("device work before the refusal")
    monkeypatch.setattr(amd._handle, "_libs", no_device)
    a = np.zeros((20, 30), dtype=np.uint8)
    sgm = amd.stereo_matching_sgm
    with pytest.raises(TypeError, match="disparity_max"):
        sgm(a, a)
    with pytest.raises(Exception, match="ONLY grayscale images of shape \\(H,W\\)"):
        sgm(np.zeros((20, 30, 3), dtype=np.uint8), a, disparity_max=16)
    with pytest.raises(Exception, match="ONLY grayscale images of shape \\(H,W\\)"):
        sgm(a, np.zeros((20, 30, 3), dtype=np.uint8), disparity_max=16)
    with pytest.raises(Exception, match="ONLY grayscale images of shape \\(H,W\\)"):
        sgm(a, [[0]], disparity_max=16)
    with pytest.raises(Exception, match="must have the same shape"):
        sgm(a, a[:, :-1], disparity_max=16)
    with pytest.raises(Exception, match="must have the same dtype"):
        sgm(a, a.astype(np.uint16), disparity_max=16)
    with pytest.raises(Exception, match="dtype uint8 or uint16, not float32"):
        sgm(a.astype(np.float32), a.astype(np.float32), disparity_max=16)
    for dmin, dmax in ((0, 0), (0, 40), (0, 272), (16, 0), (-8, 0)):
        with pytest.raises(Exception, match="must be a positive multiple of 16, at most 256"):
            sgm(a, a, disparity_min=dmin, disparity_max=dmax)
    with pytest.raises(Exception, match="disparity_max must be an integer"):
        sgm(a, a, disparity_max=16.)
    for P1, P2 in ((-1, 120), (121, 120), (10, 194)):
        with pytest.raises(Exception, match="must have 0 <= P1 <= P2 <= 193"):
            sgm(a, a, disparity_max=16, P1=P1, P2=P2)
    for paths in (0, 5, 16):
        with pytest.raises(Exception, match="paths must be 4 or 8"):
            sgm(a, a, disparity_max=16, paths=paths)
    for ratio in (-1, 100):
        with pytest.raises(Exception, match="uniqueness_ratio must be in 0..99"):
            sgm(a, a, disparity_max=16, uniqueness_ratio=ratio)
    for dmin in (2032, -2048):
        with pytest.raises(Exception, match="leave int16"):
            sgm(a, a, disparity_min=dmin, disparity_max=dmin + 16)
    # the resident object refuses the same, and a shape that is none
    with pytest.raises(Exception, match="paths must be 4 or 8"):
        amd.StereoMatcherSGM((20, 30), np.uint8, disparity_max=16, paths=3)
    with pytest.raises(Exception, match="dtype uint8 or uint16"):
        amd.StereoMatcherSGM((20, 30), np.float32, disparity_max=16)
    with pytest.raises(Exception, match="shape must be \\(H,W\\)"):
        amd.StereoMatcherSGM((20, 30, 3), np.uint8, disparity_max=16)
    with pytest.raises(Exception, match="shape must be \\(H,W\\)"):
        amd.StereoMatcherSGM((0, 30), np.uint8, disparity_max=16)
    # (what is in order goes on to the device)
    with pytest.raises(AssertionError, match="device work"):
        sgm(a, a, disparity_min=-2047, disparity_max=-2031, P1=0, P2=0, paths=4, uniqueness_ratio=99, disp12_max_diff=-5)
    assert amd.STEREO_SGM_DISPARITY_SCALE == 16 == chk.SCALE


def test_rectification_disparity_refuses_before_any_device_work(amd):
    """Rectification.disparity() checks its arguments before it calls the library"""
    r = amd.Rectification.__new__(amd.Rectification)        # (no device: the object is not initialised)
    r.handle, r._L = 1, None
    a = np.zeros((20, 30), dtype=np.uint8)
    with pytest.raises(Exception, match="paths must be 4 or 8"):
        r.disparity(a, a, disparity_max=16, paths=2)
    with pytest.raises(Exception, match="ONLY grayscale images"):
        r.disparity(np.zeros((20, 30, 3), dtype=np.uint8), a, disparity_max=16)
    with pytest.raises(Exception, match="must have the same dtype"):
        r.disparity(a, a.astype(np.uint16), disparity_max=16)
    with pytest.raises(Exception, match="dtype uint8 or uint16"):
        r.disparity(a.astype(np.float32), a.astype(np.float32), disparity_max=16)
    r.handle = None


def test_sgm_plan_under_the_host_sanitizers():
    """csrc/sgm_plan.hpp driven by a stand-alone program with its own main, built with ASan and UBSan"""
    hostbuild.assert_prints_ok("sgm_plan_check")


# --------------------------------------------------------------------------------------------------- on the GPU ---
def report_difference(got, expected):
    bad = np.argwhere(got != expected)
    return f"{len(bad)} of {got.size} pixels differ; the first at (y,x) = {tuple(bad[0])}: {got[tuple(bad[0])]} for {expected[tuple(bad[0])]}"


def assert_same(got, expected):
    assert got.dtype == np.int16 and got.shape == expected.shape
    assert np.array_equal(got, expected), report_difference(got, expected)


@pytest.mark.gpu
@pytest.mark.parametrize("case", equality_cases(), ids=case_id)
def test_equals_the_checker(amd, image, case):
    """every pixel, no tolerance"""
    (H, W), kw = case["size"], case_keywords(case)
    image0, image1 = noise_pair(H, W, seed=H*W) if case["noise"] else piecewise_pair(image, H, W, case["disparity_min"])
    expected = chk.stereo_matching_sgm(image0, image1, **kw)
    if case["noise"] and case["uniqueness_ratio"] > 0 and H*W > 100:
        assert (expected == 16*(case["disparity_min"] - 1)).mean() > 0.5        # (nearly every pixel fails uniqueness)
    assert_same(amd.stereo_matching_sgm(image0, image1, **kw), expected)


@pytest.mark.gpu
@pytest.mark.parametrize("disparity_min", (-20, 0, 5))
@pytest.mark.parametrize("paths", (4, 8))
def test_ties_go_to_the_first_minimum(amd, disparity_min, paths):
    """Two constant images: every census word is 0, C is 0 where x - d is inside the image and 62 elsewhere. With
    disparity_min >= 0 the index 0 is inside wherever any is, S(p,.) is least and flat from i = 0 on, and the first
    minimum is i* = 0: 16 disparity_min where x - disparity_min is inside, invalid elsewhere. With disparity_min < 0 that
    does not follow from the definition: at the right edge the small indices are outside, their cost of 62 reaches the
    other columns along the paths, and i* is not 0 (the checker and the plain loops agree on that); that case is held
    to the checker alone"""
    kw = dict(disparity_min=disparity_min, disparity_max=disparity_min + 48, paths=paths)
    image0, image1 = np.full((20, 70), 7, dtype=np.uint8), np.full((20, 70), 200, dtype=np.uint8)
    d = amd.stereo_matching_sgm(image0, image1, **kw)
    if disparity_min >= 0:
        x = np.arange(70)
        inside = (x - disparity_min >= 0) & (x - disparity_min < 70)
        assert_same(d, np.broadcast_to(np.where(inside, 16*disparity_min, 16*(disparity_min - 1)).astype(np.int16), (20, 70)))
    assert_same(d, chk.stereo_matching_sgm(image0, image1, **kw))
    # period 4 in x: a minimum every 4 disparities
    rng = np.random.default_rng(4)
    periodic = np.tile(rng.integers(0, 256, size=(20, 4), dtype=np.uint8), (1, 18))[:, :70]
    for ratio in (0, 10):
        assert_same(amd.stereo_matching_sgm(periodic, periodic, uniqueness_ratio=ratio, **kw),
                    chk.stereo_matching_sgm(periodic, periodic, uniqueness_ratio=ratio, **kw))


@pytest.mark.gpu
def test_the_subpixel_division_is_a_floor(amd, image):
    """the case has pixels whose numerator (a - c) 16 + den is negative and no multiple of 2 den: a truncating
    division gives another value there"""
    image0, image1, _ = slanted_pair(image)
    expected, inter = chk.stereo_matching_sgm(image0, image1, disparity_max=32, intermediates=True)
    met = inter["valid"] & inter["inner"] & (inter["numerator"] < 0) & (inter["numerator"] % (2*inter["den"]) != 0)
    print(f"{met.sum()} of {met.size} pixels have a negative numerator that the floor rounds down")
    assert met.sum() > 100
    assert_same(amd.stereo_matching_sgm(image0, image1, disparity_max=32), expected)


@pytest.mark.gpu
def test_uint16(amd, image):
    image0, image1 = piecewise_pair(image, 40, 100, 0)
    kw = dict(disparity_max=32)
    d8 = amd.stereo_matching_sgm(image0, image1, **kw)
    # the same order of every pair of pixels: the same census, the same bits
    assert_same(amd.stereo_matching_sgm(image0.astype(np.uint16)*np.uint16(257), image1.astype(np.uint16)*np.uint16(257), **kw), d8)
    # the information in the low byte alone: the high bytes are constant
    low0, low1 = image0.astype(np.uint16) + np.uint16(0x4100), image1.astype(np.uint16) + np.uint16(0x4100)
    assert_same(amd.stereo_matching_sgm(low0, low1, **kw), d8)
    # ... and in both: what a uint8 cast would lose decides comparisons
    rng = np.random.default_rng(16)
    both0 = (image0.astype(np.uint16) >> 4 << 8) + rng.integers(0, 256, size=image0.shape).astype(np.uint16)
    both1 = np.ascontiguousarray(np.roll(both0, -5, axis=1))
    expected = chk.stereo_matching_sgm(both0, both1, **kw)
    assert not np.array_equal(expected, chk.stereo_matching_sgm((both0 >> 8).astype(np.uint8), (both1 >> 8).astype(np.uint8), **kw))
    assert_same(amd.stereo_matching_sgm(both0, both1, **kw), expected)


@pytest.mark.gpu
def test_the_resident_matcher(amd, image):
    live0 = amd.device_buffers_live()
    kw = dict(disparity_min=-4, disparity_max=28, paths=4)
    pairs = [piecewise_pair(image, 33, 70, -4), noise_pair(33, 70, seed=1), piecewise_pair(image[100:], 33, 70, 0)]
    one_shot = [amd.stereo_matching_sgm(a, b, **kw) for a, b in pairs]
    assert amd.device_buffers_live() == live0
    assert_same(one_shot[0], chk.stereo_matching_sgm(*pairs[0], **kw))
    assert_same(amd.stereo_matching_sgm(*pairs[0], **kw), one_shot[0])         # the same bits twice
    with amd.StereoMatcherSGM((33, 70), np.uint8, **kw) as matcher:
        assert amd.device_buffers_live() > live0
        with pytest.raises(Exception, match="no match has been made yet"):
            matcher.stage_milliseconds()
        for (a, b), expected in zip(pairs, one_shot):
            assert_same(matcher.match(a, b), expected)
        assert_same(matcher.match(*pairs[0]), one_shot[0])                      # nothing of the pairs before is left
        # out=: a dense array is filled in place, one that is not dense is filled too
        out = np.zeros((33, 70), dtype=np.int16)
        assert matcher.match(*pairs[1], out=out) is out
        assert_same(out, one_shot[1])
        wide = np.zeros((33, 140), dtype=np.int16)
        assert_same(matcher.match(*pairs[2], out=wide[:, ::2]), one_shot[2])
        assert_same(np.ascontiguousarray(wide[:, ::2]), one_shot[2])
        assert not wide[:, 1::2].any()
        # images that are not dense; a transposed view
        assert_same(matcher.match(np.asfortranarray(pairs[0][0]), pairs[0][1]), one_shot[0])
        with pytest.raises(Exception, match="'out' must be a numpy array of shape"):
            matcher.match(*pairs[0], out=np.zeros((33, 70), dtype=np.uint16))
        with pytest.raises(Exception, match="this matcher was made for images of shape"):
            matcher.match(pairs[0][0][:-1], pairs[0][1][:-1])
        with pytest.raises(Exception, match="this matcher was made for images of shape"):
            matcher.match(pairs[0][0].astype(np.uint16), pairs[0][1].astype(np.uint16))
        times = matcher.stage_milliseconds()
        assert set(times) == {"census", "paths", "select", "check"} and all(t >= 0 for t in times.values())
    assert amd.device_buffers_live() == live0
    with pytest.raises(Exception, match="has been closed"):
        matcher.match(*pairs[0])


def plane_scene(amd, image):
    """Two pinhole cameras look at the plane z = 0 of the reference frame, which carries the fixture as its texture:
    the construction of test_match_feature.py's plane, the cameras side by side"""
    D = 5.
    texture = amd.cameramodel(intrinsics=('LENSMODEL_PINHOLE', np.array((500., 500., 360.5, 240.5))), imagersize=(722, 482),
                              rt_cam_ref=np.array((0., 0., 0., 0., 0., D)))
    def camera(r, position, f):
        R = amd.R_from_r(np.array(r))
        return amd.cameramodel(intrinsics=('LENSMODEL_PINHOLE', np.array((f, f, 320., 230.))), imagersize=(640, 460),
                               rt_cam_ref=np.concatenate((r, -R @ np.array(position))))
    models = (camera((0.02, -0.03, 0.01), (-0.1, 0.02, -5.1), 560.), camera((-0.01, 0.02, -0.02), (0.1, -0.01, -5.0), 550.))
    images = [amd.transform_image(image, amd.image_transformation_map(texture, m, plane_n=np.array((0., 0., 1.)), plane_d=D))
              for m in models]
    return models, images


def plane_truth(amd, models_rectified):
    """per pixel of the rectified camera 0: the range to the plane z = 0 along the pixel's ray, the disparity, and the
    range formula restated (the law of sines for LATLON, z = baseline fx/disparity for PINHOLE)"""
    lensmodel, (fx, fy, cx, cy) = models_rectified[0].intrinsics()
    W, H = (int(n) for n in models_rectified[0].imagersize())
    Rt01 = amd.compose_Rt(models_rectified[0].Rt_cam_ref(), models_rectified[1].Rt_ref_cam())
    baseline = np.linalg.norm(Rt01[3])
    qx, qy = np.meshgrid(np.arange(W, dtype=float), np.arange(H, dtype=float))
    ux, uy = (qx - cx)/fx, (qy - cy)/fy
    latlon = lensmodel == 'LENSMODEL_LATLON'
    if latlon: v = np.stack((np.sin(ux), np.cos(ux)*np.sin(uy), np.cos(ux)*np.cos(uy)), axis=-1)
    else:      v = np.stack((ux, uy, np.ones_like(ux)), axis=-1)/np.sqrt(ux*ux + uy*uy + 1.)[..., None]
    Rt_ref_rect = models_rectified[0].Rt_ref_cam()
    vref, origin = v @ Rt_ref_rect[:3].T, Rt_ref_rect[3]
    range_true = -origin[2]/vref[..., 2]
    p1 = v*range_true[..., None] - np.array((baseline, 0., 0.))          # in the rectified camera 1
    if latlon: disparity_true = fx*(ux - np.arctan2(p1[..., 0], np.hypot(p1[..., 1], p1[..., 2])))
    else:      disparity_true = fx*(ux - p1[..., 0]/p1[..., 2])
    def range_of(disparity):
        parallax = disparity/fx
        if latlon: return baseline*np.cos(ux - parallax)/np.sin(parallax)
        return baseline/parallax*np.sqrt(ux*ux + uy*uy + 1.)
    assert np.allclose(range_of(disparity_true), range_true, rtol=1e-9, atol=0)
    return range_true, disparity_true, range_of


@pytest.mark.gpu
@pytest.mark.parametrize("rectification_model", ("LENSMODEL_LATLON", "LENSMODEL_PINHOLE"))
def test_image_pair_to_ranges(amd, image, rectification_model):
    """Rectification.disparity() is the checker applied to Rectification.rectify()'s images, to the bit, and
    Rectification.range() of it is the plane's range.

    The pixels that are held to the plane: those whose (checker's) disparity is valid and within 1/16 px, one step of
    the scale, of the true one. There the range may be off by what 1/16 px of disparity moves it: per pixel, the larger
    of |range_of(true disparity +- 1/16) - true range|, from the range formula restated in plane_truth(), relative to
    the true range, with a margin of 1e-6 of it for the kernel's own rounding in double. The range is monotonic in the
    disparity, so that is the bound. Measured on one MI355X, the largest relative error on the pixels held against the
    largest bound there: LATLON (160 x 96, disparities 21.1 .. 24.1 px) 0.00287 against 0.00290, 0.188 of the pixels held
    (0.854 valid); PINHOLE (161 x 97) 0.00286 against 0.00291, 0.210 held (0.872 valid). The errors come that close to
    the bound because the pixels held include some that are nearly 1/16 px off: the margin is per pixel, not in these
    maxima. The share held only has to show that the assertion is about something: a tenth"""
    models, images = plane_scene(amd, image)
    models_rectified = amd.rectified_system(models, az_fov_deg=16, el_fov_deg=9.6, pixels_per_deg_az=10, pixels_per_deg_el=10,
                                            rectification_model=rectification_model)
    W, H = (int(n) for n in models_rectified[0].imagersize())
    assert 140 <= W <= 180 and 85 <= H <= 110, (W, H)
    range_true, disparity_true, range_of = plane_truth(amd, models_rectified)
    lo = int(np.floor(disparity_true.min())) - 4
    kw = dict(disparity_min=lo, disparity_max=lo + 32)
    assert disparity_true.max() < lo + 28, (disparity_true.min(), disparity_true.max())
    live0 = amd.device_buffers_live()
    with amd.Rectification(models, models_rectified) as r:
        live1 = amd.device_buffers_live()
        rect0, rect1 = r.rectify(*images)
        expected = chk.stereo_matching_sgm(rect0, rect1, **kw)
        disparity = r.disparity(*images, **kw)
        assert_same(disparity, expected)
        assert_same(amd.stereo_matching_sgm(rect0, rect1, **kw), expected)
        assert amd.device_buffers_live() == live1
        ranges = r.range(disparity, disparity_scale=16, disparity_min=lo)
        assert np.array_equal(ranges, amd.stereo_range(disparity, models_rectified, disparity_scale=16, disparity_min=lo))
    assert amd.device_buffers_live() == live0
    valid = expected != 16*(lo - 1)
    # an invalid pixel is below the minimum: range 0
    assert np.all(ranges[~valid] == 0) and np.all(ranges[valid] > 0)
    held = valid & (np.abs(expected/16. - disparity_true) <= 1/16.)
    bound = np.maximum(np.abs(range_of(disparity_true - 1/16.) - range_true), np.abs(range_of(disparity_true + 1/16.) - range_true))/range_true + 1e-6
    err = np.abs(ranges - range_true)/range_true
    print(f"{rectification_model}: {W} x {H}, disparities {disparity_true.min():.2f}..{disparity_true.max():.2f} px, valid {valid.mean():.4f}, "
          f"held {held.mean():.4f}; largest relative range error there {err[held].max():.5f}, largest bound {bound[held].max():.5f}")
    assert held.mean() > 0.1            # (the assertion below is about something)
    assert np.all(err[held] <= bound[held])
