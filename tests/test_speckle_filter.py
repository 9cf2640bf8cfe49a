"""filter_speckles(): the connected regions of similar disparity that are too small to be a surface become invalid.

Without a GPU: the checker (tests/speckle_checker.py: connected components of the grid graph) against cv2's flood
fill transcribed as plain loops, what the filter does to the checker's own SGM output where image1 has nothing to match,
every refusal before any device work, and the host planning (csrc/speckle_plan.hpp) as a stand-alone program under the
host sanitizers. On the GPU: EQUALITY with the checker, every pixel, no tolerance: random images over the sizes at
which a tile is just full or just not, structured images whose regions span every tile, the resident object, and the
filter as the last stage of stereo_matching_sgm(), StereoMatcherSGM and Rectification.disparity()."""
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR
import hostbuild
import speckle_checker as chk
import stereo_sgm_checker as sgm_chk


SIZES = ((7, 9), (8, 63), (9, 64), (10, 65), (64, 17), (65, 130))          # (H,W): the SGM tests' tile-edge list
GPU_SIZES = SIZES + ((130, 131), (35, 150))                                # ... and three tiles (64 x 16) each way, twice
PARAMS = ((3, 0, 4), (6, 1, 10), (40, 16, 25), (2, 0, 200))                # (levels, max_diff, max_speckle_size)
NEW_VALUE = -16


def random_image(H, W, levels):
    rng = np.random.default_rng(0)
    return (16*rng.integers(0, levels, size=(H, W)) - 16).astype(np.int16)


def case_id(case):
    (H, W), (levels, max_diff, max_size) = case
    return f"{H}x{W}-levels{levels}-diff{max_diff}-size{max_size}"


def noisy_half_pair(image, disparity_min=0):
    """image0: the 96 x 160 cut of the fixture at (180, 250); image1: the same cut seen disparity_min + 5 px further on,
    its right half uniform noise: nothing there matches"""
    image0 = np.ascontiguousarray(image[180:276, 250:410])
    image1 = np.ascontiguousarray(image[180:276, 255 + disparity_min:415 + disparity_min])
    image1[:, 80:] = np.random.default_rng(5).integers(0, 256, size=(96, 80), dtype=np.uint8)
    return image0, image1


SGM_KEYWORDS = dict(uniqueness_ratio=0, disp12_max_diff=-1)


@pytest.fixture(scope="module")
def image():
    return np.load(os.path.join(GOLDEN_DIR, "match_feature_image.npz"))["image"]


@pytest.fixture(scope="module")
def noisy_half(image):
    """per disparity_min: (image0, image1, the matcher's keywords, the checker's disparity image). Made once, not changed"""
    out = {}
    for disparity_min in (-3, 0):
        image0, image1 = noisy_half_pair(image, disparity_min)
        kw = dict(disparity_min=disparity_min, disparity_max=disparity_min + 32, **SGM_KEYWORDS)
        d = sgm_chk.stereo_matching_sgm(image0, image1, **kw)
        d.setflags(write=False)
        out[disparity_min] = (image0, image1, kw, d)
    return out


# ------------------------------------------------------------------------------------------------ without a GPU ---
@pytest.mark.parametrize("case", [(s, p) for s in SIZES for p in PARAMS], ids=case_id)
def test_checker_against_cv2s_loops(case):
    (H, W), (levels, max_diff, max_size) = case
    img = random_image(H, W, levels)
    before = img.copy()
    got = chk.filter_speckles(img, NEW_VALUE, max_size, max_diff)
    assert np.array_equal(img, before)                                  # (a new array)
    assert got.dtype == np.int16 and np.array_equal(got, chk.filter_speckles_loops(img, NEW_VALUE, max_size, max_diff))
    # nothing but small regions changes, and only to new_value
    changed = got != img
    assert np.all(got[changed] == NEW_VALUE)
    if (levels, max_diff, max_size) == (3, 0, 4):
        removed, kept = changed.mean(), (got != NEW_VALUE).mean()
        print(f"{H} x {W}: {removed:.2f} of the pixels removed, {kept:.2f} kept")
        assert removed > 0.1 and kept > 0.1                             # both kinds of pixel are there (measured: 0.35-0.49, 0.21-0.32)


def test_checker_on_the_definitions_edges():
    # max_speckle_size = 0 changes nothing; a pixel equal to new_value is never changed, and walls in mid-range
    img = random_image(20, 30, 5)
    assert np.array_equal(chk.filter_speckles(img, NEW_VALUE, 0, 100), img)
    assert np.array_equal(chk.filter_speckles(img, 16, 10**9, 65535) == 16, np.ones(img.shape, dtype=bool))
    # the difference in more than 16 bits
    ends = np.array([[-32768, 32767, -32768]], dtype=np.int16)
    assert np.array_equal(chk.filter_speckles(ends, 0, 2, 65534), np.zeros((1, 3), dtype=np.int16))
    assert np.array_equal(chk.filter_speckles(ends, 0, 2, 65535), ends)
    assert np.array_equal(chk.filter_speckles_loops(ends, 0, 2, 65534), np.zeros((1, 3), dtype=np.int16))
    assert np.array_equal(chk.filter_speckles_loops(ends, 0, 2, 65535), ends)


def test_the_filter_on_the_checkers_own_sgm_output(noisy_half):
    """measured: columns [0, 64) 1.000 valid before and after, and unchanged; columns [88, 160), where image1 is noise,
    from 1.000 valid to 0.178. The bounds: the textured part is one surface, which the filter must not touch; of the
    noise at least half must go"""
    image0, image1, kw, d = noisy_half[0]
    invalid = 16*(kw["disparity_min"] - 1)
    f = chk.filter_speckles(d, invalid, 50, 16)
    valid_before, valid_after = d != invalid, f != invalid
    print(f"columns [0,64): valid {valid_before[:, :64].mean():.3f} -> {valid_after[:, :64].mean():.3f}; "
          f"columns [88,160): {valid_before[:, 88:].mean():.3f} -> {valid_after[:, 88:].mean():.3f}")
    assert valid_before.all()                                           # (no uniqueness test, no left-right check)
    assert np.array_equal(f[:, :64], d[:, :64])
    assert valid_after[:, 88:].mean() < 0.5


def test_refusals_before_any_device_work(amd, monkeypatch):
    def no_device(*a, **k): raise AssertionError("device work before the refusal")
    monkeypatch.setattr(amd._handle, "_libs", no_device)
    a = np.zeros((20, 30), dtype=np.int16)
    kw = dict(new_value=-16, max_speckle_size=10, max_diff=16)
    flt = amd.filter_speckles
    with pytest.raises(TypeError, match="new_value"):
        flt(a)
    for bad in (a.astype(np.uint16), a.astype(np.float32), np.zeros((20, 30, 1), dtype=np.int16), np.zeros((20,), dtype=np.int16), [[0]]):
        with pytest.raises(Exception, match="^filter_speckles\\(\\): the disparity image must be a 2-D int16 array"):
            flt(bad, **kw)
    with pytest.raises(Exception, match="^filter_speckles\\(\\): images of 30 x 0 pixels cannot be filtered"):
        flt(np.zeros((0, 30), dtype=np.int16), **kw)
    # more than 2^28 pixels (a view: no memory behind it)
    huge = np.lib.stride_tricks.as_strided(np.zeros((1,), dtype=np.int16), shape=(1 << 14, (1 << 14) + 1), strides=(0, 0))
    with pytest.raises(Exception, match="^filter_speckles\\(\\): images of 16385 x 16384 pixels cannot be filtered"):
        flt(huge, **kw)
    for new_value in (-32769, 32768):
        with pytest.raises(Exception, match="^filter_speckles\\(\\): new_value must be in -32768..32767"):
            flt(a, **dict(kw, new_value=new_value))
    with pytest.raises(Exception, match="^filter_speckles\\(\\): new_value must be an integer"):
        flt(a, **dict(kw, new_value=1.))
    for name in ("max_speckle_size", "max_diff"):
        for bad in (-1, 2.5, 3., True, None):
            with pytest.raises(Exception, match=f"^filter_speckles\\(\\): {name} must be a non-negative integer"):
                flt(a, **dict(kw, **{name: bad}))
    for out in (np.zeros((20, 31), dtype=np.int16), np.zeros((20, 30), dtype=np.uint16), [[0]]):
        with pytest.raises(Exception, match="^filter_speckles\\(\\): 'out' must be a numpy array of shape \\(20, 30\\) and dtype int16"):
            flt(a, out=out, **kw)
    # the resident form: a shape that is none
    for shape in ((20, 30, 3), (20,), 5):
        with pytest.raises(Exception, match="^filter_speckles\\(\\): shape must be \\(H,W\\)"):
            amd.SpeckleFilter(shape)
    with pytest.raises(Exception, match="^filter_speckles\\(\\): images of 30 x 0 pixels cannot be filtered"):
        amd.SpeckleFilter((0, 30))
    with pytest.raises(Exception, match="^filter_speckles\\(\\): images of 32768 x 8193 pixels cannot be filtered"):
        amd.SpeckleFilter((8193, 1 << 15))
    # ... and one that is handed another shape (no device: the object is not initialised)
    f = amd.SpeckleFilter.__new__(amd.SpeckleFilter)
    f.handle, f.shape, f._L = 1, (20, 31), None
    with pytest.raises(Exception, match="^filter_speckles\\(\\): this filter was made for images of shape \\(20, 31\\), got \\(20, 30\\)"):
        f.filter(a, **kw)
    with pytest.raises(Exception, match="^filter_speckles\\(\\): max_diff must be a non-negative integer"):
        f.filter(np.zeros((20, 31), dtype=np.int16), **dict(kw, max_diff=-2))
    f.handle = None
    # the matcher's two keywords
    u8 = np.zeros((20, 30), dtype=np.uint8)
    for name in ("speckle_window_size", "speckle_range"):
        for bad in (-1, 1.5, 2.):
            with pytest.raises(Exception, match=f"^filter_speckles\\(\\): {name} must be a non-negative integer"):
                amd.stereo_matching_sgm(u8, u8, disparity_max=16, **{name: bad})
            with pytest.raises(Exception, match=f"^filter_speckles\\(\\): {name} must be a non-negative integer"):
                amd.StereoMatcherSGM((20, 30), np.uint8, disparity_max=16, **{name: bad})
    r = amd.Rectification.__new__(amd.Rectification)
    r.handle, r._L = 1, None
    with pytest.raises(Exception, match="^filter_speckles\\(\\): speckle_range must be a non-negative integer"):
        r.disparity(u8, u8, disparity_max=16, speckle_window_size=5, speckle_range=-1)
    r.handle = None
    # (what is in order goes on to the device: a max_diff above 65535 means 65535, and is no refusal)
    with pytest.raises(AssertionError, match="device work"):
        flt(a, new_value=-32768, max_speckle_size=0, max_diff=1 << 40)
    with pytest.raises(AssertionError, match="device work"):
        amd.stereo_matching_sgm(u8, u8, disparity_max=16, speckle_window_size=1 << 40, speckle_range=1 << 40)


def test_speckle_plan_under_the_host_sanitizers():
    """csrc/speckle_plan.hpp driven by a stand-alone program with its own main, built with ASan and UBSan"""
    hostbuild.assert_prints_ok("speckle_plan_check")


# --------------------------------------------------------------------------------------------------- on the GPU ---
def report_difference(got, expected):
    bad = np.argwhere(got != expected)
    return f"{len(bad)} of {got.size} pixels differ; the first at (y,x) = {tuple(bad[0])}: {got[tuple(bad[0])]} for {expected[tuple(bad[0])]}"


def assert_same(got, expected):
    assert got.dtype == np.int16 and got.shape == expected.shape
    assert np.array_equal(got, expected), report_difference(got, expected)


def assert_equals_the_checker(amd, img, new_value, max_size, max_diff):
    before = img.copy()
    got = amd.filter_speckles(img, new_value=new_value, max_speckle_size=max_size, max_diff=max_diff)
    assert got is not img and np.array_equal(img, before)
    expected = chk.filter_speckles(img, new_value, max_size, min(max_diff, 65535))
    assert_same(got, expected)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(s, p) for s in GPU_SIZES for p in PARAMS], ids=case_id)
def test_equals_the_checker(amd, case):
    """every pixel, no tolerance"""
    (H, W), (levels, max_diff, max_size) = case
    assert_equals_the_checker(amd, random_image(H, W, levels), NEW_VALUE, max_size, max_diff)


H0, W0 = 130, 131


def serpentine():
    """even rows, and a connector at alternate ends of the odd ones: ONE region that runs through every tile, 8580 pixels"""
    img = np.full((H0, W0), NEW_VALUE, dtype=np.int16)
    img[0::2] = 160
    img[1::4, -1] = 160
    img[3::4, 0] = 160
    assert (img == 160).sum() == 8580
    return img


@pytest.mark.gpu
def test_a_serpentine_is_one_region(amd):
    img = serpentine()
    assert_same(assert_equals_the_checker(amd, img, NEW_VALUE, 8579, 0), img)
    assert_same(assert_equals_the_checker(amd, img, NEW_VALUE, 8580, 0), np.full((H0, W0), NEW_VALUE, dtype=np.int16))
    # the same, upside down and mirrored: the root is at the other end of the path
    assert_same(assert_equals_the_checker(amd, np.ascontiguousarray(img[::-1, ::-1]), NEW_VALUE, 8579, 0), img[::-1, ::-1])
    # a cut in the middle: two regions, of 4294 and of 4285 pixels, the smaller one small enough
    cut = img.copy()
    cut[64, 70] = NEW_VALUE
    got = assert_equals_the_checker(amd, cut, NEW_VALUE, 4290, 0)
    assert (got == 160).any() and (got != cut).any()


@pytest.mark.gpu
def test_structured_images(amd):
    N = H0*W0
    # all one value: a single region over every tile
    flat = np.full((H0, W0), 7, dtype=np.int16)
    assert_same(assert_equals_the_checker(amd, flat, NEW_VALUE, N - 1, 0), flat)
    assert_same(assert_equals_the_checker(amd, flat, NEW_VALUE, N, 0), np.full((H0, W0), NEW_VALUE, dtype=np.int16))
    # all new_value: nothing takes part
    none = np.full((H0, W0), NEW_VALUE, dtype=np.int16)
    assert_same(assert_equals_the_checker(amd, none, NEW_VALUE, N, 65535), none)
    # a checkerboard of two values: all singletons
    yy, xx = np.mgrid[:H0, :W0]
    board = np.where((yy + xx) % 2 == 0, 100, 101).astype(np.int16)
    assert_same(assert_equals_the_checker(amd, board, NEW_VALUE, 0, 0), board)
    assert_same(assert_equals_the_checker(amd, board, NEW_VALUE, 1, 0), none)
    assert_same(assert_equals_the_checker(amd, board, NEW_VALUE, N - 1, 1), board)
    # a horizontal ramp in steps of exactly max_diff: one region; in steps of max_diff + 1: a region a column
    for max_diff in (0, 16):
        ramp = np.broadcast_to((np.arange(W0)*max_diff).astype(np.int16), (H0, W0)).copy()
        assert_same(assert_equals_the_checker(amd, ramp, -1, N - 1, max_diff), ramp)
        assert_same(assert_equals_the_checker(amd, ramp, -1, N, max_diff), np.full((H0, W0), -1, dtype=np.int16))
        steep = np.broadcast_to((np.arange(W0)*(max_diff + 1)).astype(np.int16), (H0, W0)).copy()
        assert_same(assert_equals_the_checker(amd, steep, -1, H0 - 1, max_diff), steep)
        assert_same(assert_equals_the_checker(amd, steep, -1, H0, max_diff), np.full((H0, W0), -1, dtype=np.int16))
        # ... and vertically
        assert_same(assert_equals_the_checker(amd, np.ascontiguousarray(steep[:, :H0].T), -1, H0 - 1, max_diff), steep[:, :H0].T)
    # -32768 against 32767: the difference is 65535, in more than 16 bits
    ends = np.where((yy + xx) % 2 == 0, -32768, 32767).astype(np.int16)
    assert_same(assert_equals_the_checker(amd, ends, 0, N - 1, 65534), np.zeros((H0, W0), dtype=np.int16))
    assert_same(assert_equals_the_checker(amd, ends, 0, N - 1, 65535), ends)
    assert_same(assert_equals_the_checker(amd, ends, 0, N - 1, 1 << 20), ends)         # (above 65535 means 65535)
    # new_value in the middle of the range: walls between pixels that could otherwise be joined
    rng = np.random.default_rng(3)
    walls = (16*rng.integers(0, 3, size=(H0, W0))).astype(np.int16)
    got = assert_equals_the_checker(amd, walls, 16, 30, 32)
    assert (got != walls).any() and (got != 16).any()
    assert not np.array_equal(got, chk.filter_speckles(walls, -1, 30, 32))
    # max_speckle_size = 0 returns the input
    img = random_image(H0, W0, 6)
    assert_same(assert_equals_the_checker(amd, img, NEW_VALUE, 0, 16), img)


@pytest.mark.gpu
def test_the_resident_filter(amd):
    live0 = amd.device_buffers_live()
    img = random_image(H0, W0, 6)
    kw = dict(new_value=NEW_VALUE, max_speckle_size=10, max_diff=16)
    first = amd.filter_speckles(img, **kw)
    assert amd.device_buffers_live() == live0
    assert_same(first, chk.filter_speckles(img, NEW_VALUE, 10, 16))
    assert (first != img).any()
    assert_same(amd.filter_speckles(img, **kw), first)                  # the same bits twice
    # out=: the same as the returned array; one that is not dense; in place
    out = np.zeros_like(img)
    assert amd.filter_speckles(img, out=out, **kw) is out
    assert_same(out, first)
    wide = np.zeros((H0, 2*W0), dtype=np.int16)
    assert_same(amd.filter_speckles(img, out=wide[:, ::2], **kw), first)
    assert not wide[:, 1::2].any()
    inplace = img.copy()
    assert amd.filter_speckles(inplace, out=inplace, **kw) is inplace
    assert_same(inplace, first)
    assert_same(amd.filter_speckles(np.asfortranarray(img), **kw), first)
    # one filter, other parameters every time: equal to fresh calls, and nothing of the call before is left
    others = [dict(new_value=NEW_VALUE, max_speckle_size=200, max_diff=0), dict(new_value=32, max_speckle_size=3, max_diff=65535),
              dict(new_value=NEW_VALUE, max_speckle_size=0, max_diff=16), kw]
    with amd.SpeckleFilter((H0, W0)) as f:
        assert amd.device_buffers_live() == live0 + 1                   # ONE pooled allocation
        for milliseconds in (f.milliseconds, f.pass_milliseconds):
            with pytest.raises(Exception, match="no image has been filtered yet"):
                milliseconds()
        for k in others:
            assert_same(f.filter(img, **k), amd.filter_speckles(img, **k))
            assert_same(f.filter(img, **k), chk.filter_speckles(img, k["new_value"], k["max_speckle_size"], k["max_diff"]))
        assert f.milliseconds() >= 0
        passes = f.pass_milliseconds()
        assert set(passes) == {"label", "merge", "count", "apply"} and all(t >= 0 for t in passes.values())
        with pytest.raises(Exception, match="this filter was made for images of shape"):
            f.filter(img[:-1], **kw)
    assert amd.device_buffers_live() == live0
    with pytest.raises(Exception, match="has been closed"):
        f.filter(img, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("disparity_min", (-3, 0))
def test_the_filter_inside_the_matcher(amd, noisy_half, disparity_min):
    image0, image1, kw, d = noisy_half[disparity_min]
    invalid = 16*(disparity_min - 1)
    expected = chk.filter_speckles(d, invalid, 50, 16)
    assert (expected != d).mean() > 0.1                                 # (the filter has something to do)
    live0 = amd.device_buffers_live()
    plain = amd.stereo_matching_sgm(image0, image1, **kw)
    assert_same(plain, d)
    # a window of 0 is the call without the keywords
    assert_same(amd.stereo_matching_sgm(image0, image1, speckle_window_size=0, speckle_range=7, **kw), plain)
    got = amd.stereo_matching_sgm(image0, image1, speckle_window_size=50, speckle_range=1, **kw)
    assert_same(got, expected)
    assert_same(amd.filter_speckles(plain, new_value=invalid, max_speckle_size=50, max_diff=16), expected)
    assert amd.device_buffers_live() == live0
    with amd.StereoMatcherSGM(image0.shape, image0.dtype, speckle_window_size=50, speckle_range=1, **kw) as matcher:
        live1 = amd.device_buffers_live()
        with pytest.raises(Exception, match="no match has been made yet"):
            matcher.speckle_milliseconds()
        assert_same(matcher.match(image0, image1), expected)
        assert_same(matcher.match(image0, image1), expected)            # (S, lent to the filter, is made anew)
        assert amd.device_buffers_live() == live1                       # the filter allocates nothing
        assert set(matcher.stage_milliseconds()) == {"census", "paths", "select", "check"}
        assert matcher.speckle_milliseconds() > 0
    with amd.StereoMatcherSGM(image0.shape, image0.dtype, **kw) as matcher:
        assert_same(matcher.match(image0, image1), plain)
        assert matcher.speckle_milliseconds() == 0
    assert amd.device_buffers_live() == live0


def plane_scene(amd, image):
    """two pinhole cameras side by side look at the plane z = 0 of the reference frame, which carries the fixture as its
    texture: test_stereo_sgm.py's scene"""
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


@pytest.mark.gpu
def test_the_filter_after_rectification(amd, image):
    models, images = plane_scene(amd, image)
    images[1] = images[1].copy()
    images[1][:, 320:] = np.random.default_rng(6).integers(0, 256, size=images[1][:, 320:].shape, dtype=np.uint8)
    models_rectified = amd.rectified_system(models, az_fov_deg=16, el_fov_deg=9.6, pixels_per_deg_az=10, pixels_per_deg_el=10)
    kw = dict(disparity_min=8, disparity_max=40, **SGM_KEYWORDS)
    with amd.Rectification(models, models_rectified) as r:
        plain = r.disparity(*images, **kw)
        assert_same(r.disparity(*images, speckle_window_size=0, **kw), plain)
        expected = amd.filter_speckles(plain, new_value=16*7, max_speckle_size=50, max_diff=32)
        assert_same(expected, chk.filter_speckles(plain, 16*7, 50, 32))
        assert (expected != plain).any()
        assert_same(r.disparity(*images, speckle_window_size=50, speckle_range=2, **kw), expected)
