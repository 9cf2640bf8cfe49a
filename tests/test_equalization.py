"""equalize_clahe(), equalize_stretch(), ImageEqualizer and the equalization keywords of Rectification and FeatureMatcher
(csrc/equalize.hip; the definition: include/mrcal_amd.h, "equalization").

Without a GPU: the vectorised checker (tests/equalize_checker.py) against its second transcription as plain loops on
every size, what the definition implies (no clipping is plain tile histogram equalization, a constant image, monotone
LUTs, one tile has nothing to interpolate), that the cases reach every path of the clipper, every refusal before any
device work, and the host planning (csrc/equalize_plan.hpp) as a stand-alone program under the host sanitizers.
On the GPU: EQUALITY with the checker, every pixel, no tolerance, and bit equality of every resident path with the
composed one. cv2 is no part of this project: nothing here is held to it."""
import functools
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR
import hostbuild
import equalize_checker as chk


# ((H,W), tiles): the smallest at which something can go wrong
CASES = (((8, 8), (8, 8)),          # tiles of one pixel, the clip limit held at 1
         ((16, 16), (8, 8)),        # divisible: no padding
         ((17, 16), (8, 8)),        # the divisible side gets a whole extra 8
         ((17, 23), (8, 8)),
         ((9, 64), (8, 8)),
         ((65, 130), (8, 8)),
         ((131, 257), (8, 8)),
         ((31, 47), (3, 5)))
# ... and two of few grey levels and ONE tile, so that a uint16 histogram too hands back more than it has bins
# (batch > 0) and to every bin (step == 1)
FEW_LEVELS = (((200, 300), (1, 1)), ((300, 301), (1, 1)))
CLIP_LIMITS = (2, 8, 40)
DTYPES = (np.uint8, np.uint16)
PATHS = ('clipped', 'step>1', 'step==1', 'batch')


@functools.lru_cache(maxsize=None)
def fixture_image():
    image = np.load(os.path.join(GOLDEN_DIR, "match_feature_image.npz"))["image"]
    image.setflags(write=False)
    return image


@functools.lru_cache(maxsize=None)
def crop(shape, dtype, few_levels=False):
    """the fixture's cut at (100,200); uint16: times 257 plus low-bit noise. Made once, not changed"""
    H, W = shape
    c = np.ascontiguousarray(fixture_image()[100:100 + H, 200:200 + W])
    if few_levels: c = c & 0xC0
    if np.dtype(dtype) == np.uint16:
        c = c.astype(np.uint16)*257
        if not few_levels: c += np.random.default_rng(H*1000 + W).integers(0, 4, size=c.shape, dtype=np.uint16)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def expected_clahe(shape, dtype, clip_limit, tiles, few_levels=False):
    e = chk.equalize_clahe(crop(shape, dtype, few_levels), clip_limit, tiles)
    e.setflags(write=False)
    return e


def case_id(case):
    (H, W), tiles = case
    return f"{H}x{W}-tiles{tiles[0]}x{tiles[1]}"


def all_cases():
    """(shape, tiles, dtype, clip_limit, few_levels)"""
    for dtype in DTYPES:
        for clip_limit in CLIP_LIMITS:
            for shape, tiles in CASES:      yield shape, tiles, dtype, clip_limit, False
        for shape, tiles in FEW_LEVELS:     yield shape, tiles, dtype, 8, True


# ------------------------------------------------------------------------------------------------ without a GPU ---
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("case", CASES + FEW_LEVELS[:1], ids=case_id)
def test_checker_against_the_loops(case, dtype):
    shape, tiles = case
    few = case in FEW_LEVELS
    # (the loops over 65536 bins a tile take 0.7 s a call: every size, but all three clip limits at the largest only)
    every_limit = not few and (dtype is np.uint8 or shape == (131, 257))
    for clip_limit in (CLIP_LIMITS if every_limit else (8,)):
        image = crop(shape, dtype, few)
        got = expected_clahe(shape, dtype, clip_limit, tiles, few)
        assert got.dtype == image.dtype and got.shape == image.shape
        assert np.array_equal(got, chk.equalize_clahe_loops(image, clip_limit, tiles)), (shape, tiles, clip_limit)
    assert np.array_equal(chk.equalize_stretch(image), chk.equalize_stretch_loops(image))


def test_the_cases_reach_every_path_of_the_clipper():
    """a condition, not a measurement: over the cases that are run, each of these happens in some tile, per dtype"""
    for dtype in DTYPES:
        counts = dict.fromkeys(PATHS, 0)
        for shape, tiles, dt, clip_limit, few in all_cases():
            if dt is not dtype: continue
            paths = chk.clahe_luts(crop(shape, dtype, few), clip_limit, tiles)[3]
            print(f"{np.dtype(dtype).name} {shape} tiles {tiles} clip_limit {clip_limit}: of {tiles[0]*tiles[1]} tiles {paths}")
            for k in PATHS: counts[k] += paths[k]
        print(f"{np.dtype(dtype).name}: in all {counts}")
        for k in PATHS:
            assert counts[k] > 0, (np.dtype(dtype).name, k)


def test_uniform_noise_would_prove_nothing():
    """why the cases are cuts of a real image: noise clips in no tile at mrcal's clip limit"""
    noise = np.random.default_rng(1).integers(0, 256, size=(131, 257), dtype=np.uint8)
    assert chk.clahe_luts(noise, 8, (8, 8))[3]['clipped'] == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_what_the_definition_implies(dtype):
    hist_size = chk.hist_size_of(dtype)
    for shape, tiles in CASES[1:]:
        image = crop(shape, dtype)
        # no clipping: the LUT is the tile's plain histogram equalization, computed another way (sorting)
        luts, tw, th, paths = chk.clahe_luts(image, 0, tiles)
        assert not any(paths.values())
        padded = chk.padded(image, tiles)[0]
        scale = np.float32(hist_size - 1)/np.float32(tw*th)
        for ty in range(tiles[1]):
            for tx in range(tiles[0]):
                values = np.sort(padded[ty*th:(ty + 1)*th, tx*tw:(tx + 1)*tw].ravel())
                cdf = np.searchsorted(values, np.arange(hist_size), side='right')            # pixels <= i
                plain = np.clip(np.rint(cdf.astype(np.float32)*scale), 0, hist_size - 1)
                assert np.array_equal(luts[ty, tx], plain.astype(dtype))
        # every LUT is monotone, clipped or not, and ends at the top of the range
        for clip_limit in (0,) + CLIP_LIMITS:
            luts = chk.clahe_luts(image, clip_limit, tiles)[0].astype(np.int64)
            assert (np.diff(luts, axis=-1) >= 0).all()
            assert (luts[..., -1] == hist_size - 1).all()
    # the padding: both sides, the divisible one by a whole 8, by reflection
    p, tw, th = chk.padded(crop((17, 16), dtype), (8, 8))
    assert p.shape == (24, 24) and (tw, th) == (3, 3)
    assert np.array_equal(p[:17, 16:], crop((17, 16), dtype)[:, 14:6:-1]) and np.array_equal(p[17:, :16], crop((17, 16), dtype)[15:8:-1])
    assert chk.padded(crop((16, 16), dtype), (8, 8))[0].shape == (16, 16)
    # a constant image maps to a constant; stretch: to zeros
    for value in (0, 7, hist_size - 1):
        c = np.full((17, 23), value, dtype=dtype)
        out = chk.equalize_clahe(c, 8, (8, 8))
        assert (out == out[0, 0]).all()
        assert not chk.equalize_stretch(c).any()
    # one tile: nothing to interpolate, the output is lut[v]
    for shape in ((16, 16), (31, 47)):
        image = crop(shape, dtype)
        for clip_limit in CLIP_LIMITS:
            luts = chk.clahe_luts(image, clip_limit, (1, 1))[0]
            assert np.array_equal(chk.equalize_clahe(image, clip_limit, (1, 1)), luts[0, 0][image])
    # stretch: the extremes go to 0 and 255, and the order is kept
    image = crop((65, 130), dtype)
    s = chk.equalize_stretch(image)
    assert s.dtype == np.uint8 and s[image == image.min()].max() == 0 and s[image == image.max()].min() == 255
    order = np.argsort(image.ravel(), kind='stable')
    assert (np.diff(s.ravel()[order].astype(int)) >= 0).all()
    # what cannot be padded by reflection, and tiles that are none
    with pytest.raises(Exception, match="too small"):
        chk.equalize_clahe(np.zeros((5, 3), dtype=dtype), 8, (8, 8))
    with pytest.raises(Exception, match="tiles must be at least"):
        chk.equalize_clahe(np.zeros((16, 16), dtype=dtype), 8, (0, 8))


def test_refusals_before_any_device_work(amd, monkeypatch):
    def no_device(*a, **k): raise AssertionError("device work before the refusal")
    monkeypatch.setattr(amd._handle, "_libs", no_device)
    a = np.zeros((20, 30), dtype=np.uint8)
    bgr = np.zeros((20, 30, 3), dtype=np.uint8)
    fake = amd.Rectification.__new__(amd.Rectification)
    fake.handle, fake._L, fake.Naz, fake.Nel = 1, None, 30, 20
    # every way in: (what is called with the keywords, the images it takes)
    def rectify(i0, i1, **kw):   return fake.rectify(i0, i1, **kw)
    def disparity(i0, i1, **kw): return fake.disparity(i0, i1, disparity_max=16, **kw)
    def matcher(i0, i1, **kw):   return amd.FeatureMatcher(i0, i1, **kw)
    def match(i0, i1, **kw):     return amd.match_feature(i0, i1, np.array((15., 10.)), q1_estimate=np.array((15., 10.)),
                                                          search_radius1=2, template_size1=3, **kw)
    for f in (amd.equalize_clahe, amd.equalize_stretch):
        with pytest.raises(Exception, match="^equalize\\(\\): 'image' must be a grayscale image of shape \\(H,W\\), got \\(20, 30, 3\\): convert a colour image first"):
            f(bgr)
        for bad in (a.astype(np.float32), a.astype(np.int16)):
            with pytest.raises(Exception, match="^equalize\\(\\): 'image' must have dtype uint8 or uint16, not"):
                f(bad)
        with pytest.raises(Exception, match="^equalize\\(\\): 'image' must be a numpy array"):
            f([[0]])
        with pytest.raises(Exception, match="^equalize\\(\\): images of 30 x 0 pixels cannot be equalized"):
            f(np.zeros((0, 30), dtype=np.uint8))
    huge = np.lib.stride_tricks.as_strided(np.zeros((1,), dtype=np.uint8), shape=(1 << 14, (1 << 14) + 1), strides=(0, 0))
    with pytest.raises(Exception, match="^equalize\\(\\): images of 16385 x 16384 pixels cannot be equalized"):
        amd.equalize_stretch(huge)
    for tiles in ((0, 8), (8, -1), (65, 64), (8,), 8, (8., 8), (True, 8)):
        with pytest.raises(Exception, match="^equalize\\(\\): tiles must be"):
            amd.equalize_clahe(a, tiles=tiles)
        with pytest.raises(Exception, match="^equalize\\(\\): tiles must be"):
            amd.ImageEqualizer((20, 30), np.uint8, tiles=tiles)
    with pytest.raises(Exception, match="^equalize\\(\\): tiles must be at least \\(1,1\\) and at most 4096 in all. Got \\(0,8\\)"):
        amd.equalize_clahe(a, tiles=(0, 8))
    with pytest.raises(Exception, match="^equalize\\(\\): an image of 3 x 5 pixels is too small for \\(8,8\\) tiles: it would be padded by \\(5,3\\) pixels, and a reflection reaches \\(2,4\\)"):
        amd.equalize_clahe(np.zeros((5, 3), dtype=np.uint8))
    for bad in (None, 'eight', np.nan, True):
        with pytest.raises(Exception, match="^equalize\\(\\): clip_limit must be a number"):
            amd.equalize_clahe(a, clip_limit=bad)
    for out in (np.zeros((20, 31), dtype=np.uint8), np.zeros((20, 30), dtype=np.uint16), [[0]]):
        with pytest.raises(Exception, match="^equalize\\(\\): 'out' must be a numpy array of shape \\(20, 30\\) and dtype uint8"):
            amd.equalize_clahe(a, out=out)
        with pytest.raises(Exception, match="^equalize\\(\\): 'out' must be a numpy array of shape \\(20, 30\\) and dtype uint8"):
            amd.equalize_stretch(a.astype(np.uint16), out=out)
    # the resident form
    for method in (None, 'CLAHE', 'fieldscale', 1):
        with pytest.raises(Exception, match="^equalize\\(\\): the method must be 'clahe' or 'stretch', not"):
            amd.ImageEqualizer((20, 30), np.uint8, method)
    for shape in ((20, 30, 3), (20,), 5):
        with pytest.raises(Exception, match="^equalize\\(\\): shape must be \\(H,W\\)"):
            amd.ImageEqualizer(shape, np.uint8)
    for dtype in (np.float32, np.int16, None, "colour"):
        with pytest.raises(Exception, match="^equalize\\(\\): images are uint8 or uint16, not"):
            amd.ImageEqualizer((20, 30), dtype)
    with pytest.raises(Exception, match="too small for \\(8,8\\) tiles"):
        amd.ImageEqualizer((5, 3), np.uint8)
    e = amd.ImageEqualizer.__new__(amd.ImageEqualizer)
    e.handle, e.shape, e.dtype, e.dtype_out, e._L = 1, (20, 31), np.dtype(np.uint8), np.dtype(np.uint8), None
    with pytest.raises(Exception, match="^equalize\\(\\): this equalizer was made for images of shape \\(20, 31\\) and dtype uint8, got \\(20, 30\\) and uint8"):
        e.apply(a)
    with pytest.raises(Exception, match="this equalizer was made for"):
        e.apply(np.zeros((20, 31), dtype=np.uint16))
    e.handle = None
    with pytest.raises(Exception, match="this ImageEqualizer has been closed"):
        e.apply(a)
    # the keywords, wherever they are taken
    for call in (rectify, disparity, matcher, match):
        with pytest.raises(Exception, match="^equalize\\(\\): the method must be None, 'clahe' or 'stretch', not 'fieldscale'"):
            call(a, a, equalization='fieldscale')
        with pytest.raises(Exception, match="^equalize\\(\\): tiles must be at least \\(1,1\\) and at most 4096 in all. Got \\(0,8\\)"):
            call(a, a, equalization='clahe', clahe_tiles=(0, 8))
        with pytest.raises(Exception, match="^equalize\\(\\): clip_limit must be a number"):
            call(a, a, equalization='clahe', clahe_clip_limit='8')
        with pytest.raises(Exception, match="too small for \\(64,64\\) tiles"):
            call(a, a, equalization='clahe', clahe_tiles=(64, 64))
    for call in (rectify, matcher, match):      # (float32 is theirs to take without the keyword)
        with pytest.raises(Exception, match="^equalize\\(\\): 'image0' must have dtype uint8 or uint16, not float32"):
            call(a.astype(np.float32), a.astype(np.float32), equalization='stretch')
    with pytest.raises(Exception, match="^equalize\\(\\): 'image0' must be a grayscale image of shape \\(H,W\\), got \\(20, 30, 3\\)"):
        rectify(bgr, bgr, equalization='clahe')
    with pytest.raises(Exception, match="^equalize\\(\\): 'image1' must be a grayscale image"):
        rectify(a, bgr, equalization='clahe')
    fake._models = fake._models_rectified = None
    with pytest.raises(Exception, match="^equalize\\(\\): the method must be None, 'clahe' or 'stretch', not 'histogram'"):
        fake.point_cloud_of_images(a, a, disparity_max=16, equalization='histogram')
    fake.handle = None
    # (what is in order goes on to the device)
    with pytest.raises(AssertionError, match="device work"):
        amd.equalize_clahe(a, clip_limit=-1, tiles=(3, 4))
    with pytest.raises(AssertionError, match="device work"):
        amd.equalize_stretch(a.astype(np.uint16))
    with pytest.raises(AssertionError, match="device work"):
        amd.FeatureMatcher(a, a, equalization='clahe', clahe_tiles=(2, 2))


def test_equalize_plan_under_the_host_sanitizers():
    """csrc/equalize_plan.hpp driven by a stand-alone program with its own main, built with ASan and UBSan"""
    hostbuild.assert_prints_ok("equalize_plan_check")


# --------------------------------------------------------------------------------------------------- on the GPU ---
def assert_same(got, expected):
    assert got.dtype == expected.dtype and got.shape == expected.shape, (got.dtype, got.shape, expected.dtype, expected.shape)
    if not np.array_equal(got, expected):
        bad = np.argwhere(got != expected)
        first = tuple(bad[0])
        raise AssertionError(f"{len(bad)} of {got.size} entries differ; the first at {first}: {got[first]} for {expected[first]}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("case", CASES + FEW_LEVELS, ids=case_id)
def test_equals_the_checker(amd, case, dtype):
    shape, tiles = case
    few = case in FEW_LEVELS
    image = crop(shape, dtype, few)
    for clip_limit in (CLIP_LIMITS if not few else (8,)):
        got = amd.equalize_clahe(image, clip_limit=clip_limit, tiles=tiles)
        assert got is not image
        assert_same(got, expected_clahe(shape, dtype, clip_limit, tiles, few))
    assert_same(amd.equalize_clahe(image, clip_limit=0, tiles=tiles), chk.equalize_clahe(image, 0, tiles))
    assert_same(amd.equalize_stretch(image), chk.equalize_stretch(image))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_the_full_fixture(amd, dtype):
    """(482,722): padded to (488,728), more than one workgroup of every kernel, a width that is no multiple of 4"""
    image = fixture_image() if dtype is np.uint8 else crop((482, 722), dtype)
    first = amd.equalize_clahe(image)                                   # mrcal's: clip_limit 8, 8 x 8 tiles
    assert_same(first, chk.equalize_clahe(image, 8.0, (8, 8)))
    assert (first != image).any()
    assert_same(amd.equalize_clahe(image), first)                       # the same bits twice
    stretched = amd.equalize_stretch(image)
    assert_same(stretched, chk.equalize_stretch(image))
    assert_same(amd.equalize_stretch(image), stretched)
    # (480,720): every row a whole number of 4-pixel groups, the wide loads and stores
    cut = np.ascontiguousarray(image[:480, :720])
    assert_same(amd.equalize_clahe(cut, clip_limit=3), chk.equalize_clahe(cut, 3, (8, 8)))
    # a constant image: CLAHE a constant, stretch zeros (the reference divides by zero)
    c = np.full((40, 52), 77, dtype=dtype)
    assert_same(amd.equalize_clahe(c), chk.equalize_clahe(c))
    assert not amd.equalize_stretch(c).any()
    # more tiles than the LDS holds LUTs for (uint8: 12 x 12 x 256 bytes > 32 KiB)
    assert_same(amd.equalize_clahe(image, tiles=(12, 12)), chk.equalize_clahe(image, 8.0, (12, 12)))


@pytest.mark.gpu
def test_the_resident_equalizer(amd):
    live0 = amd.device_buffers_live()
    shape = (131, 257)
    for dtype in DTYPES:
        image, other = crop(shape, dtype), np.ascontiguousarray(crop(shape, dtype)[::-1, ::-1]//2)
        with amd.ImageEqualizer(shape, dtype, 'clahe', clip_limit=2, tiles=(8, 8)) as e:
            assert amd.device_buffers_live() == live0 + 1               # ONE pooled allocation
            with pytest.raises(Exception, match="no image has been equalized yet"):
                e.stage_milliseconds()
            for im in (image, other, image):                            # (nothing of the call before is left)
                assert_same(e.apply(im), amd.equalize_clahe(im, clip_limit=2))
                assert_same(e.apply(im), chk.equalize_clahe(im, 2, (8, 8)))
            ms = e.stage_milliseconds()
            assert set(ms) == {"histogram", "lut", "apply"} and all(t >= 0 for t in ms.values())
            with pytest.raises(Exception, match="this equalizer was made for images of shape"):
                e.apply(image[:-1])
        with pytest.raises(Exception, match="has been closed"):
            e.apply(image)
        with amd.ImageEqualizer(shape, dtype, 'stretch') as e:
            for im in (image, other):
                assert_same(e.apply(im), chk.equalize_stretch(im))
            assert e.stage_milliseconds()["lut"] == 0
        # out=: the same as the returned array; one that is not dense; an image that is not dense
        out = np.zeros(shape, dtype=dtype)
        assert amd.equalize_clahe(image, out=out) is out
        assert_same(out, expected_clahe(shape, dtype, 8, (8, 8)))
        wide = np.zeros((shape[0], 2*shape[1]), dtype=np.uint8)
        assert_same(amd.equalize_stretch(image, out=wide[:, ::2]), chk.equalize_stretch(image))
        assert not wide[:, 1::2].any()
        assert_same(amd.equalize_clahe(np.asfortranarray(image)), expected_clahe(shape, dtype, 8, (8, 8)))
    assert amd.device_buffers_live() == live0


def plane_scene(amd):
    """two pinhole cameras side by side look at a plane that carries the fixture as its texture: test_stereo_sgm.py's
    scene, dimmed to a quarter of the range so that an equalization has something to do"""
    D = 5.
    image = fixture_image()
    texture = amd.cameramodel(intrinsics=('LENSMODEL_PINHOLE', np.array((500., 500., 360.5, 240.5))), imagersize=(722, 482),
                              rt_cam_ref=np.array((0., 0., 0., 0., 0., D)))
    def camera(r, position, f):
        R = amd.R_from_r(np.array(r))
        return amd.cameramodel(intrinsics=('LENSMODEL_PINHOLE', np.array((f, f, 320., 230.))), imagersize=(640, 460),
                               rt_cam_ref=np.concatenate((r, -R @ np.array(position))))
    models = (camera((0.02, -0.03, 0.01), (-0.1, 0.02, -5.1), 560.), camera((-0.01, 0.02, -0.02), (0.1, -0.01, -5.0), 550.))
    images = [amd.transform_image(image, amd.image_transformation_map(texture, m, plane_n=np.array((0., 0., 1.)), plane_d=D))//4 + 20
              for m in models]
    models_rectified = amd.rectified_system(models, az_fov_deg=16, el_fov_deg=9.6, pixels_per_deg_az=10, pixels_per_deg_el=10)
    return models, models_rectified, images


SGM = dict(disparity_min=8, disparity_max=40)


def assert_same_cloud(got, expected):
    assert len(got) == len(expected) == 3
    for g, e in zip(got, expected):
        assert_same(g, e)


@pytest.mark.gpu
def test_the_rectification_equalizes_on_the_device(amd):
    live0 = amd.device_buffers_live()
    models, models_rectified, images = plane_scene(amd)
    clahe = [amd.equalize_clahe(i) for i in images]
    other = [amd.equalize_clahe(i, clip_limit=3, tiles=(4, 6)) for i in images]
    images16 = [i.astype(np.uint16)*50 + 1000 for i in images]
    stretched = [amd.equalize_stretch(i) for i in images16]
    assert stretched[0].dtype == np.uint8 and (clahe[0] != images[0]).mean() > 0.5
    with amd.Rectification(models, models_rectified) as r:
        live1 = amd.device_buffers_live()
        plain = r.rectify(*images)
        plain_disparity = r.disparity(*images, **SGM)
        plain_cloud = r.point_cloud_of_images(*images, dtype=np.float32, **SGM)
        # rectify()
        for got, expected in zip(r.rectify(*images, equalization='clahe'), r.rectify(*clahe)):
            assert_same(got, expected)
            assert (got != plain[0]).any()
        for got, expected in zip(r.rectify(*images, equalization='clahe', clahe_clip_limit=3, clahe_tiles=(4, 6)), r.rectify(*other)):
            assert_same(got, expected)
        for got, expected in zip(r.rectify(*images16, equalization='stretch'), r.rectify(*stretched)):
            assert_same(got, expected)
            assert got.dtype == np.uint8
        # disparity(), with and without the speckle keywords
        expected = r.disparity(*clahe, **SGM)
        assert (expected != plain_disparity).any()
        assert_same(r.disparity(*images, equalization='clahe', **SGM), expected)
        speckle = dict(speckle_window_size=50, speckle_range=2)
        assert_same(r.disparity(*images, equalization='clahe', **speckle, **SGM), r.disparity(*clahe, **speckle, **SGM))
        assert_same(r.disparity(*images16, equalization='stretch', **SGM), r.disparity(*stretched, **SGM))
        # point_cloud_of_images(): the colours are the EQUALIZED image0's; a colour image that is given is used as it is
        got = r.point_cloud_of_images(*images, equalization='clahe', dtype=np.float32, **SGM)
        assert_same_cloud(got, r.point_cloud_of_images(*clahe, dtype=np.float32, **SGM))
        assert len(got[0]) > 1000 and got[1].dtype == np.uint8
        assert_same_cloud(r.point_cloud_of_images(*images, equalization='clahe', color_image=images[0], **speckle, **SGM),
                          r.point_cloud_of_images(*clahe, color_image=images[0], **speckle, **SGM))
        got = r.point_cloud_of_images(*images16, equalization='stretch', **SGM)
        assert_same_cloud(got, r.point_cloud_of_images(*stretched, **SGM))
        assert got[1].dtype == np.uint8
        got = r.point_cloud_of_images(*images16, equalization='stretch', color_image=images16[0], **SGM)
        assert_same_cloud(got, r.point_cloud_of_images(*stretched, color_image=images16[0], **SGM))
        assert got[1].dtype == np.uint16
        # None: the bits of the call without the keyword, after everything above too
        for got, expected in zip(r.rectify(*images, equalization=None), plain):
            assert_same(got, expected)
        assert_same(r.disparity(*images, equalization=None, **SGM), plain_disparity)
        assert_same(r.disparity(*images, **SGM), plain_disparity)
        assert_same_cloud(r.point_cloud_of_images(*images, equalization=None, dtype=np.float32, **SGM), plain_cloud)
        assert_same_cloud(r.point_cloud_of_images(*images, dtype=np.float32, **SGM), plain_cloud)
        assert amd.device_buffers_live() >= live1
    assert amd.device_buffers_live() == live0


@pytest.mark.gpu
def test_the_feature_matcher_equalizes_on_the_device(amd):
    live0 = amd.device_buffers_live()
    image = fixture_image()
    image0 = np.ascontiguousarray(image[40:340, 100:500])//4 + 20
    image1 = np.ascontiguousarray(image[47:347, 91:491])//4 + 20
    q0 = np.array(((200., 150.), (120.5, 80.25), (300., 220.)))
    kw = dict(q1_estimate=q0 + np.array((7., -5.)), search_radius1=12, template_size1=(21, 17))
    equalized = [amd.equalize_clahe(i) for i in (image0, image1)]
    with amd.FeatureMatcher(image0, image1, equalization='clahe') as m, amd.FeatureMatcher(*equalized) as composed, \
         amd.FeatureMatcher(image0, image1, equalization=None) as none, amd.FeatureMatcher(image0, image1) as plain:
        assert amd.device_buffers_live() == live0 + 8                   # two images each: nothing of the equalization is kept
        for method in (None, amd.TM_CCOEFF_NORMED, amd.TM_SQDIFF):
            got = m.match(q0, method=method, diagnostics=True, **kw)
            expected = composed.match(q0, method=method, diagnostics=True, **kw)
            assert np.array_equal(got[1], expected[1]) and (got[1] == 0).all()
            assert np.array_equal(got[0], expected[0])
            assert np.abs(got[0] - (q0 + np.array((9., -7.)))).max() < 1.     # (image1 is image0 moved by (9,-7); the tiles move with it)
            for g, e in zip(got[2], expected[2]):
                assert_same(g['matchoutput_image'], e['matchoutput_image'])
                assert_same(g['template'], e['template'])
            a, b = none.match(q0, method=method, **kw), plain.match(q0, method=method, **kw)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        unequalized = plain.match(q0, method=amd.TM_SQDIFF, diagnostics=True, **kw)
        assert (unequalized[2][0]['template'] != m.match(q0, method=amd.TM_SQDIFF, diagnostics=True, **kw)[2][0]['template']).any()
    # stretch of a uint16 pair: the templates are uint8
    pair16 = [i.astype(np.uint16)*50 + 1000 for i in (image0, image1)]
    with amd.FeatureMatcher(*pair16, equalization='stretch') as m, amd.FeatureMatcher(*[amd.equalize_stretch(i) for i in pair16]) as composed:
        got, expected = m.match(q0, diagnostics=True, **kw), composed.match(q0, diagnostics=True, **kw)
        assert np.array_equal(got[0], expected[0]) and np.array_equal(got[1], expected[1])
        assert got[2][0]['template'].dtype == np.uint8
        assert_same(got[2][0]['template'], expected[2][0]['template'])
    # the one-shot form
    q1, _ = amd.match_feature(image0, image1, q0[0], equalization='clahe', **dict(kw, q1_estimate=kw['q1_estimate'][0]))
    q1_composed, _ = amd.match_feature(*equalized, q0[0], **dict(kw, q1_estimate=kw['q1_estimate'][0]))
    assert np.array_equal(q1, q1_composed)
    assert amd.device_buffers_live() == live0
