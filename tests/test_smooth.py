"""The anti-aliasing Gaussian pre-filter on the GPU (csrc/smooth.hip): EQUAL to the checker (tests/smooth_checker.py) in
every pixel, alone and in front of the remaps that take the antialias keyword."""
import ctypes
import functools
import math

import numpy as np
import pytest

import smooth_checker as chk

DTYPES = (np.uint8, np.uint16)
# (H,W): one pixel, one row, one column, smaller than every radius (the clamps overlap from both sides), no multiple of
# any tile, several tiles down with halos across their edges, and one more than the issue's: wider than the 256 pixels
# of a uint8 tile, so that a halo crosses a tile's edge in x for that type too
SHAPES = ((1, 1), (1, 70), (70, 1), (3, 5), (35, 67), (70, 130), (9, 300))
SIGMAS = (0.5, 1.3, 1.936, 8, (0, 2), (2, 0), (0.5, 8))


def ids(x):
    return np.dtype(x).name if isinstance(x, type) else "x".join(str(n) for n in x)


@functools.lru_cache(maxsize=None)
def noise(shape, dtype):
    """uniform over the whole range: every pixel differs from its neighbours. Made once, not changed"""
    image = np.random.default_rng(shape[0]*1000 + shape[1]).integers(0, np.iinfo(dtype).max + 1, size=shape).astype(dtype)
    image.setflags(write=False)
    return image


def assert_same(got, expected):
    assert got.dtype == expected.dtype and got.shape == expected.shape, (got.dtype, got.shape, expected.dtype, expected.shape)
    if not np.array_equal(got, expected):
        bad = np.argwhere(got != expected)
        first = tuple(bad[0])
        raise AssertionError(f"{len(bad)} of {got.size} entries differ; the first at {first}: {got[first]} for {expected[first]}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_equals_the_checker(amd, shape, dtype):
    image = noise(shape, dtype)
    for sigma in SIGMAS:
        got = amd.smooth_gaussian(image, sigma)
        assert got is not image
        try:
            assert_same(got, chk.smooth(image, sigma))
        except AssertionError as e:
            raise AssertionError(f"sigma = {sigma}: {e}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_extreme_images(amd, dtype):
    top = np.iinfo(dtype).max
    shape = (70, 130)
    for sigma in (0.5, 1.936, 8, (0, 2), (2, 0)):
        # the accumulator's last bit: 65535 256 256 + 32768 = 2^32 - 32768
        full = np.full(shape, top, dtype=dtype)
        assert_same(amd.smooth_gaussian(full, sigma), full)
        for value in (0, 1, top//2):
            c = np.full((35, 67), value, dtype=dtype)
            assert_same(amd.smooth_gaussian(c, sigma), c)
        binary = (np.random.default_rng(5).integers(0, 2, size=shape)*top).astype(dtype)
        assert_same(amd.smooth_gaussian(binary, sigma), chk.smooth(binary, sigma))
    # one impulse in the middle: the taps themselves
    impulse = np.zeros(shape, dtype=dtype)
    impulse[35, 65] = 255
    for sigma in ((1.3, 1.936), (8, 0.5), (2, 0)):
        wx, wy = chk.weights(sigma[0]), chk.weights(sigma[1])
        expected = np.zeros(shape, dtype=dtype)
        for j in range(-(len(wy) - 1), len(wy)):
            for i in range(-(len(wx) - 1), len(wx)):
                expected[35 + j, 65 + i] = (255*wy[abs(j)]*wx[abs(i)] + 32768) >> 16
        assert_same(amd.smooth_gaussian(impulse, sigma), expected)


@pytest.mark.gpu
def test_behaviour(amd):
    live0 = amd.device_buffers_live()
    shape = (70, 130)
    for dtype in DTYPES:
        image, other = noise(shape, dtype), np.ascontiguousarray(noise(shape, dtype)[::-1, ::-1]//2)
        expected = chk.smooth(image, (1.3, 1.936))
        with amd.ImageSmoother(shape, dtype, (1.3, 1.936)) as s:
            assert amd.device_buffers_live() == live0 + 1               # ONE pooled allocation
            with pytest.raises(Exception, match="no image has been smoothed yet"):
                s.milliseconds()
            for im in (image, other, image):                            # (nothing of the call before is left)
                assert_same(s.apply(im), amd.smooth_gaussian(im, (1.3, 1.936)))
            assert_same(s.apply(image), expected)
            assert_same(s.apply(image), expected)                       # the same bits twice
            assert s.milliseconds() >= 0
            with pytest.raises(Exception, match="this smoother was made for images of shape"):
                s.apply(image[:-1])
        with pytest.raises(Exception, match="has been closed"):
            s.apply(image)
        # out=: the same as the returned array; one that is not dense; an image that is not dense
        out = np.zeros(shape, dtype=dtype)
        assert amd.smooth_gaussian(image, (1.3, 1.936), out=out) is out
        assert_same(out, expected)
        wide = np.zeros((shape[0], 2*shape[1]), dtype=dtype)
        assert_same(amd.smooth_gaussian(image, (1.3, 1.936), out=wide[:, ::2]), expected)
        assert not wide[:, 1::2].any()
        assert_same(amd.smooth_gaussian(np.asfortranarray(image), (1.3, 1.936)), expected)
    # what only the library can refuse: its message
    with pytest.raises(Exception, match="smooth\\(\\) failed:.*there are taps for sigma = 0"):
        amd.smooth_weights(9)
    assert amd.device_buffers_live() == live0


# ------------------------------------------------------------------------------------------ in front of a remap ---
SGM = dict(disparity_min=0, disparity_max=16)
SIGMA = (1.3, 0.87)


def stereo_scene(amd):
    """two pinhole cameras of 256 x 192 pixels side by side look at a plane with a noisy texture; rectified to half their
    resolution, which is what the filter is for"""
    D = 5.
    rng = np.random.default_rng(11)
    coarse = rng.integers(30, 226, size=(60, 80)).astype(np.uint8)
    texture_image = np.ascontiguousarray(np.kron(coarse, np.ones((4, 4), dtype=np.uint8)))       # (240, 320)
    texture = amd.cameramodel(intrinsics=('LENSMODEL_PINHOLE', np.array((250., 250., 159.5, 119.5))), imagersize=(320, 240),
                              rt_cam_ref=np.array((0., 0., 0., 0., 0., D)))
    def camera(r, position, f):
        R = amd.R_from_r(np.array(r))
        return amd.cameramodel(intrinsics=('LENSMODEL_PINHOLE', np.array((f, f, 128., 96.))), imagersize=(256, 192),
                               rt_cam_ref=np.concatenate((r, -R @ np.array(position))))
    models = (camera((0.02, -0.03, 0.01), (-0.1, 0.02, -5.1), 224.), camera((-0.01, 0.02, -0.02), (0.1, -0.01, -5.0), 220.))
    images = [amd.transform_image(texture_image, amd.image_transformation_map(texture, m, plane_n=np.array((0., 0., 1.)), plane_d=D))
              for m in models]
    models_rectified = amd.rectified_system(models, az_fov_deg=40, el_fov_deg=30, pixels_per_deg_az=2, pixels_per_deg_el=2)
    return models, models_rectified, images


@pytest.mark.gpu
def test_the_rectification_filters_on_the_device(amd):
    live0 = amd.device_buffers_live()
    models, models_rectified, images = stereo_scene(amd)
    assert images[0].shape == (192, 256) and images[0].dtype == np.uint8
    filtered = [chk.smooth(i, SIGMA) for i in images]
    assert (filtered[0] != images[0]).mean() > 0.5
    images16 = [i.astype(np.uint16)*257 for i in images]
    with amd.Rectification(models, models_rectified) as r:
        plain = r.rectify(*images)
        plain_disparity = r.disparity(*images, **SGM)
        plain_cloud = r.point_cloud_of_images(*images, dtype=np.float32, **SGM)
        # rectify()
        for got, expected in zip(r.rectify(*images, antialias=SIGMA), r.rectify(*filtered)):
            assert_same(got, expected)
        assert (r.rectify(*images, antialias=SIGMA)[0] != plain[0]).any()
        for got, expected in zip(r.rectify(*images16, antialias=2), r.rectify(*[chk.smooth(i, 2) for i in images16])):
            assert_same(got, expected)
        # ... with an equalization in front: equalize, filter, rectify
        clahe = [chk.smooth(amd.equalize_clahe(i), SIGMA) for i in images]
        for got, expected in zip(r.rectify(*images, equalization='clahe', antialias=SIGMA), r.rectify(*clahe)):
            assert_same(got, expected)
        stretched = [chk.smooth(amd.equalize_stretch(i), SIGMA) for i in images16]
        for got, expected in zip(r.rectify(*images16, equalization='stretch', antialias=SIGMA), r.rectify(*stretched)):
            assert_same(got, expected)
            assert got.dtype == np.uint8
        # disparity(): stereo_matching_sgm() of the filtered-then-rectified images
        expected = amd.stereo_matching_sgm(*r.rectify(*filtered), **SGM)
        assert (expected != plain_disparity).any() and (expected > 0).any()
        assert_same(r.disparity(*images, antialias=SIGMA, **SGM), expected)
        assert_same(r.disparity(*images, equalization='clahe', antialias=SIGMA, speckle_window_size=50, speckle_range=2, **SGM),
                    r.disparity(*clahe, speckle_window_size=50, speckle_range=2, **SGM))
        # point_cloud_of_images(): the colours are NOT filtered: image0's as it was before the filter
        got = r.point_cloud_of_images(*images, antialias=SIGMA, dtype=np.float32, **SGM)
        for g, e in zip(got, r.point_cloud_of_images(*filtered, color_image=images[0], dtype=np.float32, **SGM)):
            assert_same(g, e)
        assert len(got[0]) > 100
        got = r.point_cloud_of_images(*images, equalization='clahe', antialias=SIGMA, dtype=np.float32, **SGM)
        for g, e in zip(got, r.point_cloud_of_images(*clahe, color_image=amd.equalize_clahe(images[0]), dtype=np.float32, **SGM)):
            assert_same(g, e)
        # 'auto': the larger of the two maps' sigmas, which is not 0 here
        maps = r.maps()
        auto = max(chk.antialias_sigma(maps[0]), chk.antialias_sigma(maps[1]))
        assert 0.5 <= auto <= 2 and r._antialias_auto() == pytest.approx(auto, rel=1e-12)
        for got, expected in zip(r.rectify(*images, antialias='auto'), r.rectify(*[chk.smooth(i, r._antialias_auto()) for i in images])):
            assert_same(got, expected)
        # a colour image is refused
        bgr = np.ascontiguousarray(np.stack((images[0],)*3, axis=-1))
        with pytest.raises(Exception, match="an image that is filtered is grey"):
            r.rectify(bgr, bgr, antialias=SIGMA)
        # None: the bits of the call without the keyword, after everything above too
        for got, expected in zip(r.rectify(*images, antialias=None), plain):
            assert_same(got, expected)
        for got, expected in zip(r.rectify(*images), plain):
            assert_same(got, expected)
        assert_same(r.disparity(*images, antialias=None, **SGM), plain_disparity)
        assert_same(r.disparity(*images, **SGM), plain_disparity)
        for g, e in zip(r.point_cloud_of_images(*images, dtype=np.float32, **SGM), plain_cloud):
            assert_same(g, e)
    assert amd.device_buffers_live() == live0


def decimating_map(shape, step):
    H, W = shape
    x, y = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    return np.ascontiguousarray(np.stack((x*step, y*step), axis=-1).astype(np.float32))


@pytest.mark.gpu
def test_transform_image_filters_on_the_device(amd):
    live0 = amd.device_buffers_live()
    for dtype in DTYPES:
        image = noise((70, 130), dtype)
        mapxy = (decimating_map((20, 40), 3) + np.float32(0.37)).astype(np.float32)
        plain = amd.transform_image(image, mapxy)
        assert_same(amd.transform_image(image, mapxy, antialias=SIGMA), amd.transform_image(chk.smooth(image, SIGMA), mapxy))
        assert_same(amd.transform_image(image, mapxy, antialias=1.936, interpolation='nearest', borderMode='transparent'),
                    amd.transform_image(chk.smooth(image, 1.936), mapxy, interpolation='nearest', borderMode='transparent'))
        assert_same(amd.transform_image(image, mapxy, antialias=None), plain)
        assert_same(amd.transform_image(image, mapxy, antialias=0), plain)
        # 'auto': the checker's sigma of the map
        sigma = chk.antialias_sigma(mapxy)
        assert sigma == pytest.approx(0.5*math.sqrt(8), rel=1e-6)
        assert_same(amd.transform_image(image, mapxy, antialias='auto'), amd.transform_image(chk.smooth(image, amd.antialias_sigma(mapxy)), mapxy))
        assert amd.antialias_sigma(decimating_map((20, 40), 4)) == chk.antialias_sigma(decimating_map((20, 40), 4)) == 0.5*math.sqrt(15)
    # a map of scale 1 runs nothing, whatever the image: the bits of None
    m = amd.cameramodel(intrinsics=('LENSMODEL_PINHOLE', np.array((100., 100., 64.5, 34.5))), imagersize=(130, 70))
    identity = amd.image_transformation_map(m, m, intrinsics_only=True)
    assert amd.antialias_sigma(identity) == chk.antialias_sigma(identity) == 0.0
    for image in (noise((70, 130), np.uint8), np.stack((noise((70, 130), np.uint8),)*3, axis=-1), noise((70, 130), np.uint8).astype(np.float32)):
        assert_same(amd.transform_image(image, identity, antialias='auto'), amd.transform_image(image, identity))
    # a colour image, a float image
    bgr = np.ascontiguousarray(np.stack((noise((70, 130), np.uint8),)*3, axis=-1))
    with pytest.raises(Exception, match="an image that is filtered is grey"):
        amd.transform_image(bgr, decimating_map((20, 40), 3), antialias=2)
    # ... by the library too, whose callers may not have asked Python first
    from mrcal_amd._cabi import _ptr
    p, out, m = amd.smoothing._SmoothParams(2.0, 2.0), np.zeros((20, 40, 3), dtype=np.uint8), decimating_map((20, 40), 3)
    for image, channels, dtype, words in ((bgr, 3, 0, "smooth(): an image that is filtered is grey, not of 3 channels"),
                                          (noise((70, 130), np.uint8).astype(np.float32), 1, 2, "smooth(): images are uint8 or uint16")):
        assert not amd._lib.lib.mrcal_amd_transform_image_smoothed(_ptr(out), _ptr(image), 130, 70, channels, dtype, _ptr(m), 40, 20, 1, 0, None,
                                                                   ctypes.addressof(p))
        assert words in amd._api._last_error()
    assert amd.device_buffers_live() == live0


def stripes():
    """vertical stripes of a period of 2.5 pixels, and the pixels of a 4 x decimation whose filter window lies inside the
    image: nearer the border the replicated edge, which is not the stripes' continuation, is part of what is filtered"""
    H, W = 64, 256
    image = np.ascontiguousarray(np.broadcast_to(np.round(128 + 100*np.sin(2*np.pi*np.arange(W)/2.5)).astype(np.uint8), (H, W)))
    R = math.ceil(3*0.5*math.sqrt(15))
    inside = [i for i in range(W//4) if 4*i - R >= 0 and 4*i + R <= W - 1]
    return image, decimating_map((H//4, W//4), 4), inside


def span(a):
    return int(a.max()) - int(a.min())


def test_the_purpose_by_the_checker():
    """the two figures of the purpose test, on the CPU: what is asserted of the GPU below holds for the definition"""
    image, mapxy, inside = stripes()
    assert chk.antialias_sigma(mapxy) == 0.5*math.sqrt(15)
    print("unfiltered span:", span(image[::4, ::4][:, inside]))
    assert span(image[::4, ::4][:, inside]) > 100
    filtered = chk.smooth(image, 0.5*math.sqrt(15))[::4, ::4]
    print("filtered span:", span(filtered[:, inside]), "with the border's pixels:", span(filtered))
    assert span(filtered[:, inside]) <= 2


@pytest.mark.gpu
def test_the_purpose(amd):
    """Stripes of a period of 2.5 pixels, decimated 4 x: without the filter they alias into stripes of more than 100 grey
    levels; with 'auto' (sigma = 0.5 sqrt(15) = 1.936) at most 2 levels are left of them. The span is taken over the
    pixels whose filter window lies inside the image: with the two columns at the left border, where the replicated edge
    is filtered too, the checker's own span is 4 (127 .. 131)"""
    image, mapxy, inside = stripes()
    aliased = amd.transform_image(image, mapxy)
    smooth = amd.transform_image(image, mapxy, antialias='auto')
    print("unfiltered span:", span(aliased[:, inside]), "filtered span:", span(smooth[:, inside]), "with the border's pixels:", span(smooth))
    assert span(aliased[:, inside]) > 100
    assert span(smooth[:, inside]) <= 2
    assert_same(smooth, chk.smooth(image, 0.5*math.sqrt(15))[::4, ::4])
