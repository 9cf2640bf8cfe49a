"""The anti-aliasing Gaussian pre-filter (include/mrcal_amd.h, "smoothing"), the part that needs no GPU: the two
restatements of the definition against each other, the taps of the library against the checker's, the plan of
csrc/smooth_plan.hpp under the host sanitizers, the sigma that 'auto' picks, and every refusal that is made before any
device work."""
import math

import numpy as np
import pytest

import hostbuild
import smooth_checker as chk

SIGMAS = (0.5, 0.87, 1.3, 1.936, 3.3, 5, 8)


def noise(shape, dtype, seed=0):
    return np.random.default_rng(seed).integers(0, np.iinfo(dtype).max + 1, size=shape).astype(dtype)


@pytest.mark.parametrize("dtype", (np.uint8, np.uint16), ids=lambda d: np.dtype(d).name)
def test_checker_against_the_loops(dtype):
    for shape, sigma in (((1, 1), 0.5), ((3, 5), 1.3), ((3, 5), 8), ((1, 30), (2, 0)), ((30, 1), (0, 2)), ((13, 17), 1.936),
                         ((13, 17), (0.5, 8)), ((9, 40), (3.3, 0.87))):
        image = noise(shape, dtype, seed=shape[0]*100 + shape[1])
        got = chk.smooth(image, sigma)
        assert got.dtype == image.dtype and np.array_equal(got, chk.smooth_loops(image, sigma)), (shape, sigma)


def test_what_the_definition_implies():
    # the numbers the definition's text quotes
    assert chk.weights(0) == [256] and chk.weights(0.5)[0] == 202
    for sigma in SIGMAS:
        w = chk.weights(sigma)
        assert len(w) == math.ceil(3*sigma) + 1 and w[0] + 2*sum(w[1:]) == 256 and min(w) >= 0 and max(w) <= 255
    w = chk.weights(5)
    assert any(w[k + 1] > w[k] for k in range(len(w) - 1))             # not monotone: eight bits are too coarse
    for dtype in (np.uint8, np.uint16):
        top = np.iinfo(dtype).max
        for value in (0, 1, 77, top - 1, top):                          # a constant image comes back unchanged
            c = np.full((7, 9), value, dtype=dtype)
            assert np.array_equal(chk.smooth(c, (0.5, 8)), c)
        image = noise((20, 31), dtype)
        assert np.array_equal(chk.smooth(image, (0, 2))[:, 5], chk.smooth(np.ascontiguousarray(image[:, 5:6]), (0, 2))[:, 0])
        assert np.array_equal(chk.smooth(image, (2, 0))[5], chk.smooth(np.ascontiguousarray(image[5:6]), (2, 0))[0])
        assert np.array_equal(chk.smooth(image, (2, 1.3)).T, chk.smooth(np.ascontiguousarray(image.T), (1.3, 2)))


@pytest.mark.parametrize("sigma", SIGMAS + (0,))
def test_the_librarys_taps(amd, sigma):
    w = amd.smooth_weights(sigma)
    assert w.dtype == np.int32 and w.tolist() == chk.weights(sigma)


def test_smooth_plan_under_the_host_sanitizers():
    """csrc/smooth_plan.hpp driven by a stand-alone program with its own main, built with ASan and UBSan: host code only"""
    hostbuild.assert_prints_ok("smooth_plan_check")


def decimating_map(shape, step):
    H, W = shape
    x, y = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    return np.ascontiguousarray(np.stack((x*step, y*step), axis=-1).astype(np.float32))


def test_antialias_sigma(amd):
    for step, expected in ((1, 0.0), (0.5, 0.0), (1.3, 0.0), (1.5, 0.5*math.sqrt(1.25)), (4, 0.5*math.sqrt(15)), (100, 8.0)):
        m = decimating_map((40, 50), step)
        assert chk.antialias_sigma(m) == pytest.approx(expected, abs=1e-12)
        assert amd.antialias_sigma(m) == chk.antialias_sigma(m)
    # the larger of the two directions; entries that are not finite are skipped; a map of one pixel has no step
    m = decimating_map((40, 50), 1)
    m[..., 1] *= 3
    assert amd.antialias_sigma(m) == chk.antialias_sigma(m) == pytest.approx(0.5*math.sqrt(8))
    m[::32] = np.nan
    m[5, 5] = np.inf
    assert amd.antialias_sigma(m) == chk.antialias_sigma(m) == pytest.approx(0.5*math.sqrt(8))
    m[:] = np.nan
    assert amd.antialias_sigma(m) == chk.antialias_sigma(m) == 0.0
    assert amd.antialias_sigma(decimating_map((1, 1), 4)) == chk.antialias_sigma(decimating_map((1, 1), 4)) == 0.0
    rng = np.random.default_rng(3)
    m = (decimating_map((67, 45), 2.5) + rng.normal(size=(67, 45, 2))).astype(np.float32)
    assert amd.antialias_sigma(m) == pytest.approx(chk.antialias_sigma(m), rel=1e-12) and chk.antialias_sigma(m) > 0.5


def test_refusals_before_any_device_work(amd, monkeypatch):
    a = np.zeros((20, 30), dtype=np.uint8)
    bgr = np.zeros((20, 30, 3), dtype=np.uint8)
    # (the taps are host code of the library: asked for before it is taken away)
    for bad in (-1, 8.01, float('nan'), float('inf')):
        with pytest.raises(Exception, match="^smooth\\(\\) failed:.*there are taps for sigma = 0 and for sigma > 0 with ceil\\(3 sigma\\) <= 24"):
            amd.smooth_weights(bad)
    with pytest.raises(Exception, match="^smooth\\(\\): 'sigma' must be a number"):
        amd.smooth_weights('2')

    def no_device(*a, **k): raise AssertionError("device work before the refusal")
    monkeypatch.setattr(amd._handle, "_libs", no_device)
    fake = amd.Rectification.__new__(amd.Rectification)
    fake.handle, fake._L, fake.Naz, fake.Nel = 1, None, 30, 20
    fake._models = fake._models_rectified = None
    mapxy = decimating_map((5, 7), 4)
    def smooth(image, antialias):    return amd.smooth_gaussian(image, antialias)
    def smoother(image, antialias):  return amd.ImageSmoother(image.shape, image.dtype, antialias)
    def transform(image, antialias): return amd.transform_image(image, mapxy, antialias=antialias)
    def rectify(image, antialias):   return fake.rectify(image, image, antialias=antialias)
    def disparity(image, antialias): return fake.disparity(image, image, disparity_max=16, antialias=antialias)
    def cloud(image, antialias):     return fake.point_cloud_of_images(image, image, disparity_max=16, antialias=antialias)
    every_way_in = (smooth, smoother, transform, rectify, disparity, cloud)
    for call in every_way_in:
        for bad, got in ((0.49, "\\(0.49,0.49\\)"), (8.01, "\\(8.01,8.01\\)"), (-1, "\\(-1,-1\\)"), (float('nan'), "\\(nan,nan\\)"),
                         ((2, 9), "\\(2,9\\)"), ((0.3, 0), "\\(0.3,0\\)")):
            with pytest.raises(Exception, match="^smooth\\(\\): a sigma is 0 \\(that axis is not filtered\\) or lies in \\[0.5, 8\\]. Got " + got):
                call(a, bad)
        for bad in ((2,), (2, 2, 2), (2, '2'), True, [None, 2]):
            with pytest.raises(Exception, match="^smooth\\(\\): '(sigma|antialias)' must be a number or \\(sigma_x, sigma_y\\)"):
                call(a, bad)
    for call in (smooth, smoother):
        for bad in (0, (0, 0), 0.0):
            with pytest.raises(Exception, match="^smooth\\(\\): both sigmas are 0: there is nothing to run"):
                call(a, bad)
    for call in (transform, rectify, disparity, cloud):
        with pytest.raises(Exception, match="^smooth\\(\\): antialias must be None, 'auto', a sigma or \\(sigma_x, sigma_y\\), not 'gaussian'"):
            call(a, 'gaussian')
    # the images: grey, uint8 or uint16
    with pytest.raises(Exception, match="^smooth\\(\\): 'image' must be a grayscale image of shape \\(H,W\\), got \\(20, 30, 3\\): an image that is filtered is grey"):
        amd.smooth_gaussian(bgr, 2)
    with pytest.raises(Exception, match="^smooth\\(\\): 'image' must be a grayscale image of shape \\(H,W\\), got \\(20, 30, 3\\): an image that is filtered is grey"):
        transform(bgr, 2)
    with pytest.raises(Exception, match="^smooth\\(\\): 'image0' must be a grayscale image of shape \\(H,W\\), got \\(20, 30, 3\\): an image that is filtered is grey"):
        rectify(bgr, (2, 0))
    for bad in (a.astype(np.float32), a.astype(np.int16)):
        with pytest.raises(Exception, match="^smooth\\(\\): 'image' must have dtype uint8 or uint16, not"):
            amd.smooth_gaussian(bad, 2)
    with pytest.raises(Exception, match="^smooth\\(\\): 'image' must have dtype uint8 or uint16, not float32"):
        transform(a.astype(np.float32), 2)
    with pytest.raises(Exception, match="^smooth\\(\\): 'image0' must have dtype uint8 or uint16, not float32"):
        rectify(a.astype(np.float32), 2)
    with pytest.raises(Exception, match="^smooth\\(\\): 'image' must be a numpy array"):
        amd.smooth_gaussian([[0]], 2)
    with pytest.raises(Exception, match="^smooth\\(\\): images of 30 x 0 pixels cannot be smoothed"):
        amd.smooth_gaussian(np.zeros((0, 30), dtype=np.uint8), 2)
    huge = np.lib.stride_tricks.as_strided(np.zeros((1,), dtype=np.uint8), shape=(1 << 14, (1 << 14) + 1), strides=(0, 0))
    with pytest.raises(Exception, match="^smooth\\(\\): images of 16385 x 16384 pixels cannot be smoothed"):
        amd.smooth_gaussian(huge, 2)
    for out in (np.zeros((20, 31), dtype=np.uint8), np.zeros((20, 30), dtype=np.uint16), [[0]]):
        with pytest.raises(Exception, match="^smooth\\(\\): 'out' must be a numpy array of shape \\(20, 30\\) and dtype uint8"):
            amd.smooth_gaussian(a, 2, out=out)
    # the resident form
    for shape in ((20, 30, 3), (20,), 5):
        with pytest.raises(Exception, match="^smooth\\(\\): shape must be \\(H,W\\)"):
            amd.ImageSmoother(shape, np.uint8, 2)
    for dtype in (np.float32, np.int16, None, "colour"):
        with pytest.raises(Exception, match="^smooth\\(\\): images are uint8 or uint16, not"):
            amd.ImageSmoother((20, 30), dtype, 2)
    s = amd.ImageSmoother.__new__(amd.ImageSmoother)
    s.handle, s.shape, s.dtype, s._L = 1, (20, 31), np.dtype(np.uint8), None
    with pytest.raises(Exception, match="^smooth\\(\\): this smoother was made for images of shape \\(20, 31\\) and dtype uint8, got \\(20, 30\\) and uint8"):
        s.apply(a)
    s.handle = None
    with pytest.raises(Exception, match="this ImageSmoother has been closed"):
        s.apply(a)
    with pytest.raises(Exception, match="this ImageSmoother has been closed"):
        s.milliseconds()
    # 'auto' on a map that does not shrink the image, 0 and None: nothing of the filter is asked for, whatever the image
    from mrcal_amd.smoothing import antialias_params
    for antialias in ('auto', 0, (0, 0), None):
        assert antialias_params(antialias, lambda: amd.antialias_sigma(decimating_map((5, 7), 1)), (bgr.astype(np.float32),)) is None
    p = antialias_params('auto', lambda: amd.antialias_sigma(mapxy), (a,))
    assert p.sigma_x == p.sigma_y == 0.5*math.sqrt(15)
    fake.handle = None
    # (what is in order goes on to the device)
    with pytest.raises(AssertionError, match="device work"):
        amd.smooth_gaussian(a, (0, 0.5))
    with pytest.raises(AssertionError, match="device work"):
        amd.ImageSmoother((20, 30), np.uint16, 8)
