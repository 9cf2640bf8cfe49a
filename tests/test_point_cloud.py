"""stereo_point_cloud(): the disparities of a rectified pair to a compacted, coloured cloud of points
(csrc/point_cloud.hip; the definition: include/mrcal_amd.h, "stereo_point_cloud"), Rectification.point_cloud() and
.point_cloud_of_images(), StereoPointCloud, and write_point_cloud_as_ply().

The checker (point_cloud_checker.py) restates the definition in numpy and again as per-pixel loops. index and color are
held to it entry for entry; points to 1e-12 relative of (range + |t|), the bound the range kernels are held to against
numpy (test_stereo.py), and for frame = 'rect0' to the BITS of the existing stereo_unproject()."""
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR
import hostbuild
import point_cloud_checker as chk

MODELS = ("LENSMODEL_LATLON", "LENSMODEL_PINHOLE")
GPU_SIZES = ((1, 1), (7, 9), (8, 63), (9, 64), (10, 65), (64, 17), (65, 130), (130, 131))       # (H,W)
SPAN = 1024                     # the pixels of a workgroup (csrc/point_cloud_plan.hpp: CLOUD_SPAN)
BASELINE = 0.31
SCALE, DMIN, DMAX = 16, 32, 8000
INVALID = -16                   # what a matcher with disparity_min = 0 marks an invalid pixel with
IMAGE_W, IMAGE_H = 37, 23       # of the colour image of the synthetic cases


def fxycxy_of(W, H):
    return np.array((220.3, 231.7, (W - 1)/2. + 0.3, (H - 1)/2. - 0.2))


def rectified_models(amd, rectification_model, W, H):
    """two rectified cameras BASELINE apart along the rectified x, turned and moved in the reference frame"""
    r, t0 = np.array((0.1, -0.2, 0.05)), np.array((0.3, 0.4, -0.2))
    return [amd.cameramodel(intrinsics=(rectification_model, fxycxy_of(W, H)), imagersize=(W, H),
                            rt_cam_ref=np.concatenate((r, t0 - np.array((x, 0., 0.))))) for x in (0., BASELINE)]


def valid_disparities(rng, H, W):
    """2 .. 56 px: every range is positive, for both models"""
    return rng.integers(DMIN, 900, size=(H, W)).astype(np.int16)


def patterns(H, W, seed):
    """(name, int16 disparity image): which pixels are kept, in every way the compaction can go wrong"""
    rng = np.random.default_rng(seed)
    valid = valid_disparities(rng, H, W)
    i = np.arange(H*W).reshape(H, W)
    y, x = np.divmod(i, W)
    def only(keep): return np.where(keep, valid, np.int16(INVALID)).astype(np.int16)
    kinds = np.array((0, 0, INVALID, DMIN - 1, DMAX + 1, -32768, 6720), dtype=np.int16)     # (6720 = 420 px: a negative LATLON range)
    mixed = np.where(i % 8 == 0, valid, kinds[i % 8 % len(kinds)]).astype(np.int16)
    mixed[i % 8 == 7] = DMIN                    # (the minimum itself is inside)
    return (("all", valid), ("none", only(i < 0)), ("first", only(i == 0)), ("last", only(i == H*W - 1)),
            ("checkerboard", only((x + y) % 2 == 0)), ("halves", only(rng.random((H, W)) < 0.5)),
            ("borders", only((i % SPAN >= SPAN - 40) | (i % SPAN < 24))), ("kinds", mixed))


def poked_map(H, W, seed):
    """a map into the IMAGE_W x IMAGE_H colour image: entries inside, outside, and at the first pixels every kind of
    entry the colour-pixel test has to decide"""
    rng = np.random.default_rng(seed)
    m = rng.uniform((-3., -3.), (IMAGE_W + 2., IMAGE_H + 2.), size=(H, W, 2)).astype(np.float32)
    f32, inside = np.float32, (5.25, 7.5)
    below = np.nextafter(f32(-0.5), f32(-1))
    pokes = [(np.nan, inside[1]), (inside[0], np.nan), (np.inf, inside[1]), (inside[0], -np.inf),
             (-0.5, inside[1]), (inside[0], -0.5), (below, inside[1]), (inside[0], below),                  # -0.5: pixel 0; just below: outside
             (IMAGE_W - 0.5, inside[1]), (inside[0], IMAGE_H - 0.5),                                        # rounds up to the size: outside
             (np.nextafter(f32(IMAGE_W - 0.5), f32(0)), inside[1]), (inside[0], np.nextafter(f32(IMAGE_H - 0.5), f32(0))),
             (-0.5, -0.5), (IMAGE_W - 1, IMAGE_H - 1), (3e9, 2.), (2., -3e9)]                                # (beyond int32)
    flat = m.reshape(-1, 2)
    for k, poke in enumerate(pokes):
        flat[(5*k) % (H*W)] = poke
    return m


def color_images(seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, size=(IMAGE_H, IMAGE_W), dtype=np.uint8), rng.integers(0, 256, size=(IMAGE_H, IMAGE_W, 3), dtype=np.uint8),
            rng.integers(0, 65536, size=(IMAGE_H, IMAGE_W), dtype=np.uint16), rng.integers(0, 65536, size=(IMAGE_H, IMAGE_W, 3), dtype=np.uint16))


# ------------------------------------------------------------------------------------------------ without a GPU ---
@pytest.mark.parametrize("rectification_model", MODELS)
@pytest.mark.parametrize("shape", ((7, 9), (8, 63)))
def test_checker_against_plain_loops(shape, rectification_model):
    H, W = shape
    fxycxy, map0 = fxycxy_of(W, H), poked_map(H, W, 3)
    Rt = np.array(((0.36, 0.48, -0.8), (-0.8, 0.6, 0.), (0.48, 0.64, 0.6), (0.1, -2., 3.)))
    for ipattern, (name, disparity) in enumerate(patterns(H, W, 5)):
        base = dict(disparity_scale=SCALE, disparity_scaled_min=DMIN, disparity_scaled_max=DMAX)
        ranges = chk.point_cloud(disparity, rectification_model, fxycxy, BASELINE, **base)[3]
        limits = dict()
        s = np.unique(ranges)
        if len(s) >= 4:             # between two ranges that occur: on neither
            limits = dict(range_min=(s[len(s)//4 - 1] + s[len(s)//4])/2., range_max=(s[-2] + s[-1])/2.)
        image0 = color_images(7)[ipattern % 4]
        for kw in (base, dict(base, **limits), dict(base, map0=map0, image0=image0), dict(base, map0=map0, image0=image0, Rt_out_rect0=Rt, **limits)):
            p, c, i, _ = chk.point_cloud(disparity, rectification_model, fxycxy, BASELINE, **kw)
            pl, cl, il = chk.point_cloud_loops(disparity, rectification_model, fxycxy, BASELINE, **kw)
            assert np.array_equal(i, il), (name, kw.keys())
            assert (c is None and cl is None) or (c.dtype == cl.dtype and c.shape == cl.shape and np.array_equal(c, cl)), name
            assert p.shape == pl.shape and np.allclose(p, pl, rtol=1e-13, atol=1e-13), name
        if name == "all":           # the cases are about something: colours drop some pixels, limits more
            n = [len(chk.point_cloud(disparity, rectification_model, fxycxy, BASELINE, **kw)[2])
                 for kw in (base, dict(base, **limits), dict(base, map0=map0, image0=image0))]
            assert n[0] == H*W and 0 < n[1] < n[0] and 0 < n[2] < n[0]


def test_checker_refuses_a_bound_on_a_range():
    H, W = 7, 9
    disparity = valid_disparities(np.random.default_rng(1), H, W)
    ranges = chk.point_cloud(disparity, MODELS[0], fxycxy_of(W, H), BASELINE, disparity_scale=SCALE)[3]
    with pytest.raises(AssertionError, match="is on the bound"):
        chk.point_cloud(disparity, MODELS[0], fxycxy_of(W, H), BASELINE, disparity_scale=SCALE, range_max=ranges[5]*(1 + 1e-10))


def test_refusals_before_any_device_work(amd, monkeypatch):
    models_rectified = rectified_models(amd, MODELS[0], 30, 20)
    models = [amd.cameramodel(intrinsics=('LENSMODEL_PINHOLE', np.array((500., 500., 31.5, 23.5))), imagersize=(64, 48),
                              rt_cam_ref=np.array((0., 0., 0., -x, 0., 0.))) for x in (0., BASELINE)]
    def no_device(*a, **k): raise AssertionError("device work before the refusal")
    monkeypatch.setattr(amd._handle, "_libs", no_device)
    d = np.full((20, 30), 160, dtype=np.int16)
    image = np.zeros((48, 64), dtype=np.uint8)
    cloud = amd.stereo_point_cloud
    for bad in ([[160]], d[0], d[:, :, None], d.astype(np.complex64), d.astype(bool)):
        with pytest.raises(Exception, match="^stereo_point_cloud\\(\\): the disparity must be a 2-D numeric numpy array"):
            cloud(bad, models_rectified)
    with pytest.raises(Exception, match="^stereo_point_cloud\\(\\): the disparity and the rectified images MUST have the same dimensions. I have disparity.shape=\\(20, 31\\)"):
        cloud(np.zeros((20, 31), dtype=np.int16), models_rectified)
    with pytest.raises(Exception, match="Must have received exactly two models"):
        cloud(d, models_rectified[:1])
    with pytest.raises(Exception, match="I need exactly 2 camera models"):
        cloud(d, models_rectified, models=models[:1])
    with pytest.raises(Exception, match="^stereo_point_cloud\\(\\): frame must be one of \\('ref', 'cam0', 'rect0'\\), not 'world'"):
        cloud(d, models_rectified, frame='world')
    with pytest.raises(Exception, match="^stereo_point_cloud\\(\\): frame='cam0' needs 'models'"):
        cloud(d, models_rectified, frame='cam0')
    with pytest.raises(Exception, match="^stereo_point_cloud\\(\\): 'image0' needs 'models'"):
        cloud(d, models_rectified, image0=image)
    for bad in (image.astype(np.float32), image.astype(np.int16), [[0]]):
        with pytest.raises(Exception, match="^stereo_point_cloud\\(\\): 'image0' must be a numpy array of dtype uint8 or uint16"):
            cloud(d, models_rectified, models=models, image0=bad)
    for bad in (np.zeros((48, 64, 2), dtype=np.uint8), np.zeros((48,), dtype=np.uint8), np.zeros((48, 64, 3, 1), dtype=np.uint8)):
        with pytest.raises(Exception, match="^stereo_point_cloud\\(\\): 'image0' must have shape \\(H,W\\) or \\(H,W,3\\)"):
            cloud(d, models_rectified, models=models, image0=bad)
    for bad in (np.zeros((48, 65), dtype=np.uint8), np.zeros((64, 48, 3), dtype=np.uint16)):
        with pytest.raises(Exception, match="^stereo_point_cloud\\(\\): 'image0' must have the imager size of camera 0, \\(H,W\\) = \\(48, 64\\)"):
            cloud(d, models_rectified, models=models, image0=bad)
    for bad in (np.float16, np.int32, "no dtype"):
        with pytest.raises(Exception, match="^stereo_point_cloud\\(\\): dtype must be float64 or float32"):
            cloud(d, models_rectified, dtype=bad)
    with pytest.raises(Exception, match="^stereo_point_cloud\\(\\): must have range_min <= range_max. Got 3 and 2"):
        cloud(d, models_rectified, range_min=3., range_max=2.)
    with pytest.raises(Exception, match="^stereo_point_cloud\\(\\): must have range_min <= range_max"):
        cloud(d, models_rectified, range_max=np.nan)
    with pytest.raises(Exception, match="^stereo_point_cloud\\(\\): must have disparity_scaled_max > disparity_scaled_min. Got 100 and 100"):
        cloud(d, models_rectified, disparity_scaled_min=100, disparity_scaled_max=100)
    with pytest.raises(Exception, match="disparity_min and disparity_scaled_min may not both be given"):
        cloud(d, models_rectified, disparity_min=1, disparity_scaled_min=2)
    # more than 2^28 pixels (a view: no memory behind it)
    big = [amd.cameramodel(intrinsics=(MODELS[0], fxycxy_of(30, 20)), imagersize=((1 << 14) + 1, 1 << 14),
                           rt_cam_ref=np.array((0., 0., 0., -x, 0., 0.))) for x in (0., BASELINE)]
    huge = np.lib.stride_tricks.as_strided(np.zeros((1,), dtype=np.int16), shape=(1 << 14, (1 << 14) + 1), strides=(0, 0))
    with pytest.raises(Exception, match="^stereo_point_cloud\\(\\): a disparity image of 16385 x 16384 pixels cannot be made a cloud of"):
        cloud(huge, big)
    with pytest.raises(Exception, match="^stereo_point_cloud\\(\\): a disparity image of 16385 x 16384 pixels cannot be made a cloud of"):
        amd.StereoPointCloud(big)
    with pytest.raises(Exception, match="^stereo_point_cloud\\(\\): map0 must be a float32 numpy array of shape \\(20, 30, 2\\)"):
        amd.StereoPointCloud(models_rectified, map0=np.zeros((20, 30, 2)))

    # the resident forms (no device: the objects are not initialised)
    r = amd.Rectification.__new__(amd.Rectification)
    r.handle, r._L, r._models, r._models_rectified, r.Naz, r.Nel = 1, None, models, models_rectified, 30, 20
    u8 = np.zeros((48, 64), dtype=np.uint8)
    with pytest.raises(Exception, match="^stereo_point_cloud\\(\\): disparity_min must not be negative: .* Got -3$"):
        r.point_cloud_of_images(u8, u8, disparity_min=-3, disparity_max=13)
    with pytest.raises(Exception, match="^stereo_matching_sgm\\(\\): disparity_max - disparity_min must be a positive multiple of 16"):
        r.point_cloud_of_images(u8, u8, disparity_max=17)
    with pytest.raises(Exception, match="^filter_speckles\\(\\): speckle_range must be a non-negative integer"):
        r.point_cloud_of_images(u8, u8, disparity_max=16, speckle_window_size=5, speckle_range=-1)
    with pytest.raises(Exception, match="^stereo_matching_sgm\\(\\) accepts ONLY grayscale images"):
        r.point_cloud_of_images(np.zeros((48, 64, 3), dtype=np.uint8), u8, disparity_max=16)
    with pytest.raises(Exception, match="^stereo_point_cloud\\(\\): 'color_image' must have the imager size of camera 0"):
        r.point_cloud_of_images(u8, u8, disparity_max=16, color_image=np.zeros((48, 63, 3), dtype=np.uint8))
    with pytest.raises(Exception, match="^stereo_point_cloud\\(\\): 'color_image' must be a numpy array of dtype uint8 or uint16"):
        r.point_cloud_of_images(u8, u8, disparity_max=16, color_image=np.zeros((48, 64, 3), dtype=np.float32))
    with pytest.raises(Exception, match="^stereo_point_cloud\\(\\): frame must be one of"):
        r.point_cloud_of_images(u8, u8, disparity_max=16, frame='rect1')
    with pytest.raises(Exception, match="^stereo_point_cloud\\(\\): 'image0' must have the imager size of camera 0"):
        r.point_cloud(d, image0=np.zeros((20, 30), dtype=np.uint8))
    with pytest.raises(Exception, match="^stereo_point_cloud\\(\\): frame must be one of"):
        r.point_cloud(d, frame=None)
    r.handle = None
    # ... and a closed Rectification
    with pytest.raises(Exception, match="this Rectification has been closed"):
        r.point_cloud(d)
    with pytest.raises(Exception, match="this Rectification has been closed"):
        r.point_cloud_of_images(u8, u8, disparity_max=16)
    with pytest.raises(Exception, match="this Rectification has been closed"):
        r.point_cloud_stage_milliseconds()
    c = amd.StereoPointCloud.__new__(amd.StereoPointCloud)
    c.handle, c._L, c._models_rectified, c.Naz, c.Nel, c._has_map = 1, None, models_rectified, 30, 20, False
    with pytest.raises(Exception, match="^stereo_point_cloud\\(\\): frame='cam0' needs 'models'"):
        c.point_cloud(d, frame='cam0')
    with pytest.raises(Exception, match="^stereo_point_cloud\\(\\): 'image0' needs the rectification map of camera 0"):
        c.point_cloud(d, image0=image)
    c.handle = None
    with pytest.raises(Exception, match="this StereoPointCloud has been closed"):
        c.point_cloud(d)
    # (what is in order goes on to the device)
    with pytest.raises(AssertionError, match="device work"):
        cloud(d, models_rectified, range_min=1., range_max=1., frame='rect0', dtype=np.float32)
    with pytest.raises(AssertionError, match="device work"):
        cloud(d, models_rectified, models=models, image0=image, frame='cam0')


def test_point_cloud_plan_under_the_host_sanitizers():
    """csrc/point_cloud_plan.hpp driven by a stand-alone program with its own main, built with ASan and UBSan"""
    hostbuild.assert_prints_ok("point_cloud_plan_check")


# ------------------------------------------------------------------------------------------------ the PLY writer ---
PLY_HEADER = "ply\nformat {} 1.0\nelement vertex {}\nproperty float x\nproperty float y\nproperty float z\n{}end_header\n"
PLY_GRAY, PLY_RGB = "property uchar intensity\n", "property uchar red\nproperty uchar green\nproperty uchar blue\n"


def ply_points(N, seed=2):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(N, 3))*100., rng.integers(0, 256, size=(N,), dtype=np.uint8), rng.integers(0, 256, size=(N, 3), dtype=np.uint8)


@pytest.mark.parametrize("N", (0, 1, 50))
def test_ply_binary_bytes(amd, tmp_path, N):
    points, gray, bgr = ply_points(N)
    f = str(tmp_path / "cloud.ply")
    def expect(color_header, dtype, fill):
        record = np.zeros((N,), dtype=dtype)
        record['xyz'] = points.astype(np.float32)
        fill(record)
        return PLY_HEADER.format("binary_little_endian", N, color_header).encode() + record.tobytes()
    want_plain = expect("", [('xyz', '<f4', 3)], lambda r: None)
    def fill_gray(r): r['i'] = gray
    want_gray  = expect(PLY_GRAY, [('xyz', '<f4', 3), ('i', 'u1')], fill_gray)
    def fill_rgb(r): r['rgb'] = bgr[:, ::-1]
    want_rgb   = expect(PLY_RGB, [('xyz', '<f4', 3), ('rgb', 'u1', 3)], fill_rgb)
    assert len(want_rgb) == len(PLY_HEADER.format("binary_little_endian", N, PLY_RGB)) + 15*N
    for kw, want in ((dict(), want_plain), (dict(color=gray), want_gray), (dict(color=bgr), want_rgb)):
        assert amd.write_point_cloud_as_ply(f, points, **kw) is None
        assert open(f, "rb").read() == want
        amd.write_point_cloud_as_ply(f, points.astype(np.float32), binary=True, **kw)
        assert open(f, "rb").read() == want
    # the colours in the trailing columns say the same
    amd.write_point_cloud_as_ply(f, np.concatenate((points, gray[:, None]), axis=1))
    assert open(f, "rb").read() == want_gray
    amd.write_point_cloud_as_ply(f, np.concatenate((points, bgr), axis=1))
    assert open(f, "rb").read() == want_rgb


@pytest.mark.parametrize("N", (0, 3, 50))
def test_ply_ascii_reads_back(amd, tmp_path, N):
    points, gray, bgr = ply_points(N, 4)
    f = str(tmp_path / "cloud.ply")
    for kw, color_header, columns in ((dict(), "", 3), (dict(color=gray), PLY_GRAY, 4), (dict(color=bgr), PLY_RGB, 6)):
        amd.write_point_cloud_as_ply(f, points, binary=False, **kw)
        text = open(f, "rb").read().decode()
        header = PLY_HEADER.format("ascii", N, color_header)
        assert text.startswith(header)
        rows = [line.split() for line in text[len(header):].splitlines()]
        # exactly the properties the header declares, a vertex a line
        assert len(rows) == N and all(len(row) == columns for row in rows)
        if N == 0: continue
        # %.9g: the float32 that the binary form holds survives
        assert np.array_equal(np.array([[float(v) for v in row[:3]] for row in rows]).astype(np.float32), points.astype(np.float32))
        got = np.array([[int(v) for v in row[3:]] for row in rows])
        if columns == 4: assert np.array_equal(got[:, 0], gray)
        if columns == 6: assert np.array_equal(got, bgr[:, ::-1])       # BGR in, red green blue out
    amd.write_point_cloud_as_ply(f, np.concatenate((points, bgr), axis=1), binary=False)
    assert open(f, "rb").read().decode() == text


def test_ply_refusals(amd, tmp_path):
    f = str(tmp_path / "cloud.ply")
    points, gray, bgr = ply_points(5)
    w = amd.write_point_cloud_as_ply
    with pytest.raises(Exception, match="^points.shape must be \\(N,3\\) or \\(N,4\\) or \\(N,6\\), but points.ndim=1$"):
        w(f, points[0])
    with pytest.raises(Exception, match="^points.shape\\[-1\\] must be one of \\(3,4,6\\) to indicate no-color or grayscale or bgr colors respectively. Instead got points.shape\\[-1\\] = 5$"):
        w(f, np.zeros((5, 5)))
    with pytest.raises(Exception, match="^Both 'points' and 'color' are specifying color information. At most one of those should provide it$"):
        w(f, np.zeros((5, 4)), color=gray)
    with pytest.raises(Exception, match="^color.shape must be \\(N,\\) or \\(N,3\\), but color.ndim=3$"):
        w(f, points, color=np.zeros((5, 3, 1), dtype=np.uint8))
    with pytest.raises(Exception, match="^Inconsistent point counts: len\\(points\\)=5 but len\\(color\\)=4$"):
        w(f, points, color=gray[:4])
    with pytest.raises(Exception, match="^color.shape must be \\(N,\\) or \\(N,3\\), but color.shape=\\(5, 2\\)$"):
        w(f, points, color=np.zeros((5, 2), dtype=np.uint8))
    # the departures: no truncation
    with pytest.raises(Exception, match="uint16 colours would be truncated"):
        w(f, points, color=gray.astype(np.uint16))
    with pytest.raises(Exception, match="must lie in 0..255"):
        w(f, np.concatenate((points, np.full((5, 1), 256.)), axis=1))
    assert not os.path.exists(f)


# --------------------------------------------------------------------------------------------------- on the GPU ---
def assert_cloud_equals_the_checker(got, want, Rt, what):
    """index and color: every entry. points: |dp| <= 1e-12 (range + |t|)"""
    points, color, index = got
    wpoints, wcolor, windex, wranges = want
    assert index.dtype == np.int32 and index.shape == windex.shape and np.array_equal(index, windex), what
    if wcolor is None: assert color is None, what
    else:              assert color.dtype == wcolor.dtype and color.shape == wcolor.shape and np.array_equal(color, wcolor), what
    assert points.shape == wpoints.shape, what
    t = 0. if Rt is None else np.linalg.norm(Rt[3])
    err = np.linalg.norm(points.astype(np.float64) - wpoints, axis=-1)
    assert np.all(err <= 1e-12*(wranges + t)), (what, err.max())


@pytest.mark.gpu
@pytest.mark.parametrize("rectification_model", MODELS)
@pytest.mark.parametrize("shape", GPU_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_equals_the_checker(amd, shape, rectification_model):
    """every size, every pattern, with and without colours (uint8 gray, uint8 BGR, uint16 gray, uint16 BGR in turn),
    through the stand-alone object and a test map with every kind of entry"""
    H, W = shape
    models_rectified = rectified_models(amd, rectification_model, W, H)
    fxycxy, map0, images = fxycxy_of(W, H), poked_map(H, W, 11), color_images(13)
    Rt = models_rectified[0].Rt_ref_cam()
    kw  = dict(disparity_scale=SCALE, disparity_scaled_min=DMIN, disparity_scaled_max=DMAX)
    live0 = amd.device_buffers_live()
    with amd.StereoPointCloud(models_rectified, map0=map0) as cloud:
        with pytest.raises(Exception, match="no cloud has been computed yet"):
            cloud.stage_milliseconds()
        for ipattern, (name, disparity) in enumerate(patterns(H, W, 17)):
            before = disparity.copy()
            want = chk.point_cloud(disparity, rectification_model, fxycxy, BASELINE, Rt_out_rect0=Rt, **kw)
            got = cloud.point_cloud(disparity, **kw)
            assert got[0].dtype == np.float64 and got[0].shape == (len(want[2]), 3) and got[1] is None
            assert_cloud_equals_the_checker(got, want, Rt, (name, "no colour"))
            if name == "all":   assert len(got[2]) == H*W
            if name == "none":  assert len(got[2]) == 0
            if name == "first": assert list(got[2]) == [0]
            if name == "last":  assert list(got[2]) == [H*W - 1]
            image0 = images[ipattern % 4]
            want = chk.point_cloud(disparity, rectification_model, fxycxy, BASELINE, Rt_out_rect0=Rt, map0=map0, image0=image0, **kw)
            got = cloud.point_cloud(disparity, image0=image0, **kw)
            assert got[1].dtype == image0.dtype and got[1].shape == (len(want[2]),) + image0.shape[2:]
            assert_cloud_equals_the_checker(got, want, Rt, (name, "colour"))
            assert np.array_equal(disparity, before)
        ms = cloud.stage_milliseconds()
        assert set(ms) == {"mask", "scan", "scatter"} and all(v >= 0 for v in ms.values())
    assert amd.device_buffers_live() == live0


@pytest.mark.gpu
def test_every_colour_type_meets_every_kind_of_map_entry(amd):
    """poked_map()'s pokes land on kept pixels of the "all" pattern: that the colour test decided each as the checker
    does is in test_equals_the_checker; here, that they are decided the way the definition says"""
    H, W = 10, 65
    models_rectified = rectified_models(amd, MODELS[0], W, H)
    map0 = poked_map(H, W, 11)
    disparity = patterns(H, W, 17)[0][1]
    with amd.StereoPointCloud(models_rectified, map0=map0) as cloud:
        for image0 in color_images(19):
            points, color, index = cloud.point_cloud(disparity, image0=image0, disparity_scale=SCALE)
            kept = np.zeros(H*W, dtype=bool)
            kept[index] = True
            # NaN, infinite, just below -0.5, rounding up to the size, beyond int32: dropped. -0.5, just below size - 0.5: kept
            assert not kept[[0, 5, 10, 15, 30, 35, 40, 45, 70, 75]].any()
            assert kept[[20, 25, 50, 55, 60, 65]].all()
            where = {int(i): k for k, i in enumerate(index)}
            # (the entry that is inside, (5.25, 7.5), is pixel (5, 8): a half rounds up)
            assert np.array_equal(color[where[20]], image0[8, 0]) and np.array_equal(color[where[25]], image0[0, 5])
            assert np.array_equal(color[where[60]], image0[0, 0]) and np.array_equal(color[where[65]], image0[IMAGE_H - 1, IMAGE_W - 1])
            assert np.array_equal(color[where[50]], image0[8, IMAGE_W - 1]) and np.array_equal(color[where[55]], image0[IMAGE_H - 1, 5])


@pytest.mark.gpu
@pytest.mark.parametrize("rectification_model", MODELS)
def test_range_limits(amd, rectification_model):
    H, W = 65, 130
    models_rectified = rectified_models(amd, rectification_model, W, H)
    fxycxy = fxycxy_of(W, H)
    disparity = patterns(H, W, 23)[7][1]
    kw = dict(disparity_scale=SCALE, disparity_scaled_min=DMIN, disparity_scaled_max=DMAX)
    s = np.unique(chk.point_cloud(disparity, rectification_model, fxycxy, BASELINE, **kw)[3])
    # between two ranges that occur, so that neither bound is within 1e-9 of a range (the checker asserts it)
    lo, hi = (s[len(s)//3 - 1] + s[len(s)//3])/2., (s[2*len(s)//3 - 1] + s[2*len(s)//3])/2.
    assert (s[len(s)//3] - s[len(s)//3 - 1]) > 1e-8*lo and (s[2*len(s)//3] - s[2*len(s)//3 - 1]) > 1e-8*hi
    counts = []
    for limits in (dict(range_min=lo), dict(range_max=hi), dict(range_min=lo, range_max=hi), dict(range_min=0., range_max=np.inf)):
        want = chk.point_cloud(disparity, rectification_model, fxycxy, BASELINE, **kw, **limits)
        got = amd.stereo_point_cloud(disparity, models_rectified, frame='rect0', **kw, **limits)
        assert_cloud_equals_the_checker(got, want, None, limits)
        counts.append(len(got[2]))
    assert 0 < counts[2] < counts[0] < counts[3] and counts[2] < counts[1] < counts[3]


@pytest.mark.gpu
@pytest.mark.parametrize("rectification_model", MODELS)
@pytest.mark.parametrize("shape", ((10, 65), (65, 130)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_rect0_points_are_the_bits_of_stereo_unproject(amd, shape, rectification_model):
    H, W = shape
    models_rectified = rectified_models(amd, rectification_model, W, H)
    for name, disparity in patterns(H, W, 29):
        points, color, index = amd.stereo_point_cloud(disparity, models_rectified, frame='rect0', disparity_scale=SCALE,
                                                      disparity_scaled_min=DMIN, disparity_scaled_max=DMAX)
        qrect0 = np.ascontiguousarray(np.stack(np.meshgrid(np.arange(W, dtype=float), np.arange(H, dtype=float)), axis=-1))
        dense = amd.stereo_unproject(disparity.astype(np.uint16).astype(float), models_rectified, disparity_scale=SCALE, qrect0=qrect0)
        assert points.dtype == np.float64 and dense.dtype == np.float64
        assert np.array_equal(points.view(np.uint64), dense.reshape(-1, 3)[index].view(np.uint64)), name
        # float32: the float64 points rounded once
        p32, _, i32 = amd.stereo_point_cloud(disparity, models_rectified, frame='rect0', dtype=np.float32, disparity_scale=SCALE,
                                             disparity_scaled_min=DMIN, disparity_scaled_max=DMAX)
        assert p32.dtype == np.float32 and np.array_equal(i32, index)
        assert np.array_equal(p32.view(np.uint32), points.astype(np.float32).view(np.uint32)), name
        # ... in the reference frame too
        p64 = amd.stereo_point_cloud(disparity, models_rectified, disparity_scale=SCALE, disparity_scaled_min=DMIN, disparity_scaled_max=DMAX)[0]
        p32 = amd.stereo_point_cloud(disparity, models_rectified, dtype=np.float32, disparity_scale=SCALE, disparity_scaled_min=DMIN, disparity_scaled_max=DMAX)[0]
        assert np.array_equal(p32.view(np.uint32), p64.astype(np.float32).view(np.uint32)), name


@pytest.fixture(scope="module")
def image():
    return np.load(os.path.join(GOLDEN_DIR, "match_feature_image.npz"))["image"]


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


def plane_system(amd, models, rectification_model):
    models_rectified = amd.rectified_system(models, az_fov_deg=16, el_fov_deg=9.6, pixels_per_deg_az=10, pixels_per_deg_el=10,
                                            rectification_model=rectification_model)
    W, H = (int(n) for n in models_rectified[0].imagersize())
    assert 140 <= W <= 180 and 85 <= H <= 110, (W, H)
    return models_rectified, W, H


def plane_truth(amd, models_rectified):
    """per pixel of the rectified camera 0: the range to the plane z = 0 along the pixel's ray, the true disparity, the
    range formula restated (the law of sines for LATLON, z = baseline fx/disparity for PINHOLE), and the z component of
    the pixel's ray in the reference frame"""
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
    return range_true, disparity_true, range_of, vref[..., 2]


def assert_same_cloud(got, want, what=""):
    for g, w in zip(got, want):
        if w is None: assert g is None, what
        else:         assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), what


def blobs(H, W, keep_share, seed):
    rng = np.random.default_rng(seed)
    d = rng.integers(40, 600, size=(H, W)).astype(np.int16)
    d[rng.random((H, W)) >= keep_share] = INVALID
    return d


@pytest.mark.gpu
def test_the_same_bits_resident_and_one_shot(amd, image):
    """the resident call is the one-shot call; a Rectification reused over disparity images whose N shrinks and then
    outgrows the output buffers gives what fresh calls give; no buffer stays behind"""
    models, images = plane_scene(amd, image)
    models_rectified, W, H = plane_system(amd, models, MODELS[0])
    color_image = np.stack((images[0], 255 - images[0], images[0]//2), axis=-1)
    disparities = [blobs(H, W, share, 31 + k) for k, share in enumerate((0.3, 0.004, 0.95))]    # (N: ~4600, ~60, ~14600)
    kw = dict(disparity_scale=SCALE, disparity_min=2)
    live0 = amd.device_buffers_live()
    fresh = [amd.stereo_point_cloud(d, models_rectified, models=models, image0=color_image, frame='cam0', **kw) for d in disparities]
    assert amd.device_buffers_live() == live0
    assert len(fresh[1][2]) < 4096 < len(fresh[0][2]) < 8192 < len(fresh[2][2])
    with amd.Rectification(models, models_rectified) as r:
        live1 = amd.device_buffers_live()
        for twice in range(2):
            for d, want in zip(disparities, fresh):
                assert_same_cloud(r.point_cloud(d, image0=color_image, frame='cam0', **kw), want)
        # without colours, and without the models: the stand-alone object
        want = amd.stereo_point_cloud(disparities[0], models_rectified, **kw)
        assert want[1] is None
        assert_same_cloud(r.point_cloud(disparities[0], **kw), want)
        assert_same_cloud(amd.stereo_point_cloud(disparities[0], models_rectified, models=models, **kw), want)
        with amd.StereoPointCloud(models_rectified, map0=r.maps()[0]) as c:
            assert_same_cloud(c.point_cloud(disparities[0], **kw), want)
            gray = c.point_cloud(disparities[2], image0=images[0], **kw)
            assert_same_cloud(gray, r.point_cloud(disparities[2], image0=images[0], **kw))
            assert gray[1].shape == gray[2].shape and gray[1].dtype == np.uint8
        # the cloud's buffers are the rectification's: they go with it
        assert amd.device_buffers_live() > live1
    assert amd.device_buffers_live() == live0


@pytest.mark.gpu
@pytest.mark.parametrize("rectification_model", MODELS)
def test_image_pair_to_cloud(amd, image, rectification_model):
    """point_cloud_of_images() is point_cloud() of Rectification.disparity()'s image, to the bit, with and without the
    speckle filter; the points lie on the plane; the colours are those of the reference's way.

    The points held to the plane: those whose disparity is within 1/16 px, one step of the scale, of the true one.
    A point is origin + range ray, and the true point has z = 0 in the reference frame, so |z| = |range - true range|
    |ray_z|; the range is monotonic in the disparity, so |range - true range| is at most the larger of
    |range_of(true disparity +- 1/16) - true range|, from the range formula restated in plane_truth(), with 1e-9 of the
    range for the rounding in double on either side.

    The reference's colours: project the double-precision points into camera 0 and round to the nearest pixel. A
    projection within 1e-3 px of a half-integer is left out: the float32 map cannot resolve it (at 640 px its spacing
    is 6e-5 px). With a uniform fractional part 2 x 2e-3 = 0.4 % of the pixels are; above 2 % the test fails"""
    models, images = plane_scene(amd, image)
    models_rectified, W, H = plane_system(amd, models, rectification_model)
    range_true, disparity_true, range_of, ray_z = plane_truth(amd, models_rectified)
    lo = int(np.floor(disparity_true.min())) - 4
    kw = dict(disparity_min=lo, disparity_max=lo + 32)
    assert lo > 0 and disparity_true.max() < lo + 28
    live0 = amd.device_buffers_live()
    with amd.Rectification(models, models_rectified) as r:
        disparity = r.disparity(*images, **kw)
        want = r.point_cloud(disparity, image0=images[0], disparity_scale=16, disparity_min=lo)
        got = r.point_cloud_of_images(*images, **kw)
        assert_same_cloud(got, want)
        # no pixel the matcher calls invalid
        assert np.all(disparity.ravel()[want[2]] != 16*(lo - 1))
        for frame, dtype in (('cam0', np.float64), ('rect0', np.float32)):
            assert_same_cloud(r.point_cloud_of_images(*images, frame=frame, dtype=dtype, **kw),
                              r.point_cloud(disparity, image0=images[0], disparity_scale=16, disparity_min=lo, frame=frame, dtype=dtype))
        # a colour image of its own, and range limits
        color_image = np.stack((images[0], 255 - images[0], images[0]//2), axis=-1).astype(np.uint16)*257
        limits = dict(range_min=float(np.percentile(range_true, 20)) + 1e-4, range_max=float(np.percentile(range_true, 80)) + 1e-4)
        limited = r.point_cloud_of_images(*images, color_image=color_image, **limits, **kw)
        assert_same_cloud(limited, r.point_cloud(disparity, image0=color_image, disparity_scale=16, disparity_min=lo, **limits))
        assert 0 < len(limited[2]) < len(want[2]) and limited[1].shape == (len(limited[2]), 3) and limited[1].dtype == np.uint16
        # with the speckle filter: the filtered image's cloud
        filtered = r.disparity(*images, speckle_window_size=50, speckle_range=2, **kw)
        assert (filtered != disparity).any()
        assert_same_cloud(r.point_cloud_of_images(*images, speckle_window_size=50, speckle_range=2, **kw),
                          r.point_cloud(filtered, image0=images[0], disparity_scale=16, disparity_min=lo))
        cam0 = r.point_cloud(disparity, image0=images[0], disparity_scale=16, disparity_min=lo, frame='cam0')
    assert amd.device_buffers_live() == live0

    points, color, index = want
    assert len(index) > 0.5*W*H
    # on the plane
    d = disparity.ravel()[index]/16.
    held = np.abs(d - disparity_true.ravel()[index]) <= 1/16.
    bound = (np.maximum(np.abs(range_of(disparity_true - 1/16.) - range_true), np.abs(range_of(disparity_true + 1/16.) - range_true))
             + 1e-9*range_true)*np.abs(ray_z)
    off, bound = np.abs(points[:, 2]), bound.ravel()[index]
    worst = np.argmax(np.where(held, off/bound, 0))
    print(f"{rectification_model}: {W} x {H}, N = {len(index)} ({len(index)/(W*H):.4f} of the pixels), held {held.mean():.4f}; "
          f"the worst point held is {off[worst]:.6f} off the plane, bound {bound[worst]:.6f}; largest bound {bound[held].max():.6f}")
    assert held.mean() > 0.1            # (the assertion below is about something)
    assert np.all(off[held] <= bound[held])

    # the colours, the reference's way
    assert np.array_equal(cam0[2], index)
    q = amd.project(cam0[0], *models[0].intrinsics())
    fraction = q - np.floor(q)
    unresolved = (np.abs(fraction - 0.5) < 1e-3).any(axis=-1)
    print(f"{rectification_model}: {unresolved.mean():.5f} of the projections are within 1e-3 px of a half-integer")
    assert unresolved.mean() <= 0.02
    iq = np.floor(q[~unresolved] + 0.5).astype(int)
    assert np.all(iq >= 0) and np.all(iq[:, 0] < images[0].shape[1]) and np.all(iq[:, 1] < images[0].shape[0])
    assert np.array_equal(color[~unresolved], images[0][iq[:, 1], iq[:, 0]])
