"""image_transformation_map() and transform_image() (kernels: marked gpu), the two pinhole helpers and the refusals
(host code: no GPU). The map's checker is the reference's compiled unprojection, a numpy transform and the
reference's compiled projection (tests/rectification_checker.py); the remap's is bilinear interpolation in double,
written for these tests."""
import numpy as np
import pytest

from conftest import GOLDEN_DIR
import rectification_checker as chk


def opencv8(amd):  return amd.cameramodel(f"{GOLDEN_DIR}/cam0.opencv8.cameramodel")
def splined(amd):  return amd.cameramodel(f"{GOLDEN_DIR}/cam0.splined.cameramodel")


def small_imager(amd, model, W, H):
    """the same lens looking the same way through a W x H window around its optical axis"""
    lensmodel, intrinsics = model.intrinsics()
    intrinsics = np.array(intrinsics)
    intrinsics[2:4] = ((W - 1.)/2., (H - 1.)/2.)
    return amd.cameramodel(intrinsics=(lensmodel, intrinsics), imagersize=(W, H), rt_cam_ref=model.rt_cam_ref())


def map_checker(ref_api, amd, model_from, model_to, *, intrinsics_only=False, distance=None, plane_n=None, plane_d=None):
    W, H = (int(x) for x in model_to.imagersize())
    v = ref_api.unproject(chk.grid(W, H), *model_to.intrinsics())
    if not intrinsics_only:
        Rt_to_from = amd.compose_Rt(model_to.Rt_cam_ref(), model_from.Rt_ref_cam())
        R, t = Rt_to_from[:3, :], Rt_to_from[3, :]
        if plane_n is not None:
            v = v @ np.linalg.inv(plane_d*R + np.outer(t, plane_n)).T
        elif distance is not None:
            v = (v/np.linalg.norm(v, axis=-1, keepdims=True)*distance - t) @ R        # R^T (x - t)
        else:
            v = v @ R
    return ref_api.project(v, *model_from.intrinsics())


# -------------------------------------------------------------------------------------------------------------------
# host code

def test_scale_focal__best_pinhole_fit(amd, ref_api):
    model = opencv8(amd)
    W, H = model.imagersize()
    lensmodel, intrinsics = model.intrinsics()
    fits = {"corners":            np.array(((0., 0.), (0., H-1.), (W-1., H-1.), (W-1., 0.))),
            "centers-horizontal": np.array(((0, (H-1.)/2.), (W-1., (H-1.)/2.))),
            "centers-vertical":   np.array((((W-1.)/2., 0), ((W-1.)/2., H-1.)))}
    for fit, q in list(fits.items()) + [(np.array(((100., 200.), (W-50., H-300.))),)*2]:
        scale = amd.scale_focal__best_pinhole_fit(model, fit)
        # the scaled pinhole model sees every one of the points, and one of them on an edge of its imager
        v = ref_api.unproject(q, lensmodel, intrinsics)
        qp = v[:, :2]/v[:, 2:]*intrinsics[:2]*scale + intrinsics[2:4]
        assert np.all(qp > -1e-6) and np.all(qp < np.array((W-1., H-1.)) + 1e-6)
        on_edge = np.minimum(np.abs(qp), np.abs(qp - (W-1., H-1.))).min()
        assert on_edge < 1e-6
        pinhole = amd.pinhole_model_for_reprojection(model, fit)
        assert pinhole.intrinsics()[0] == "LENSMODEL_PINHOLE"
        assert np.allclose(pinhole.intrinsics()[1], intrinsics[:4]*(scale, scale, 1, 1), rtol=0, atol=1e-9)
        assert tuple(pinhole.imagersize()) == (W, H) and np.array_equal(pinhole.rt_cam_ref(), model.rt_cam_ref())
    assert amd.scale_focal__best_pinhole_fit(model, None) == 1.0
    assert np.allclose(amd.pinhole_model_for_reprojection(model, scale_focal=0.5).intrinsics()[1], intrinsics[:4]*(.5, .5, 1, 1))
    # scale_image: the centre of the imager keeps its direction
    half = amd.pinhole_model_for_reprojection(model, scale_image=0.5)
    W2, H2 = half.imagersize()
    assert (W2, H2) == (round(W*0.5), round(H*0.5))
    centre  = ((np.array((W, H)) - 1.)/2. - intrinsics[2:4])/intrinsics[:2]
    centre2 = ((W*0.5 - 1.)/2. - half.intrinsics()[1][2], (H*0.5 - 1.)/2. - half.intrinsics()[1][3])/half.intrinsics()[1][:2]
    assert np.allclose(centre, centre2, rtol=0, atol=1e-12)
    with pytest.raises(Exception, match="fit must be either None"):
        amd.scale_focal__best_pinhole_fit(model, "edges")
    with pytest.raises(Exception, match="fit must be either None"):
        amd.scale_focal__best_pinhole_fit(model, 3)
    with pytest.raises(Exception, match=r"shape \(...,2\)"):
        amd.pinhole_model_for_reprojection(model, np.zeros((4, 3)))
    with pytest.raises(Exception, match="At most one of"):
        amd.pinhole_model_for_reprojection(model, "corners", scale_focal=1.)


def test_refusals(amd):
    """every one of them before any device work: they are raised without a GPU"""
    model = opencv8(amd)
    pinhole = amd.pinhole_model_for_reprojection(model, "corners")
    with pytest.raises(Exception, match="both be None or neither"):
        amd.image_transformation_map(model, pinhole, plane_n=np.array((0, 0, 1.)))
    with pytest.raises(Exception, match="both be None or neither"):
        amd.image_transformation_map(model, pinhole, plane_d=1.)
    with pytest.raises(Exception, match="intrinsics_only should be False"):
        amd.image_transformation_map(model, pinhole, plane_n=np.array((0, 0, 1.)), plane_d=1., intrinsics_only=True)
    with pytest.raises(Exception, match="'distance' makes sense only"):
        amd.image_transformation_map(model, pinhole, distance=5., intrinsics_only=True)
    with pytest.raises(Exception, match="'distance' makes sense only"):
        amd.image_transformation_map(model, pinhole, distance=5., plane_n=np.array((0, 0, 1.)), plane_d=1.)

    assert pinhole.valid_intrinsics_region() is None
    with pytest.raises(Exception, match="no valid-intrinsics region"):
        amd.image_transformation_map(pinhole, pinhole, mask_valid_intrinsics_region_from=True)

    image, mapxy = np.zeros((5, 6), dtype=np.uint8), np.zeros((3, 4, 2), dtype=np.float32)
    with pytest.raises(Exception, match="'image' must be a numpy array"):
        amd.transform_image([[1, 2], [3, 4]], mapxy)
    with pytest.raises(Exception, match="'mapxy' must be a numpy array"):
        amd.transform_image(image, [[[0., 0.]]])
    for bad in (image.astype(np.float64), image.astype(np.int16), image.astype(np.int32)):
        with pytest.raises(Exception, match="dtype"):
            amd.transform_image(bad, mapxy)
    for bad in (np.zeros(5, np.uint8), np.zeros((5, 6, 2), np.uint8), np.zeros((5, 6, 4), np.uint8), np.zeros((2, 5, 6, 3), np.uint8)):
        with pytest.raises(Exception, match="shape"):
            amd.transform_image(bad, mapxy)
    for bad in (mapxy.astype(np.float64), np.zeros((3, 4), np.float32), np.zeros((3, 4, 3), np.float32)):
        with pytest.raises(Exception, match="'mapxy' must be a float32 array"):
            amd.transform_image(image, bad)
    for bad in ("reflect", 1, 4, "wrap"):
        with pytest.raises(Exception, match="borderMode"):
            amd.transform_image(image, mapxy, borderMode=bad)
    for bad in ("cubic", 2, "area"):
        with pytest.raises(Exception, match="interpolation"):
            amd.transform_image(image, mapxy, interpolation=bad)
    for bad in (np.zeros((3, 4), np.uint16), np.zeros((3, 5), np.uint8), np.zeros((3, 4, 3), np.uint8), [0]):
        with pytest.raises(Exception, match="'out' must be"):
            amd.transform_image(image, mapxy, out=bad)
    with pytest.raises(Exception, match="borderValue"):
        amd.transform_image(np.zeros((5, 6, 3), np.uint8), mapxy, borderValue=(1, 2))


# -------------------------------------------------------------------------------------------------------------------
# image_transformation_map()

def moved(amd, model, rt):
    out = amd.cameramodel(model)
    out.rt_ref_cam(amd.compose_rt(model.rt_ref_cam(), np.asarray(rt, dtype=float)))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ("intrinsics_only", "rotation", "distance", "plane", "splined_to_opencv8"))
def test_image_transformation_map_against_the_checker(amd, ref_api, mode):
    """the maps' criterion, on each of the two imagers"""
    live = amd.device_buffers_live()
    for W, H in ((67, 5), (256, 3)):
        model_from = opencv8(amd)
        if mode == "splined_to_opencv8":
            # the TO model has no formula for its unprojection: the path through the buffer of vectors
            model_from, kw = splined(amd), {}
            model_to = small_imager(amd, moved(amd, opencv8(amd), (0.01, -0.02, 0.03, 0.1, 0.2, -0.1)), W, H)
        else:
            pinhole = amd.pinhole_model_for_reprojection(model_from, fit="corners")
            model_to = small_imager(amd, moved(amd, pinhole, (0.02, -0.03, 0.01, 0.3, -0.1, 0.2)), W, H)
            kw = dict(intrinsics_only={"intrinsics_only": True}, rotation={}, distance={"distance": 5.},
                      plane={"plane_n": np.array((0.1, -1, 0.2)), "plane_d": 1.5})[mode]
        mapxy = amd.image_transformation_map(model_from, model_to, **kw)
        assert mapxy.dtype == np.float32 and mapxy.shape == (H, W, 2)
        chk.compare_map(mapxy, map_checker(ref_api, amd, model_from, model_to, **kw), f"image_transformation_map {mode} {W}x{H}")
        assert np.array_equal(mapxy, amd.image_transformation_map(model_from, model_to, **kw))
    assert amd.device_buffers_live() == live


@pytest.mark.gpu
@pytest.mark.parametrize("model", ("opencv8", "splined"))
def test_identical_models_give_the_pixel_grid(amd, model):
    m = small_imager(amd, opencv8(amd) if model == "opencv8" else splined(amd), 67, 5)
    mapxy = amd.image_transformation_map(m, m)
    assert np.abs(mapxy - chk.grid(67, 5)).max() < 1e-3


@pytest.mark.gpu
def test_mask_valid_intrinsics_region(amd, ref_api):
    model_from = opencv8(amd)
    W0, H0 = model_from.imagersize()
    pentagon = np.array(((0.30*W0, 0.20*H0), (0.72*W0, 0.25*H0), (0.80*W0, 0.70*H0), (0.50*W0, 0.85*H0), (0.22*W0, 0.60*H0)))
    model_from.valid_intrinsics_region(pentagon)
    region = np.asarray(model_from.valid_intrinsics_region(), dtype=float)
    assert np.array_equal(region[0], region[-1])           # closed
    pinhole = amd.pinhole_model_for_reprojection(model_from, fit="corners", scale_image=1./16.)
    W, H = pinhole.imagersize()
    assert W*H > 512                                        # more than one block
    mapxy = amd.image_transformation_map(model_from, pinhole, intrinsics_only=True, mask_valid_intrinsics_region_from=True)
    unmasked = map_checker(ref_api, amd, model_from, pinhole, intrinsics_only=True)
    near_an_edge = chk.distance_to_polygon(region, unmasked) < 1e-6
    assert near_an_edge.mean() <= 1e-3
    inside = chk.inside_polygon(region, unmasked)
    assert 0.1 < inside.mean() < 0.9
    masked = np.all(mapxy == -1, axis=-1)
    assert np.array_equal(masked[~near_an_edge], ~inside[~near_an_edge])
    keep = inside & ~near_an_edge
    want = np.where(keep[..., None], unmasked, -1.)
    got  = np.where(keep[..., None], mapxy, np.float32(-1.))
    chk.compare_map(got, want, "masked map")


# -------------------------------------------------------------------------------------------------------------------
# transform_image()

WS, HS = 37, 29
WIDTHS = (1, 3, 4, 5, 63, 64, 65, 259)
DTYPES = (np.uint8, np.uint16, np.float32)


def source(dtype, channels, seed=3):
    rng = np.random.default_rng(seed)
    shape = (HS, WS) if channels == 1 else (HS, WS, 3)
    if dtype == np.float32:
        return rng.uniform(-100., 1000., size=shape).astype(np.float32)
    image = rng.integers(0, np.iinfo(dtype).max + 1, size=shape).astype(dtype)
    image.flat[:4] = (0, np.iinfo(dtype).max, np.iinfo(dtype).max, 0)        # saturation
    return image


def make_map(W, seed=5):
    """(3,W,2): integer points, half points, points within 1.5 pixels of every edge, far outside, NaN and infinities"""
    rng = np.random.default_rng(seed + W)
    m = np.empty((3, W, 2), dtype=np.float32)
    m[..., 0] = rng.uniform(-1.5, WS + 0.5, size=(3, W))
    m[..., 1] = rng.uniform(-1.5, HS + 0.5, size=(3, W))
    special = [(3., 4.), (3.5, 4.), (3., 4.5), (3.5, 4.5), (0., 0.), (WS - 1., HS - 1.), (WS - 1., 0.), (0., HS - 1.),
               (-0.5, 5.), (-1., 5.), (-1.5, 5.), (WS - 0.5, 5.), (WS, 5.), (WS + 0.5, 5.), (5., -0.5), (5., -1.), (5., HS - 0.5),
               (5., HS), (5., HS + 0.5), (-0.25, -0.75), (WS - 0.75, HS - 0.25), (-1e9, 3.), (3., 1e9), (1e30, -1e30),
               (np.nan, 3.), (3., np.nan), (np.inf, 3.), (3., -np.inf), (np.nan, np.nan), (12.25, 20.75)]
    flat = m.reshape(-1, 2)
    for i, s in enumerate(special[:flat.shape[0]]):
        flat[(i*7) % flat.shape[0]] = s
    return m


def tolerance(dtype, largest):
    if dtype == np.float32:
        return 8*np.spacing(largest.astype(np.float32)).astype(np.float64)
    return 0.5 + 8*2.**-23*np.iinfo(dtype).max


@pytest.mark.gpu
@pytest.mark.parametrize("channels", (1, 3))
@pytest.mark.parametrize("dtype", DTYPES)
def test_transform_image_against_bilinear_interpolation_in_double(amd, dtype, channels):
    image = source(dtype, channels)
    border_value = 7 if channels == 1 else (7, 200, 31)
    live = amd.device_buffers_live()
    for W in WIDTHS:
        mapxy = make_map(W)
        exact, outside, largest = chk.bilinear(image, mapxy, border_value)
        if dtype != np.float32:
            exact = np.clip(exact, 0, np.iinfo(dtype).max)
        got = amd.transform_image(image, mapxy, borderValue=border_value)
        assert got.dtype == dtype and got.shape == ((3, W) if channels == 1 else (3, W, 3))
        err = np.abs(got.astype(np.float64).reshape(exact.shape) - exact)
        assert np.all(err <= tolerance(dtype, largest)), f"W={W}: {err.max()}"
        assert np.array_equal(got, amd.transform_image(image, mapxy, borderValue=border_value, borderMode='constant', interpolation=1))

        # transparent: untouched exactly where a neighbour is outside; the same values elsewhere
        before = (np.arange(got.size).reshape(got.shape) % 251).astype(dtype)
        out = before.copy()
        ret = amd.transform_image(image, mapxy, out=out, borderMode='transparent')
        assert ret is out
        o = outside if channels == 1 else outside[..., None]
        assert np.array_equal(np.where(o, out, 0), np.where(o, before, 0))
        assert np.array_equal(np.where(o, 0, out), np.where(o, 0, got))
        assert np.array_equal(out, amd.transform_image(image, mapxy, out=before.copy(), borderMode=5))
        assert outside.any() and not outside.all() or W < 3

        # nearest: source values exactly (the map's half points are left out: a tie)
        x, y = mapxy[..., 0].astype(np.float64), mapxy[..., 1].astype(np.float64)
        with np.errstate(invalid="ignore"):
            tie = (np.abs(x - np.floor(x) - 0.5) < 1e-6) | (np.abs(y - np.floor(y) - 0.5) < 1e-6)
            finite = np.isfinite(x) & np.isfinite(y) & (np.abs(x) < 1e6) & (np.abs(y) < 1e6)
            ix, iy = np.where(finite, np.rint(x), -1).astype(int), np.where(finite, np.rint(y), -1).astype(int)
        inside = finite & (ix >= 0) & (ix < WS) & (iy >= 0) & (iy < HS)
        want = np.where(inside if channels == 1 else inside[..., None],
                        image[np.clip(iy, 0, HS-1), np.clip(ix, 0, WS-1)], np.asarray(border_value, dtype=dtype))
        got = amd.transform_image(image, mapxy, borderValue=border_value, interpolation='nearest')
        assert np.array_equal(got[~tie], want[~tie])
        assert np.array_equal(got, amd.transform_image(image, mapxy, borderValue=border_value, interpolation=0))
    assert amd.device_buffers_live() == live


@pytest.mark.gpu
@pytest.mark.parametrize("channels", (1, 3))
@pytest.mark.parametrize("dtype", DTYPES)
def test_identity_map_returns_the_image(amd, dtype, channels):
    image = source(dtype, channels)
    mapxy = chk.grid(WS, HS).astype(np.float32)
    assert np.array_equal(amd.transform_image(image, mapxy), image)
    assert np.array_equal(amd.transform_image(image, mapxy, interpolation='nearest'), image)
    # out= is honoured: a dense one is filled in place, a view is filled through a copy
    out = np.zeros_like(image)
    assert amd.transform_image(image, mapxy, out=out) is out and np.array_equal(out, image)
    wide = np.zeros((HS, 2*WS) + image.shape[2:], dtype=dtype)
    view = wide[:, ::2]
    assert amd.transform_image(image, mapxy, out=view) is view and np.array_equal(view, image) and not wide[:, 1::2].any()
    # a source that is a view
    assert np.array_equal(amd.transform_image(np.ascontiguousarray(image[:, ::-1])[:, ::-1], mapxy), image)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,channels", ((np.uint8, 1), (np.uint8, 3), (np.uint16, 1), (np.float32, 3)))
def test_rectify_is_transform_image_through_the_maps(amd, dtype, channels):
    model0 = opencv8(amd)
    model1 = moved(amd, model0, (0, 0, 0, 0.5, 0, 0))
    small = [small_imager(amd, m, WS, HS) for m in (model0, model1)]
    geometry = amd.rectified_system(small, az_fov_deg=1.2, el_fov_deg=0.8, pixels_per_deg_az=54.2, pixels_per_deg_el=51.25)
    Naz, Nel = geometry[0].imagersize()
    assert (Naz*Nel) % 4 != 0 and Naz*Nel > 1024
    image0, image1 = source(dtype, channels, 11), source(dtype, channels, 12)
    live = amd.device_buffers_live()
    with amd.Rectification(small, geometry) as r:
        maps = r.maps()
        assert np.isfinite(maps).all() and (maps > 0).mean() > 0.5          # mostly inside the images
        rect0, rect1 = r.rectify(image0, image1)
        assert np.array_equal(rect0, amd.transform_image(image0, maps[0]))
        assert np.array_equal(rect1, amd.transform_image(image1, maps[1]))
        assert rect0.any() and rect1.any()
        out = (np.empty_like(rect0), np.empty_like(rect1))
        ret = r.rectify(image0, image1, out=out)
        assert ret[0] is out[0] and ret[1] is out[1] and np.array_equal(out[0], rect0) and np.array_equal(out[1], rect1)
        with pytest.raises(Exception, match="same dtype"):
            r.rectify(image0, image1.astype(np.float32) if dtype != np.float32 else image1.astype(np.uint8))
    assert amd.device_buffers_live() == live
    with pytest.raises(Exception, match="has been closed"):
        r.maps()
