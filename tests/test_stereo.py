"""Stereo rectification: the rectified system (host code: no GPU), its maps and the ranges (kernels: marked gpu).

The checker is composed from the reference's compiled mrcal_project() / mrcal_unproject() (ref_api) and numpy written
for these tests (tests/rectification_checker.py); the geometry is also held to the numbers the reference's own
test/test-stereo.py publishes."""
import ctypes as C
import numpy as np
import pytest

from conftest import GOLDEN_DIR
import hostbuild
import rectification_checker as chk

MODELS = ("LENSMODEL_LATLON", "LENSMODEL_PINHOLE")
RT01   = np.array((0.1, 0.2, 0.05, 3.0, 0.2, 1.0))
# test/test-stereo.py: "I visualized the geometry, and confirmed that it is correct"
RT_CAM0_RECT = np.array([[0.9467916, -0.08500675, -0.31041828],
                         [0.06311944, 0.99480206, -0.07990489],
                         [0.3155972,  0.05605985,  0.94723582],
                         [0., 0., 0.]])
SYSTEM = dict(az_fov_deg=90, el_fov_deg=50, el0_deg=10., pixels_per_deg_az=-1./8., pixels_per_deg_el=-1./4.)


def pair(amd, rt01):
    model0 = amd.cameramodel(f"{GOLDEN_DIR}/cam0.opencv8.cameramodel")
    model1 = amd.cameramodel(model0)
    model1.rt_ref_cam(amd.compose_rt(model0.rt_ref_cam(), rt01))
    return model0, model1


def angle_deg(a, b):
    return np.degrees(np.arccos(np.dot(a, b)/(np.linalg.norm(a)*np.linalg.norm(b))))


@pytest.fixture(scope="module")
def hostlib():
    """csrc/stereo_geometry.cpp built for the host, by itself"""
    return C.CDLL(hostbuild.build_library("stereo_check"))


# -------------------------------------------------------------------------------------------------------------------
# the host's part: runs without a GPU

@pytest.mark.parametrize("rectification_model", MODELS)
@pytest.mark.parametrize("geometry", ("vanilla", "complex"))
def test_rectified_system_as_the_reference_tests_it(amd, ref_api, rectification_model, geometry):
    rt01 = np.array((0, 0, 0, 3.0, 0, 0)) if geometry == "vanilla" else RT01
    el0_deg = 0. if geometry == "vanilla" else 10.
    model0, model1 = pair(amd, rt01)
    models_rectified, meta = amd.rectified_system((model0, model1), **{**SYSTEM, "el0_deg": el0_deg},
                                                  rectification_model=rectification_model, return_metadata=True)
    amd.stereo._validate_models_rectified(models_rectified)
    for m in models_rectified:
        assert m.intrinsics()[0] == rectification_model
    assert np.array_equal(models_rectified[0].intrinsics()[1], models_rectified[1].intrinsics()[1])

    Rt_cam0_rect   = amd.compose_Rt(model0.Rt_cam_ref(), models_rectified[0].Rt_ref_cam())
    Rt01_rectified = amd.compose_Rt(models_rectified[0].Rt_cam_ref(), models_rectified[1].Rt_ref_cam())
    assert np.allclose(Rt_cam0_rect, amd.identity_Rt() if geometry == "vanilla" else RT_CAM0_RECT, rtol=0, atol=1e-6)
    assert abs(Rt01_rectified[3, 0] - np.linalg.norm(rt01[3:])) < 1e-9
    assert abs(meta["baseline"]     - np.linalg.norm(rt01[3:])) < 1e-9

    # az0: the mean forward direction of the two cameras against the baseline
    baseline  = rt01[3:]/np.linalg.norm(rt01[3:])
    forward01 = np.array((0, 0, 1.)) + chk.rotation(rt01[:3]) @ np.array((0, 0, 1.))
    az0, el0  = np.arcsin(np.dot(forward01, baseline)/np.linalg.norm(forward01)), np.radians(el0_deg)
    assert abs(np.radians(meta["az0_deg"]) - az0) < 1e-9

    # the centre pixel looks at (az0, el0)
    Naz, Nel = models_rectified[0].imagersize()
    unproject = lambda q: ref_api.unproject(np.asarray(q, dtype=float), *models_rectified[0].intrinsics())
    project0  = lambda v: ref_api.project(Rt_cam0_rect[:3, :] @ v, *model0.intrinsics())
    q0 = np.array(((Naz-1.)/2., (Nel-1.)/2.))
    v0 = unproject(q0); v0 /= np.linalg.norm(v0)
    if rectification_model == "LENSMODEL_LATLON":
        assert np.allclose(v0, (np.sin(az0), np.cos(az0)*np.sin(el0), np.cos(az0)*np.cos(el0)), rtol=0, atol=1e-6)
    else:
        v0_rect = np.array((np.tan(az0), np.tan(el0), 1.))
        assert np.allclose(v0, v0_rect/np.linalg.norm(v0_rect), rtol=0, atol=1e-3)

    # the pixel density is camera 0's there, over 8 and over 4: within 1 %
    v0x, v0y = unproject(q0 + (1e-1, 0)), unproject(q0 + (0, 1e-1))
    dthx, dthy = np.radians(angle_deg(v0x, v0)), np.radians(angle_deg(v0y, v0))
    assert abs(0.1/dthx*8. / (np.linalg.norm(project0(v0x) - project0(v0))/dthx) - 1.) < 1e-2
    assert abs(0.1/dthy*4. / (np.linalg.norm(project0(v0y) - project0(v0))/dthy) - 1.) < 1e-2

    # the field of view: within 1 degree in azimuth (0.5 in the vanilla geometry), 0.5 in elevation
    az_fov = angle_deg(unproject((0, (Nel-1.)/2.)), unproject((Naz-1, (Nel-1.)/2.)))
    assert abs(az_fov - 90) < (0.5 if geometry == "vanilla" else 1.)
    a, b = unproject(((Naz-1.)/2., 0)), unproject(((Naz-1.)/2., Nel-1))
    a[0] = b[0] = 0          # el_fov applies at the stereo centre only
    assert abs(angle_deg(a, b) - 50) < 0.5


@pytest.mark.parametrize("rectification_model", MODELS)
@pytest.mark.parametrize("az_edge_margin_deg", (10., 40.))
def test_rectified_system_against_the_numpy_restatement(amd, ref_api, rectification_model, az_edge_margin_deg):
    models = pair(amd, RT01)
    models_rectified, meta = amd.rectified_system(models, **SYSTEM, rectification_model=rectification_model,
                                                  az_edge_margin_deg=az_edge_margin_deg, return_metadata=True)
    fxycxy, NazNel, R_rect0_cam0, baseline, az0_deg = \
        chk.rectified_system_restated(ref_api, models, **SYSTEM, rectification_model=rectification_model,
                                      az_edge_margin_deg=az_edge_margin_deg)
    if az_edge_margin_deg == 40.:
        # the autodetected centre (24 degrees) does not fit a 90-degree view inside the margins: shifted
        assert meta["az0_deg"] == 90. - 40. - 90/2.
    assert abs(meta["az0_deg"] - az0_deg) < 1e-9
    assert tuple(int(x) for x in models_rectified[0].imagersize()) == NazNel
    assert np.allclose(models_rectified[0].intrinsics()[1], fxycxy, rtol=0, atol=1e-9)
    assert abs(meta["baseline"] - baseline) < 1e-9
    R_rect0_ref = R_rect0_cam0 @ chk.rotation(models[0].rt_cam_ref()[:3])
    assert np.allclose(models_rectified[0].Rt_cam_ref()[:3, :], R_rect0_ref, rtol=0, atol=1e-9)
    if rectification_model == "LENSMODEL_LATLON" and az_edge_margin_deg == 10.:
        # the restatement's numbers, as measured against the compiled reference projection
        assert np.allclose(fxycxy, (223.4535, 409.0919, 81.5153, 106.6), rtol=0, atol=1e-4)
        assert NazNel == (351, 357)


def test_rectified_system_legacy_entry_point_has_a_margin_of_10(amd):
    lib = amd._lib
    model0, model1 = pair(amd, RT01)
    m = lib.lensmodel(model0.intrinsics()[0])
    intrinsics = np.ascontiguousarray(model0.intrinsics()[1])
    rt0, rt1 = np.ascontiguousarray(model0.rt_cam_ref()), np.ascontiguousarray(model1.rt_cam_ref())
    results = []
    for name, margin in (("mrcal_rectified_system", ()), ("mrcal_rectified_system2", (10.,))):
        size, fxycxy, rt, baseline = (C.c_uint*2)(), np.zeros(4), np.zeros(6), C.c_double()
        az, el = C.c_double(-1/8.), C.c_double(-1/4.)
        fov, centre = (C.c_double*2)(90, 50), (C.c_double*2)(0, 10)
        f = getattr(lib.lib, name)
        f.restype  = C.c_bool
        f.argtypes = [C.c_void_p]*8 + [C.c_double]*len(margin) + [C.c_void_p]*4 + [C.c_int] + [C.c_bool]*4
        assert f(size, fxycxy.ctypes.data, rt.ctypes.data, C.addressof(baseline), C.addressof(az), C.addressof(el), fov, centre,
                 *margin, C.addressof(m), intrinsics.ctypes.data, rt0.ctypes.data, rt1.ctypes.data, 3, True, False, False, False)
        results.append((tuple(size), tuple(fxycxy), tuple(rt), baseline.value, az.value, el.value, tuple(fov), tuple(centre)))
    assert results[0] == results[1]


def test_rectified_resolution(amd, ref_api):
    model0 = amd.cameramodel(f"{GOLDEN_DIR}/cam0.opencv8.cameramodel")
    for rectification_model in MODELS + ("LENSMODEL_LONLAT",):
        az0, el0 = np.radians(4.), np.radians(6.)
        got = amd.rectified_resolution(model0, az_fov_deg=90, el_fov_deg=50, az0_deg=4., el0_deg=6.,
                                       R_cam0_rect0=amd.identity_R(), pixels_per_deg_az=-1./8., pixels_per_deg_el=-1./4.,
                                       rectification_model=rectification_model)
        # central differences of the reference's projection along az and el
        def v(az, el):
            if rectification_model == "LENSMODEL_LATLON": return np.array((np.sin(az), np.cos(az)*np.sin(el), np.cos(az)*np.cos(el)))
            if rectification_model == "LENSMODEL_LONLAT": return np.array((np.cos(el)*np.sin(az), np.sin(el), np.cos(el)*np.cos(az)))
            return np.array((np.tan(az), np.tan(el), 1.))
        q = lambda az, el: ref_api.project(v(az, el), *model0.intrinsics())
        h = 1e-5
        ppd_az = np.linalg.norm(q(az0+h, el0) - q(az0-h, el0))/(2*h)*np.pi/180./8.
        ppd_el = np.linalg.norm(q(az0, el0+h) - q(az0, el0-h))/(2*h)*np.pi/180./4.
        if rectification_model != "LENSMODEL_PINHOLE":
            ppd_az, ppd_el = round(90*ppd_az)/90., round(50*ppd_el)/50.
            assert got == (ppd_az, ppd_el)
        else:
            assert np.allclose(got, (ppd_az, ppd_el), rtol=1e-6)
        # a value that is given is used
        given = amd.rectified_resolution(model0, az_fov_deg=90, el_fov_deg=50, az0_deg=4., el0_deg=6., R_cam0_rect0=amd.identity_R(),
                                         pixels_per_deg_az=3.25, pixels_per_deg_el=-1./4., rectification_model="LENSMODEL_PINHOLE")
        assert given[0] == 3.25


@pytest.mark.parametrize("fov_deg", (20, 90, 120, 170))
@pytest.mark.parametrize("tanaz0", (0, 0.05, -0.05, 0.445, -0.445, 2, -2))
def test_quartic_of_the_pinhole_centre_pixel(hostlib, tanaz0, fov_deg):
    """The library's bracketing solver against numpy.roots, through the reference's three filters. fxy is a real
    focal length (with fxy = 1 the positive-size filter keeps both mirror solutions at small fields of view, and
    which of the two equal 'most positive' ones wins is a matter of rounding, in the reference too).

    Tolerance. numpy.roots is good to a few ulp of the root's size on a simple root: 1e-12 relative is allowed. At
    fov = 90 degrees cos(fov) = 0 (6e-17) and the quartic is MINUS A SQUARE: every root is double, and an eigenvalue
    solver returns a double root to sqrt(DBL_EPSILON) = 1.5e-8 relative at best; 1e-6 is allowed there, and the
    library's root is also held to the unsquared equation itself"""
    f = hostlib.stereocheck_rectified_pinhole_cxy
    f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_double]
    fxy = 200.
    cxy = C.c_double()
    ok = bool(f(C.addressof(cxy), fxy, tanaz0, fov_deg))
    want = chk.pinhole_cxy_restated(fxy, tanaz0, fov_deg)
    assert ok == (want is not None)
    if not ok: return
    tol = 1e-6 if fov_deg == 90 else 1e-12
    assert abs(cxy.value - want) <= tol*max(abs(want), fxy)
    # the equation that was squared: the edges of the imager are fov apart
    Cn, K = cxy.value/fxy, 2.*tanaz0
    cosfov = (1 - K*Cn - Cn*Cn)/np.sqrt((1 + Cn*Cn)*(1 + Cn*Cn + K*K + 2*K*Cn))
    assert abs(cosfov - np.cos(np.radians(fov_deg))) < 1e-12


def test_host_build_root_finder_against_numpy(hostlib):
    """polynomials of every order the solver takes, with simple, double and no real roots. Simple roots: numpy's
    eigenvalues are good to a few ulp of the largest root; 1e-12 of it is allowed. A double root is reported once, and
    numpy has it to sqrt(DBL_EPSILON): 1e-6"""
    f = hostlib.stereocheck_roots_real_polynomial
    f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_int, C.c_void_p]
    cases = [((2.5,), 0), ((-3., 2.), 0), ((1., 1., 1.), 0), ((-1., 0.), 0), ((-6., 11., -6.), 0), ((1., 0., 1., 0.), 0),
             ((24., -50., 35., -10.), 0), ((-2., 1., 0.3, -4.), 0), ((1., 0., -2., 0.), 2), ((4., -4., 1.), 1), ((0., 0., 1., -2.), 1)]
    for c, Ndouble in cases:          # c[0] + c[1] x + ... + x^n
        n = len(c)
        coeffs, roots = np.array(c, dtype=float), np.zeros(4)
        N = f(roots.ctypes.data, n, coeffs.ctypes.data)
        r = np.roots((1.,) + tuple(reversed(c)))
        want = np.sort(r[np.abs(r.imag) <= 1e-7].real)
        if Ndouble:
            want = want[np.concatenate(((True,), np.diff(want) > 1e-4))]         # each double root once
        assert N == want.size, (c, roots[:N], want)
        scale = max(1., np.abs(r).max())
        assert np.all(np.diff(roots[:N]) > 0)
        assert np.allclose(roots[:N], want, rtol=0, atol=(1e-6 if Ndouble else 1e-12)*scale), (c, roots[:N], want)


@pytest.mark.parametrize("rectification_model", MODELS)
def test_host_build_gives_the_library_s_system(amd, hostlib, rectification_model):
    """the whole of rectified_system() runs in a build that has nothing of the device in it, to the library's bits"""
    model0, model1 = pair(amd, RT01)
    m = amd._lib.lensmodel(model0.intrinsics()[0])
    intrinsics = np.ascontiguousarray(model0.intrinsics()[1])
    rt0, rt1 = np.ascontiguousarray(model0.rt_cam_ref()), np.ascontiguousarray(model1.rt_cam_ref())
    results = []
    for lib in (amd._lib.lib, hostlib):
        size, fxycxy, rt, baseline = (C.c_uint*2)(), np.zeros(4), np.zeros(6), C.c_double()
        az, el = C.c_double(-1/8.), C.c_double(-1/4.)
        fov, centre = (C.c_double*2)(90, 50), (C.c_double*2)(0, 10)
        f = lib.mrcal_rectified_system2
        f.restype  = C.c_bool
        f.argtypes = [C.c_void_p]*8 + [C.c_double] + [C.c_void_p]*4 + [C.c_int] + [C.c_bool]*4
        assert f(size, fxycxy.ctypes.data, rt.ctypes.data, C.addressof(baseline), C.addressof(az), C.addressof(el), fov, centre,
                 10., C.addressof(m), intrinsics.ctypes.data, rt0.ctypes.data, rt1.ctypes.data,
                 amd._lib.lensmodel(rectification_model).type, True, False, False, False)
        results.append((tuple(size), tuple(fxycxy), tuple(rt), baseline.value, az.value, el.value, tuple(fov), tuple(centre)))
    assert results[0] == results[1]


def test_rectified_system_refusals(amd):
    model0, model1 = pair(amd, RT01)
    ok = dict(az_fov_deg=90, el_fov_deg=50)
    with pytest.raises(Exception, match="exactly 2"):
        amd.rectified_system((model0,), **ok)
    with pytest.raises(Exception, match="pixels_per_deg_az == 0 is illegal"):
        amd.rectified_system((model0, model1), **ok, pixels_per_deg_az=0)
    with pytest.raises(Exception, match="pixels_per_deg_el == 0 is illegal"):
        amd.rectified_system((model0, model1), **ok, pixels_per_deg_el=0)
    with pytest.raises(Exception, match="must be > 0"):
        amd.rectified_system((model0, model1), az_fov_deg=0, el_fov_deg=50)
    with pytest.raises(Exception, match="must be > 0"):
        amd.rectified_system((model0, model1), az_fov_deg=90, el_fov_deg=-1)
    with pytest.raises(Exception, match="unnaturally small baseline"):
        amd.rectified_system((model0, model0), **ok)
    with pytest.raises(Exception, match="looks along the baseline"):
        amd.rectified_system((model0, model1), **ok, az0_deg=60.)
    with pytest.raises(Exception, match="az_fov_deg is too large"):
        amd.rectified_system((model0, model1), az_fov_deg=170, el_fov_deg=50)
    with pytest.raises(Exception, match="LENSMODEL_LATLON and LENSMODEL_PINHOLE"):
        amd.rectified_system((model0, model1), **ok, rectification_model="LENSMODEL_LONLAT")
    intr = np.array((1000., 1000., 500., 400., 0.01, -0.02, 0.1, 0.01, -0.01, 1e-3, 0., 0.))
    noncentral = amd.cameramodel(intrinsics=("LENSMODEL_CAHVORE_linearity=0.37", intr), imagersize=(1000, 800))
    moved = amd.cameramodel(noncentral); moved.rt_ref_cam(RT01)
    with pytest.raises(Exception, match="only possible with a central projection"):
        amd.rectified_system((noncentral, moved), **ok)
    # ... and with E = 0 it is central
    intr[-3:] = 0
    central = amd.cameramodel(intrinsics=("LENSMODEL_CAHVORE_linearity=0.37", intr), imagersize=(1000, 800))
    moved = amd.cameramodel(central); moved.rt_ref_cam(RT01)
    amd.stereo._validate_models_rectified(amd.rectified_system((central, moved), **ok))


def test_validate_models_rectified_and_range_refusals(amd):
    models_rectified = amd.rectified_system(pair(amd, RT01), az_fov_deg=90, el_fov_deg=50)
    v = amd.stereo._validate_models_rectified
    with pytest.raises(Exception, match="exactly two models"):
        v(models_rectified[:1])
    other = amd.cameramodel(models_rectified[1])
    other.intrinsics(("LENSMODEL_LATLON", models_rectified[1].intrinsics()[1] + (1., 0, 0, 0)))
    with pytest.raises(Exception, match="same intrinsics"):
        v((models_rectified[0], other))
    other = amd.cameramodel(models_rectified[1]); other.rt_cam_ref(other.rt_cam_ref() + (0.01, 0, 0, 0, 0, 0))
    with pytest.raises(Exception, match="same relative rotation"):
        v((models_rectified[0], other))
    other = amd.cameramodel(models_rectified[1]); other.rt_cam_ref(other.rt_cam_ref() + (0, 0, 0, 0, 0.01, 0))
    with pytest.raises(Exception, match=r"ONLY in the \+x"):
        v((models_rectified[0], other))
    stereographic = [amd.cameramodel(intrinsics=("LENSMODEL_STEREOGRAPHIC", m.intrinsics()[1]), imagersize=m.imagersize(),
                                     rt_cam_ref=m.rt_cam_ref()) for m in models_rectified]
    with pytest.raises(Exception, match="LENSMODEL_LATLON' or 'LENSMODEL_PINHOLE"):
        v(stereographic)
    # stereo_range(): refused before any device work
    with pytest.raises(Exception, match="may not both be given"):
        amd.stereo_range(np.zeros(3), models_rectified, qrect0=np.zeros((3, 2)), disparity_min=1, disparity_scaled_min=2)
    with pytest.raises(Exception, match="may not both be given"):
        amd.stereo_range(np.zeros(3), models_rectified, qrect0=np.zeros((3, 2)), disparity_max=1, disparity_scaled_max=2)
    with pytest.raises(Exception, match="MUST have the same dimensions"):
        amd.stereo_range(np.zeros((3, 4)), models_rectified)
    with pytest.raises(Exception, match="Exactly one of"):
        amd.stereo_unproject(None, models_rectified)
    with pytest.raises(Exception, match="Exactly one of"):
        amd.stereo_unproject(np.zeros(3), models_rectified, ranges=np.zeros(3))


# -------------------------------------------------------------------------------------------------------------------
# the device's part

def zoomed(amd, model, zoom):
    out = amd.cameramodel(model)
    intrinsics = np.array(model.intrinsics()[1]); intrinsics[:2] *= zoom
    out.intrinsics((model.intrinsics()[0], intrinsics))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("zoom", (0.6, 1., 10.))
@pytest.mark.parametrize("rectification_model", MODELS)
def test_rectification_maps_against_the_checker(amd, ref_api, rectification_model, zoom):
    """the setup of the reference's test/test-rectification-maps.py. Measured on an MI355X (the share of entries
    that differ from the checker's float32; none is further than one spacing away):
    see the f8 row of DESIGN.md section 9"""
    model0, model1 = pair(amd, RT01)
    intrinsics = np.array(model1.intrinsics()[1])
    intrinsics[:2] *= (1.01, -0.98); intrinsics[2:4] += (50, 80.)
    model1.intrinsics((model1.intrinsics()[0], intrinsics))
    models_rectified = amd.rectified_system((zoomed(amd, model0, zoom), zoomed(amd, model1, zoom)),
                                            az_fov_deg=90/zoom, el_fov_deg=50/zoom,
                                            pixels_per_deg_az=-1./8., pixels_per_deg_el=-1./4.,
                                            rectification_model=rectification_model)
    maps = amd.rectification_maps((model0, model1), models_rectified)
    Naz, Nel = models_rectified[0].imagersize()
    assert maps.dtype == np.float32 and maps.shape == (2, Nel, Naz, 2)
    checker = chk.rectification_maps_checker(ref_api, (model0, model1), models_rectified)
    chk.compare_map(maps, checker, f"rectification_maps {rectification_model} zoom {zoom} ({Naz}x{Nel})")


def stereographic_model(amd, model):
    return amd.cameramodel(intrinsics=("LENSMODEL_STEREOGRAPHIC", np.array(model.intrinsics()[1][:4])*(0.5, 0.5, 1, 1)),
                           imagersize=model.imagersize(), rt_cam_ref=model.rt_cam_ref())
def cahvore_model(amd, model):
    intr = np.concatenate((model.intrinsics()[1][:4], (0.01, -0.02, 0.1, 0.01, -0.01, 0., 0., 0.)))
    return amd.cameramodel(intrinsics=("LENSMODEL_CAHVORE_linearity=0.37", intr), imagersize=model.imagersize(),
                           rt_cam_ref=model.rt_cam_ref())


@pytest.mark.gpu
@pytest.mark.parametrize("cameras", ("opencv8+splined", "stereographic", "cahvore"))
def test_rectification_maps_shapes(amd, ref_api, cameras):
    """every tail of the two-pixels-a-lane store and more than one block, for the models of every kernel family;
    the same bits twice; the resident form gives the one-shot form's bits; no device buffer is left behind"""
    live = amd.device_buffers_live()
    model0, model1 = pair(amd, np.array((0.01, 0.02, 0.005, 0.5, 0.01, 0.02)))
    if cameras == "opencv8+splined":
        splined = amd.cameramodel(f"{GOLDEN_DIR}/cam0.splined.cameramodel")
        model1.intrinsics(splined.intrinsics(), imagersize=splined.imagersize())
    elif cameras == "stereographic": model0, model1 = stereographic_model(amd, model0), stereographic_model(amd, model1)
    else:                            model0, model1 = cahvore_model(amd, model0), cahvore_model(amd, model1)
    geometry = amd.rectified_system((model0, model1), az_fov_deg=40, el_fov_deg=20, pixels_per_deg_az=1., pixels_per_deg_el=1.)
    az_fov, el_fov = np.radians(40.), np.radians(20.)
    for Naz, Nel in ((1, 1), (3, 2), (63, 5), (64, 4), (65, 3), (257, 2)):
        for rectification_model in MODELS:
            if rectification_model == "LENSMODEL_LATLON": fx, fy = Naz/az_fov, Nel/el_fov
            else:                                         fx, fy = Naz/2./np.tan(az_fov/2.), Nel/2./np.tan(el_fov/2.)
            fxycxy = np.array((fx, fy, (Naz - 1.)/2. + 0.25, (Nel - 1.)/2. - 0.125))
            models_rectified = [amd.cameramodel(intrinsics=(rectification_model, fxycxy), imagersize=(Naz, Nel), rt_cam_ref=g.rt_cam_ref())
                                for g in geometry]
            maps = amd.rectification_maps((model0, model1), models_rectified)
            assert maps.shape == (2, Nel, Naz, 2)
            checker = chk.rectification_maps_checker(ref_api, (model0, model1), models_rectified)
            chk.compare_map(maps, checker, f"{cameras} {rectification_model} {Naz}x{Nel}")
            assert np.array_equal(maps, amd.rectification_maps((model0, model1), models_rectified))
            with amd.Rectification((model0, model1), models_rectified) as r:
                assert np.array_equal(maps, r.maps())
                assert amd.device_buffers_live() == live + 2
    assert amd.device_buffers_live() == live


def interpolate(map2, q):
    """bilinear interpolation of a (H,W,2) map at the pixels q (N,2)"""
    x0, y0 = np.floor(q[:, 0]).astype(int), np.floor(q[:, 1]).astype(int)
    fx, fy = (q[:, 0] - x0)[:, None], (q[:, 1] - y0)[:, None]
    m = map2.astype(float)
    return (1-fy)*((1-fx)*m[y0, x0] + fx*m[y0, x0+1]) + fy*((1-fx)*m[y0+1, x0] + fx*m[y0+1, x0+1])


@pytest.mark.gpu
@pytest.mark.parametrize("rectification_model", MODELS)
def test_points_through_the_maps_and_their_ranges(amd, ref_api, rectification_model):
    """the points test of the reference's test/test-stereo.py"""
    model0, model1 = pair(amd, RT01)
    models_rectified = amd.rectified_system((model0, model1), **SYSTEM, rectification_model=rectification_model)
    Rt_cam0_rect   = amd.compose_Rt(model0.Rt_cam_ref(), models_rectified[0].Rt_ref_cam())
    Rt01_rectified = amd.compose_Rt(models_rectified[0].Rt_cam_ref(), models_rectified[1].Rt_ref_cam())
    pcam0 = np.array(((1., 2., 12.), (-4., 3., 12.)))
    qcam0 = ref_api.project(pcam0, *model0.intrinsics())
    pcam1 = amd.transform_point_rt(amd.invert_rt(RT01), pcam0)
    qcam1 = ref_api.project(pcam1, *model1.intrinsics())
    prect0 = amd.transform_point_Rt(amd.invert_Rt(Rt_cam0_rect), pcam0)
    prect1 = prect0 - Rt01_rectified[3, :]
    qrect0 = ref_api.project(prect0, *models_rectified[0].intrinsics())
    qrect1 = ref_api.project(prect1, *models_rectified[1].intrinsics())
    Naz, Nel = models_rectified[0].imagersize()

    maps = amd.rectification_maps((model0, model1), models_rectified)
    assert np.abs(interpolate(maps[0], qrect0) - qcam0).max() < 0.1
    assert np.abs(interpolate(maps[1], qrect1) - qcam1).max() < 0.1
    # the same point: the same elevation
    assert np.allclose(qrect0[:, 1], qrect1[:, 1], rtol=0, atol=1e-6)

    disparity = qrect0[:, 0] - qrect1[:, 0]
    ranges = np.linalg.norm(pcam0, axis=-1)
    assert np.allclose(amd.stereo_range(disparity, models_rectified, qrect0=qrect0), ranges, rtol=0, atol=1e-6)
    r = amd.stereo_range(disparity[:1], models_rectified, qrect0=qrect0[0])
    assert r.shape == (1,) and abs(r[0] - ranges[0]) < 2e-6
    r = amd.stereo_range(float(disparity[0]), models_rectified, qrect0=qrect0[0])
    assert np.ndim(r) == 0 and abs(r - ranges[0]) < 2e-6
    assert amd.stereo_range(np.int16(-1), models_rectified, qrect0=qrect0[0], disparity_min=0) == 0

    # dense: an int16 disparity image with one invalid pixel
    disparity_scale = 16
    disparity_dense = np.int16(disparity_scale*np.mean(disparity))*np.ones((Nel, Naz), dtype=np.int16)
    disparity_dense[0, 0] = -1
    r = amd.stereo_range(disparity_dense, models_rectified, disparity_scale=disparity_scale, disparity_min=0)
    assert r.shape == (Nel, Naz) and r.dtype == np.float64
    valid = r[disparity_dense > 0]
    assert np.all(valid > ranges.mean()/2) and np.all(valid < ranges.mean()*2.)
    assert r[0, 0] == 0
    with amd.Rectification((model0, model1), models_rectified) as rectification:
        assert np.array_equal(r, rectification.range(disparity_dense, disparity_scale=disparity_scale, disparity_min=0))

    assert np.allclose(amd.stereo_unproject(disparity, models_rectified, qrect0=qrect0), prect0, rtol=0, atol=1e-6)
    p = amd.stereo_unproject(float(disparity[0]), models_rectified, qrect0=qrect0[0])
    assert p.shape == (3,) and np.allclose(p, prect0[0], rtol=0, atol=1e-6)
    assert np.allclose(amd.stereo_unproject(None, models_rectified, ranges=ranges, qrect0=qrect0), prect0, rtol=0, atol=1e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("rectification_model", MODELS)
def test_range_kernels_against_numpy(amd, rectification_model):
    """a lane an entry, N around the wave and the block; every way a disparity is invalid; the LATLON sine at zero.
    Both sides evaluate the same few operations in double: 1e-12 relative leaves room for the device's sin, cos and
    sqrt being a few ulp from numpy's, and for the division by a sine near zero amplifying none of it (the cases
    that make it EXACTLY zero give 0 on both sides)"""
    fxycxy = np.array((223.4535401, 409.09186572, 81.51526768, 106.6))
    baseline = 3.1685959
    Naz, Nel = 257, 3
    models_rectified = [amd.cameramodel(intrinsics=(rectification_model, fxycxy), imagersize=(Naz, Nel),
                                        rt_cam_ref=(0, 0, 0, -x, 0, 0)) for x in (0., baseline)]
    rng = np.random.default_rng(7)
    for N in (1, 63, 64, 65, 257):
        qrect0 = rng.uniform((0, 0), (Naz - 1, Nel - 1), size=(N, 2))
        disparity = rng.uniform(0.5, 60., size=N)
        disparity[0::7] = 0.                       # no disparity
        disparity[1::7] = -3.                      # negative
        disparity[2::7] = 1.5                      # below the minimum
        disparity[3::7] = 90.                      # above the maximum
        invalid = (disparity <= 0) | (disparity < 2.) | (disparity > 80.)
        want = np.where(invalid, 0., chk.stereo_range_one(disparity, qrect0, rectification_model, fxycxy, baseline))
        got = amd.stereo_range(disparity, models_rectified, qrect0=qrect0, disparity_min=2., disparity_max=80.)
        assert got.shape == (N,)
        assert np.all(got[invalid] == 0)
        assert np.allclose(got, want, rtol=1e-12, atol=0)
        # scaled disparities and scaled bounds say the same
        assert np.array_equal(got, amd.stereo_range(disparity*16, models_rectified, qrect0=qrect0, disparity_scale=16,
                                                    disparity_scaled_min=32., disparity_scaled_max=1280.))
    # disparity == fx az0: the second ray is the rectified forward direction. disparity == pi fx: the LATLON sine is
    # zero to rounding (sin of the double next to pi: 1.2e-16), the range huge: the same huge number on both sides,
    # as both divide the same doubles and a sine is good to an ulp or two there too
    qrect0 = np.array(((200., 1.), (100., 2.)))
    disparity = np.array(((200. - fxycxy[2]), np.pi*fxycxy[0]))
    want = chk.stereo_range_one(disparity, qrect0, rectification_model, fxycxy, baseline)
    got = amd.stereo_range(disparity, models_rectified, qrect0=qrect0)
    assert np.allclose(got, want, rtol=1e-12, atol=0)

    # dense, against the same function: uint16 disparities over the whole imager
    d = rng.integers(0, 900, size=(Nel, Naz)).astype(np.uint16)
    d[0, :5] = (0, 15, 16, 800, 801)
    got = amd.stereo_range(d, models_rectified, disparity_scale=16, disparity_scaled_min=16, disparity_scaled_max=800)
    invalid = (d == 0) | (d < 16) | (d > 800)
    want = np.where(invalid, 0., chk.stereo_range_one(d/16., chk.grid(Naz, Nel), rectification_model, fxycxy, baseline))
    assert np.all(got[invalid] == 0) and got[0, 2] != 0 and got[0, 3] != 0
    assert np.allclose(got, want, rtol=1e-12, atol=0)
