"""match_feature(): template matching between two images.

Without a GPU: apply_homography(), the checker against a brute-force loop and against the reference's own test
(test/test-match-feature.py: it must find the feature), every refusal before any device work, and the host planning
(csrc/match_plan.hpp) as a stand-alone program under the host sanitizers. On the GPU: the reference's test case by case,
the match surface against the checker (tests/match_feature_checker.py: numpy with exact integer sums, no cv2), the
template to the bit, the peak and the subpixel step, batches, and two cameras looking at a textured plane."""
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR
import hostbuild
import match_feature_checker as chk

# the reference's test: some made-up homography with scaling, rotating, skewing and translating
H01 = np.array(((0.7, 0.3, 1.), (-0.4, 0.95, 2.), (3e-5, 4e-6, 1.)))
H10 = np.linalg.inv(H01)
H10_SHIFTED = H10.copy()
H10_SHIFTED[0, 2] += 10.2
H10_SHIFTED[1, 2] -= 20.4
Q0 = np.array((294., 159.))         # the corner of one of the towers
TEMPLATESIZE, RADIUS = (30, 20), 50

TEMPLATES = ((1, 1), (3, 2), (4, 4), (5, 7), (16, 16), (17, 17), (30, 20), (33, 31), (64, 5))
RADII     = (1, 2, 7, 8, 31, 32, 50)
WIDTHS    = (499, 500, 501, 503)


@pytest.fixture(scope="module")
def image():
    return np.load(os.path.join(GOLDEN_DIR, "match_feature_image.npz"))["image"]


def as_dtype(image, dtype):
    if dtype == "uint8":  return image
    if dtype == "uint16": return image.astype(np.uint16)*np.uint16(257)
    return (image/255.).astype(np.float32)


def reference_image1(image, remap):
    """the reference test's image1: (600,500), image seen through H01"""
    return remap(image, chk.apply_homography(H01, chk.pixel_grid(0, 0, 500, 600)).astype(np.float32))


def surface_configs(dtype):
    """(template size, radius, width of image1, first pixel of the template in image1, shift to image0)"""
    out = []
    for i in range(18):
        ts, r, xmod = TEMPLATES[i % 9], RADII[i % 7], (i//4) % 4
        # the cut begins at tmin - r: at x = xmod (mod 4), so that every byte offset into a word is met
        out.append((ts, r, WIDTHS[i % 4], (200 + (xmod - (200 - r)) % 4, 180), (3.25, 2.5)))
    # the search window clipped at the left, the top, the right, the bottom of image1 (482 rows, 500 columns)
    for tmin, shift in (((2, 200), (3.25, 2.5)), ((250, 1), (3.25, 2.5)), ((494, 200), (-3.25, -2.5)), ((250, 473), (-3.25, -2.5))):
        out.append(((5, 7), 8, 500, tmin, shift))
    # more than 64 kB of LDS a workgroup
    if dtype == "float32": out.append(((120, 100), 2, 500, (150, 150), (3.25, 2.5)))
    return out


def adjacent_or_equal(a, b):
    return (a == b) | (np.nextafter(b, a) == a)


# ------------------------------------------------------------------------------------------------ without a GPU ---
def test_apply_homography(amd):
    rng = np.random.default_rng(0)
    q = rng.uniform(-100, 100, size=(4, 5, 2))
    H = H10
    x, y = q[..., 0], q[..., 1]
    d = (H[2, 0]*x + H[2, 1]*y) + H[2, 2]
    expected = np.stack((((H[0, 0]*x + H[0, 1]*y) + H[0, 2])/d, ((H[1, 0]*x + H[1, 1]*y) + H[1, 2])/d), axis=-1)
    assert np.array_equal(amd.apply_homography(H, q), expected)
    assert amd.apply_homography(H, q[0, 0]).shape == (2,) and np.array_equal(amd.apply_homography(H, q[0, 0]), expected[0, 0])
    # a homography per pixel
    Hs = np.stack([np.eye(3)*s for s in (1., 2., 3., 4., 5.)]) + rng.uniform(-.1, .1, size=(5, 3, 3))
    out = amd.apply_homography(Hs, q)
    assert out.shape == (4, 5, 2)
    for j in range(5):
        assert np.array_equal(out[:, j], amd.apply_homography(Hs[j], q[:, j]))
    assert np.allclose(amd.apply_homography(H01, amd.apply_homography(H10, q)), q, rtol=0, atol=1e-9)
    with pytest.raises(Exception, match="H must have shape"): amd.apply_homography(np.eye(2), q)
    with pytest.raises(Exception, match="q must have shape"): amd.apply_homography(H, np.zeros((3,)))
    assert (amd.TM_SQDIFF, amd.TM_SQDIFF_NORMED, amd.TM_CCORR, amd.TM_CCORR_NORMED, amd.TM_CCOEFF, amd.TM_CCOEFF_NORMED) == (0, 1, 2, 3, 4, 5)


@pytest.mark.parametrize("method", chk.METHODS)
def test_checker_against_brute_force(method):
    rng = np.random.default_rng(1)
    cut, template = rng.integers(0, 256, size=(6, 7), dtype=np.uint8), rng.integers(0, 256, size=(2, 3), dtype=np.uint8)
    z = chk.matchoutput(cut, template, method)
    assert z.shape == (5, 5) and z.dtype == np.float32
    assert np.array_equal(z, chk.matchoutput_bruteforce(cut, template, method))
    # an all-zero template: a flat surface
    flat = chk.matchoutput(cut, template*0, method)
    if method in (chk.TM_SQDIFF_NORMED, chk.TM_CCORR_NORMED, chk.TM_CCOEFF_NORMED, chk.TM_CCORR, chk.TM_CCOEFF):
        assert np.all(flat == flat[0, 0]) and chk.optimum(flat, method) == (0, 0)


@pytest.mark.parametrize("method", (chk.TM_CCOEFF_NORMED, chk.TM_SQDIFF_NORMED, chk.TM_CCORR_NORMED, chk.TM_SQDIFF))
def test_checker_finds_the_reference_tests_feature(image, method):
    """measured: 0.049, 0.014, 0.016, 0.026 px"""
    image1 = reference_image1(image, chk.remap)
    q1, d = chk.match(image, image1, Q0, H10_SHIFTED, TEMPLATESIZE, RADIUS, method)
    err = np.linalg.norm(q1 - chk.apply_homography(H10, Q0))
    print(f"method {method}: {err:.3f} px")
    assert err < 0.1


def test_refusals_before_any_device_work(amd, image, monkeypatch):
    """the reference's refusals, with its messages, raised before anything is made on the device"""
    def no_device(*a, **k): raise AssertionError("device work before the refusal")
    monkeypatch.setattr(amd.stereo.FeatureMatcher, "__init__", no_device)
    image1 = np.zeros((600, 500), dtype=np.uint8)
    kw = dict(search_radius1=RADIUS, template_size1=TEMPLATESIZE)
    with pytest.raises(Exception, match="Exactly one of \\(q1_estimate,H10\\) must be given"):
        amd.match_feature(image, image1, Q0, **kw)
    with pytest.raises(Exception, match="Exactly one of \\(q1_estimate,H10\\) must be given"):
        amd.match_feature(image, image1, Q0, H10=H10, q1_estimate=Q0, **kw)
    with pytest.raises(Exception, match="template_size1 must be an interable of length 2 OR a scalar"):
        amd.match_feature(image, image1, Q0, H10=H10, search_radius1=RADIUS, template_size1=(1, 2, 3))
    with pytest.raises(Exception, match="Each element of template_size1 must be an integer > 0"):
        amd.match_feature(image, image1, Q0, H10=H10, search_radius1=RADIUS, template_size1=(30, 0))
    with pytest.raises(Exception, match="Each element of template_size1 must be an integer > 0"):
        amd.match_feature(image, image1, Q0, H10=H10, search_radius1=RADIUS, template_size1=30.)
    with pytest.raises(Exception, match="ONLY grayscale images of shape \\(H,W\\)"):
        amd.match_feature(np.zeros((10, 10, 3), dtype=np.uint8), image1, Q0, H10=H10, **kw)
    with pytest.raises(Exception, match="ONLY grayscale images of shape \\(H,W\\)"):
        amd.match_feature(image, np.zeros((10, 10, 3), dtype=np.uint8), Q0, H10=H10, **kw)
    with pytest.raises(Exception, match="Too close to the .* edge in image1"):
        amd.match_feature(image, image1, Q0, H10=H10_SHIFTED, search_radius1=RADIUS, template_size1=(5000, 5000))
    with pytest.raises(Exception, match="Too close to the left edge in image0"):
        amd.match_feature(image, image1, np.array((5., 159.)), q1_estimate=np.array((250., 300.)), **kw)
    with pytest.raises(Exception, match="visualize"):
        amd.match_feature(image, image1, Q0, H10=H10, visualize=True, **kw)
    with pytest.raises(Exception, match="same dtype"):
        amd.match_feature(image, image1.astype(np.float32), Q0, H10=H10, **kw)
    with pytest.raises(Exception, match="method must be one of"):
        amd.match_feature(image, image1, Q0, H10=H10, method=6, **kw)
    # (what is in order goes on to the device)
    with pytest.raises(AssertionError, match="device work"):
        amd.match_feature(image, image1, Q0, H10=H10_SHIFTED, **kw)


def test_match_plan_under_the_host_sanitizers():
    """csrc/match_plan.hpp driven by a stand-alone program with its own main, built with ASan and UBSan"""
    hostbuild.assert_prints_ok("match_plan_check")


# --------------------------------------------------------------------------------------------------- on the GPU ---
@pytest.fixture(scope="module")
def image1_reference(amd, image):
    return reference_image1(image, amd.transform_image)


@pytest.mark.gpu
def test_the_reference_test_case_by_case(amd, image, image1_reference):
    image1, q1_true = image1_reference, chk.apply_homography(H10, Q0)
    assert image1.shape == (600, 500)
    kw = dict(H10=H10_SHIFTED, template_size1=TEMPLATESIZE)
    results = {}
    for method in (amd.TM_CCOEFF_NORMED, amd.TM_SQDIFF_NORMED):
        q1, d = amd.match_feature(image, image1, Q0, search_radius1=RADIUS, method=method, **kw)
        print(f"method {method}: {np.linalg.norm(q1 - q1_true):.3f} px")
        assert np.all(np.abs(q1 - q1_true) < 0.1)
        assert np.allclose(q1, d['matchoutput_optimum_subpixel_at'] + d['qshift_image1_matchoutput'], rtol=0, atol=1e-12)
        assert d['matchoutput_image'].dtype == np.float32 and d['matchoutput_image'].shape == (2*RADIUS + 1, 2*RADIUS + 1)
        results[method] = q1
    # an out-of-bounds search radius looks at the whole image
    q1, d = amd.match_feature(image, image1, Q0, search_radius1=1000, method=amd.TM_CCOEFF_NORMED, **kw)
    assert np.all(np.abs(q1 - q1_true) < 0.1)
    assert np.allclose(q1, results[amd.TM_CCOEFF_NORMED], rtol=0, atol=1e-9)
    assert d['matchoutput_image'].shape == (600 - 20 + 1, 500 - 30 + 1)
    # a failing correlation returns None
    q1, d = amd.match_feature(image*0, image1, Q0, search_radius1=RADIUS, method=amd.TM_CCOEFF_NORMED, **kw)
    assert q1 is None and np.all(d['matchoutput_image'] == 0) and np.all(d['template'] == 0)
    # a too-big template size throws an exception
    with pytest.raises(Exception, match="Too close to the"):
        amd.match_feature(image*0, image1, Q0, H10=H10_SHIFTED, search_radius1=RADIUS, template_size1=(5000, 5000),
                          method=amd.TM_CCOEFF_NORMED)
    # the default method is TM_CCORR_NORMED
    q1, d = amd.match_feature(image, image1, Q0, search_radius1=RADIUS, **kw)
    q1n, dn = amd.match_feature(image, image1, Q0, search_radius1=RADIUS, method=amd.TM_CCORR_NORMED, **kw)
    assert np.array_equal(q1, q1n) and np.array_equal(d['matchoutput_image'], dn['matchoutput_image'])
    assert np.all(np.abs(q1 - q1_true) < 0.1)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ("uint8", "uint16", "float32"))
def test_surface_against_the_checker(amd, image, dtype):
    """Every method's surface equals the checker's float32 or is the adjacent float32, at most 1e-3 of the entries
    being unequal; the checker is fed the device's template, so this is about the correlation alone. And q1 against
    the checker's subpixel step on the device's own surface: 1e-9 px."""
    image0 = as_dtype(image, dtype)
    unequal, entries, worst_q = np.zeros(6), np.zeros(6), 0.
    for ts, r, width, tmin, shift in surface_configs(dtype):
        image1 = np.ascontiguousarray(image0[:, :width])
        q1e = np.array(tmin) + (np.array(ts) - 1.)/2.
        q0  = q1e + shift
        with amd.FeatureMatcher(image0, image1) as matcher:
            sums = None
            for method in chk.METHODS:
                q1, status, diag = matcher.match(q0[np.newaxis], q1_estimate=q1e, search_radius1=r, template_size1=ts,
                                                 method=method, diagnostics=True)
                d = diag[0]
                assert status[0] in (0, 1, 2)
                wtmin, qmin, qmax = chk.window(q1e, ts, r, image1.shape)
                assert tuple(wtmin) == tuple(tmin)
                if sums is None:
                    template = d['template']
                    assert template.shape == (ts[1], ts[0]) and template.dtype == image0.dtype
                    sums = chk.sums(image1[qmin[1]:qmax[1]+1, qmin[0]:qmax[0]+1], template)
                    if dtype == "float32" and ts != (1, 1):
                        # no comparison rests on a cancelled denominator
                        IT, SI, SI2, ST, ST2, N = sums
                        assert np.all(SI2 - SI*SI/N >= 1e-6*SI2) and ST2 - ST*ST/N >= 1e-6*ST2
                else:
                    assert np.array_equal(d['template'], template)
                z = chk.score(method, *sums)
                assert d['matchoutput_image'].shape == z.shape and d['matchoutput_image'].dtype == np.float32
                ok = adjacent_or_equal(d['matchoutput_image'], z)
                assert np.all(ok), (ts, r, width, tmin, method, np.abs(d['matchoutput_image'] - z).max())
                unequal[method] += np.count_nonzero(d['matchoutput_image'] != z)
                entries[method] += z.size
                # the peak and the subpixel step, on the device's own surface
                ox, oy = chk.optimum(d['matchoutput_image'], method)
                s = chk.subpixel(d['matchoutput_image'], ox, oy)
                if s is None:
                    assert status[0] == 1 and np.all(np.isnan(q1))
                elif status[0] == 0:
                    q1_chk = np.array((ox + s[0], oy + s[1])) + (qmin + q1e - tmin)
                    worst_q = max(worst_q, np.abs(q1[0] - q1_chk).max())
                    z9 = d['matchoutput_image'][oy-1:oy+2, ox-1:ox+2].astype(float)
                    assert np.abs(d['matchoutput_optimum_subpixel'] - s[2]) <= 1e-9*max(1., np.abs(z9).max())
                else:
                    assert status[0] == 2 and not np.all(np.isfinite(s))
    print(f"{dtype}: share of entries that are the adjacent float32, by method: {unequal/entries}; "
          f"worst q1 against the checker's subpixel step: {worst_q:.3g} px")
    assert np.all(unequal <= 1e-3*entries)
    assert worst_q < 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize("ts", ((1, 1), (3, 2), (30, 20)))
@pytest.mark.parametrize("form", ("translation", "homography"))
def test_template_to_the_bit(amd, image, image1_reference, ts, form):
    """diagnostics['template'] is transform_image(image0, float32(the numpy map))"""
    kw = dict(q1_estimate=chk.apply_homography(H10_SHIFTED, Q0) + (0.3, -0.2)) if form == "translation" else dict(H10=H10_SHIFTED)
    with amd.FeatureMatcher(image, image1_reference) as matcher:
        q1, status, diag = matcher.match(Q0[np.newaxis], search_radius1=5, template_size1=ts, diagnostics=True, **kw)
    if form == "translation":
        q1e = kw["q1_estimate"]
        H10_used = np.array(((1., 0., q1e[0] - Q0[0]), (0., 1., q1e[1] - Q0[1]), (0., 0., 1.)))
    else:
        q1e, H10_used = chk.apply_homography(H10_SHIFTED, Q0), H10_SHIFTED
    tmin, qmin, qmax = chk.window(q1e, ts, 5, image1_reference.shape)
    mapxy = chk.template_map(np.linalg.inv(H10_used), tmin, ts)
    assert status[0] in (0, 1, 2)
    assert np.array_equal(diag[0]['template'], amd.transform_image(image, mapxy))
    assert np.array_equal(diag[0]['template'], chk.remap(image, mapxy))


def noise_image(seed=3, shape=(120, 160)):
    return np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("method", (chk.TM_CCORR_NORMED, chk.TM_SQDIFF))
def test_first_of_two_equal_optima_wins(amd, method):
    A = noise_image()
    pattern = A[50:61, 70:83].copy()            # (11,13): the template, cut out of image0 at (70,50)
    image1 = noise_image(seed=4)
    image1[40:51, 40:53] = pattern
    image1[40:51, 90:103] = pattern             # the same row, further right: later in row-major order
    image1[70:81, 30:43] = pattern              # and a later row, further left
    q0 = np.array((76., 55.))
    q1, d = amd.match_feature(A, image1, q0, q1_estimate=np.array((70., 60.)), search_radius1=40, template_size1=(13, 11),
                              method=method)
    z = d['matchoutput_image']
    assert np.array_equal(d['template'], pattern)
    qmin = np.array((64 - 40, 55 - 40))
    best = 1. if method == chk.TM_CCORR_NORMED else 0.
    for x, y in ((40, 40), (90, 40), (30, 70)):
        assert z[y - qmin[1], x - qmin[0]] == best
    assert np.count_nonzero(z == best) == 3
    assert tuple(np.round(d['matchoutput_optimum_subpixel_at']).astype(int)) == (40 - qmin[0], 40 - qmin[1])
    assert np.all(np.abs(q1 - (46., 45.)) < 0.5)


@pytest.mark.gpu
@pytest.mark.parametrize("edge", ((-1, 0), (1, 0), (0, -1), (0, 1)))
def test_an_optimum_on_the_edge_is_status_1(amd, edge):
    A, r = noise_image(), 6
    q0 = np.array((80., 60.))
    with amd.FeatureMatcher(A, A) as matcher:
        # the estimate is off by exactly the radius: the match is in the first or last column or row of the surface
        q1, status, diag = matcher.match(q0[np.newaxis], q1_estimate=q0 - r*np.array(edge, dtype=float), search_radius1=r,
                                         template_size1=(9, 9), method=chk.TM_CCOEFF_NORMED, diagnostics=True)
        z = diag[0]['matchoutput_image']
        assert z.shape == (2*r + 1, 2*r + 1)
        assert chk.optimum(z, chk.TM_CCOEFF_NORMED) == (r + r*edge[0], r + r*edge[1])
        assert status[0] == 1 and np.all(np.isnan(q1)) and 'matchoutput_optimum_subpixel_at' not in diag[0]
        # one pixel less: found
        q1, status = matcher.match(q0[np.newaxis], q1_estimate=q0 - (r - 1)*np.array(edge, dtype=float), search_radius1=r,
                                   template_size1=(9, 9), method=chk.TM_CCOEFF_NORMED)
        # (the neighbours of an exact match in white noise are noise: the fit stays within the pixel, no closer)
        assert status[0] == 0 and np.all(np.abs(q1[0] - q0) < 0.5)
    q1, d = amd.match_feature(A, A, q0, q1_estimate=q0 - r*np.array(edge, dtype=float), search_radius1=r, template_size1=(9, 9))
    assert q1 is None and set(d.keys()) == {'matchoutput_image', 'template'}


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.gpu
@pytest.mark.parametrize("N", (1, 2, 63, 65))
def test_a_batch_is_its_rows(amd, N):
    """mixed statuses in one call: every row is its own N = 1 call to the bit, the same bits twice, the one-shot call
    gives the same, and every buffer is given back"""
    live0 = amd.device_buffers_live()
    A, r, ts = noise_image(), 6, (9, 7)
    rng = np.random.default_rng(N)
    q0  = rng.uniform((40, 30), (120, 90), size=(N, 2))
    q1e = q0 + rng.uniform(-3, 3, size=(N, 2))
    expected = np.zeros((N,), dtype=int)
    for i in range(N):
        kind = (i + N) % 4
        if   kind == 1: q1e[i], expected[i] = np.round(q0[i]) + (r, 0), 1       # the match in the first column
        elif kind == 2: q1e[i], expected[i] = (158., 60.), 3                    # the template sticks out of image1
        elif kind == 3: q0[i],  expected[i] = (-40., 60.), 4                    # ... of image0
    q0[expected == 1] = np.round(q0[expected == 1])
    kw = dict(search_radius1=r, template_size1=ts, method=chk.TM_CCOEFF_NORMED)
    with amd.FeatureMatcher(A, A) as matcher:
        assert amd.device_buffers_live() > live0
        q1, status, diag = matcher.match(q0, q1_estimate=q1e, diagnostics=True, **kw)
        assert np.array_equal(status, expected), (status, expected)
        assert np.all(np.isnan(q1[status != 0])) and np.all(np.abs(q1[status == 0] - q0[status == 0]) < 0.5)
        q1_again, status_again = matcher.match(q0, q1_estimate=q1e, **kw)
        assert same(q1, q1_again) and np.array_equal(status, status_again)
        # translation-only homographies say the same
        H = np.tile(np.eye(3), (N, 1, 1)); H[:, :2, 2] = q1e - q0
        q1_H, status_H = matcher.match(q0, H10=H, **kw)
        assert same(q1, q1_H) and np.array_equal(status, status_H)
        for i in range(N):
            q1_i, status_i, diag_i = matcher.match(q0[i:i+1], q1_estimate=q1e[i], diagnostics=True, **kw)
            assert same(q1_i[0], q1[i]) and status_i[0] == status[i]
            assert diag_i[0].keys() == diag[i].keys()
            for k in diag[i]: assert same(np.asarray(diag_i[0][k]), np.asarray(diag[i][k])), (i, k)
    assert amd.device_buffers_live() == live0
    # the one-shot call, on the rows of each kind that come first
    for i in range(min(N, 4)):
        if status[i] in (3, 4):
            with pytest.raises(Exception, match=f"Too close to the .* edge in image{1 if status[i] == 3 else 0}"):
                amd.match_feature(A, A, q0[i], q1_estimate=q1e[i], **kw)
            continue
        q1_one, d = amd.match_feature(A, A, q0[i], q1_estimate=q1e[i], **kw)
        assert (q1_one is None) == (status[i] != 0)
        if q1_one is not None: assert np.array_equal(q1_one, q1[i])
        for k in d: assert same(np.asarray(d[k]), np.asarray(diag[i][k])), (i, k)
    assert amd.device_buffers_live() == live0


@pytest.mark.gpu
def test_two_cameras_looking_at_a_plane(amd, image):
    """Two pinhole cameras look at the plane z = 0 of the reference frame, which carries the fixture as its texture. H10
    is made by the recipe of the reference's docstring; q1 lands within 0.1 px of the true projection"""
    # the texture: what a camera 5 m in front of the plane, looking straight at it, sees
    D = 5.
    texture = amd.cameramodel(intrinsics=('LENSMODEL_PINHOLE', np.array((500., 500., 360.5, 240.5))), imagersize=(722, 482),
                              rt_cam_ref=np.array((0., 0., 0., 0., 0., D)))
    def camera(r, position, f):
        R = amd.R_from_r(np.array(r))
        return amd.cameramodel(intrinsics=('LENSMODEL_PINHOLE', np.array((f, f, 320., 230.))), imagersize=(640, 460),
                               rt_cam_ref=np.concatenate((r, -R @ np.array(position))))
    model0 = camera((0.02, -0.06, 0.01),  (-0.5,  0.1, -5.2), 560.)
    model1 = camera((-0.03, 0.07, -0.04), ( 0.6, -0.1, -4.9), 540.)
    images = [amd.transform_image(image, amd.image_transformation_map(texture, m, plane_n=np.array((0., 0., 1.)), plane_d=D))
              for m in (model0, model1)]

    def xy_from_q(model, q):
        v, dv_dq, _ = amd.unproject(q, *model.intrinsics(), get_gradients=True)
        t_ref_cam, R_ref_cam = model.Rt_ref_cam()[3, :], model.Rt_ref_cam()[:3, :]
        vref = R_ref_cam @ v
        k  = -t_ref_cam[2]/vref[2]
        xy = t_ref_cam[:2] + k*vref[:2]
        H_xy_vref = np.array(((-t_ref_cam[2], 0, xy[0] - k*vref[0]), (0, -t_ref_cam[2], xy[1] - k*vref[1]), (0, 0, 1)))
        H_v_q = np.concatenate((dv_dq, (v - dv_dq @ q)[:, np.newaxis]), axis=-1)
        return xy, H_xy_vref @ R_ref_cam @ H_v_q

    # the corner of the tower, as camera 0 sees it
    xy_tower = (Q0 - (360.5, 240.5))/500.*D
    q0 = amd.project(amd.transform_point_Rt(model0.Rt_cam_ref(), np.array((*xy_tower, 0.))), *model0.intrinsics())
    xy, H_xy_q0 = xy_from_q(model0, q0)
    assert np.allclose(xy, xy_tower, rtol=0, atol=1e-9)
    q1_true = amd.project(amd.transform_point_Rt(model1.Rt_cam_ref(), np.array((*xy, 0.))), *model1.intrinsics())
    _, H_xy_q1 = xy_from_q(model1, q1_true)
    H10 = np.linalg.solve(H_xy_q1, H_xy_q0)
    assert np.allclose(amd.apply_homography(H10, q0), q1_true, rtol=0, atol=1e-6)

    # the estimate is off: the matcher finds what the geometry says
    H10_off = H10.copy()
    H10_off[:2, 2] += (7.3, -4.6)
    for method in (None, amd.TM_CCOEFF_NORMED):
        # (template_size1 = 17: the value of the reference's docstring, where this recipe comes from)
        q1, d = amd.match_feature(images[0], images[1], q0, H10=H10_off, search_radius1=20, template_size1=17, method=method)
        print(f"method {method}: {np.linalg.norm(q1 - q1_true):.3f} px")
        assert np.all(np.abs(q1 - q1_true) < 0.1)
