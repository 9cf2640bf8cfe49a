"""projection_diff() / implied_Rt10__from_unprojections() / sample_imager() / sample_imager_unproject()
(mrcal/model_analysis.py:27-395, 1520-1928; mrcal/utils.py:268-437) with the fit on the device
(csrc/projection_diff.hip).

The checker restates the reference's residual and Jacobian (model_analysis.py:223-281) in numpy and minimises them as
the reference does: scipy.optimize.least_squares(method='dogbox', loss='huber', f_scale=(5 deg)^2, gtol=eps) from its
random start of 1e-5, for seeds 0, 1, 2. Vectors and pixels come from the reference's compiled code (ref_api), R and
dR/dr from its mrcal_R_from_r_full.

Bounds the tests set themselves:
  - cost: F_device <= F_checker (1 + 1e-6) + 32 eps sum w_i |x_i|, both F computed here in numpy from the returned
    transformation. One-sided; the last term is the rounding of 1 - cos in the sum: x_i = 2 (1 - c_i) w_i carries an
    absolute error of a few eps w_i, and F = 1/2 sum x_i^2 moves by sum |x_i| times that.
  - a model against itself: the fit starts at rt = 0, where the cost is already at the rounding of 1 - cos, and stays
    there: Rt10 is the identity exactly, and difflen is the round trip of the unprojection (its acceptance test is
    |q(v) - q|^2/2 <= 1e-4; in practice Newton ends far below): < 1e-3 px."""
import os
import numpy as np
import pytest

from conftest import ROOT, relative_error
from test_projection_uncertainty import ref_R_from_r

GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")
C_HUBER = (5.*np.pi/180.)**2
EPS = np.finfo(float).eps
SEEDS = (0, 1, 2)
RT_TRUE = np.array((0.004, -0.006, 0.003, 0.01, -0.02, 0.015))


# ------------------------------------------------------------- checker ---
def flatten_inputs(q0, p0, v1, weights, focus_center=(0., 0.), focus_radius=1e8):
    """the reference's flattening, cleaning and focus cut (model_analysis.py:174-221): p0 (M,n,3), v1 (n,3), w (M,n)"""
    q0 = np.asarray(q0, dtype=float).reshape(-1, 2)
    N = q0.shape[0]
    p0 = np.array(p0, dtype=float).reshape(-1, N, 3)
    v1 = np.array(v1, dtype=float).reshape(N, 3)
    w = np.ones(p0.shape[:-1]) if weights is None else np.array(weights, dtype=float).reshape(-1, N)
    w[~np.isfinite(w)] = 0.
    bad = ~np.isfinite(p0)
    p0[bad] = 0.
    w[bad.any(axis=-1)] = 0.
    bad = ~np.isfinite(v1)
    v1[bad] = 0.
    w[:, bad.any(axis=-1)] = 0.
    i = np.sum((q0 - np.asarray(focus_center, dtype=float))**2, axis=-1) < focus_radius*focus_radius
    if np.count_nonzero(i) < 3:
        raise Exception("Focus region contained too few points")
    return p0[:, i], v1[i], w[:, i]


def residual_of_Rt(R, t, p0, v1, w, atinfinity):
    """x (M,n) of the reference's cost at a transformation given as a matrix"""
    p = np.einsum("ij,mnj->mni", R, p0)
    if atinfinity:
        return 2.*(1. - np.sum(p*v1, axis=-1))*w
    p = p + t
    return 2.*(1. - np.sum(p*v1, axis=-1)/np.linalg.norm(p, axis=-1))*w


def residual_jacobian(ref, rt, p0, v1, w, atinfinity):
    """x (M n,) and J (M n, 3 or 6): residual_jacobian_r() / residual_jacobian_rt() of the reference"""
    R, dR = ref_R_from_r(ref, rt[:3])
    # d(R p0)_i/dr_k = sum_j dR[i,j,k] p0_j
    drp = np.einsum("ijk,mnj->mnik", dR, p0)
    p = np.einsum("ij,mnj->mni", R, p0)
    if atinfinity:
        inner = np.sum(p*v1, axis=-1)
        x = 2.*(1. - inner)*w
        J = -2.*np.einsum("ni,mnik->mnk", v1, drp)*w[..., None]
        return x.ravel(), J.reshape(-1, 3)
    p = p + rt[3:]
    dp = np.concatenate((drp, np.broadcast_to(np.eye(3), drp.shape)), axis=-1)     # (M,n,3,6)
    mag = np.linalg.norm(p, axis=-1)
    inner = np.sum(p*v1, axis=-1)
    x = 2.*(1. - inner/mag)*w
    dmag = np.einsum("mni,mnik->mnk", p, dp)/mag[..., None]
    dinner = np.einsum("ni,mnik->mnk", v1, dp)
    J = 2.*(inner[..., None]*dmag - mag[..., None]*dinner)/(mag*mag)[..., None]*w[..., None]
    return x.ravel(), J.reshape(-1, 6)


def huber_cost(x):
    z = (np.asarray(x)/C_HUBER)**2
    return 0.5*C_HUBER*C_HUBER*np.sum(np.where(z <= 1., z, 2.*np.sqrt(z) - 1.))


def checker_fit(ref, p0, v1, w, atinfinity, seed):
    """rt (6,) as the reference finds it (model_analysis.py:330-395); t = 0 at infinity"""
    import scipy.optimize
    n = 3 if atinfinity else 6
    start = np.random.RandomState(seed).random_sample(n)*1e-5
    cache = {}
    def both(rt):
        key = rt.tobytes()
        if cache.get("key") != key:
            cache["key"] = key
            cache["x"], cache["J"] = residual_jacobian(ref, np.concatenate((rt, np.zeros(6 - n))), p0, v1, w, atinfinity)
        return cache
    res = scipy.optimize.least_squares(lambda rt: both(rt)["x"], start, jac=lambda rt: both(rt)["J"], method="dogbox",
                                       loss="huber", f_scale=C_HUBER, gtol=EPS)
    return np.concatenate((res.x, np.zeros(6 - n)))


def cost_of_rt(ref, rt, p0, v1, w, atinfinity):
    return huber_cost(residual_of_Rt(ref_R_from_r(ref, rt[:3])[0], rt[3:], p0, v1, w, atinfinity))


def assert_cost_no_worse(ref, Rt10, p0, v1, w, atinfinity, seeds=SEEDS, label=""):
    """condition 2 of the module's docstring, for each seed; returns the worst F_device/F_checker - 1"""
    x = residual_of_Rt(Rt10[:3], Rt10[3], p0, v1, w, atinfinity)
    F = huber_cost(x)
    slack = 32.*EPS*np.sum(np.abs(x))
    worst = -np.inf
    for seed in seeds:
        Fc = cost_of_rt(ref, checker_fit(ref, p0, v1, w, atinfinity, seed), p0, v1, w, atinfinity)
        print(f"{label} seed {seed}: F device {F:.17g} checker {Fc:.17g} ratio-1 {F/Fc - 1.:.3g} slack {slack:.3g}")
        worst = max(worst, F/Fc - 1.)
        assert F <= Fc*(1. + 1e-6) + slack, (label, seed, F, Fc, slack)
    return worst


def vector_grid(Nw=30, Nh=17):
    """q0 (Nh,Nw,2) on a 3000 x 1700 imager and unit vectors (Nh,Nw,3) of a wide pinhole view of it"""
    q0 = np.stack(np.meshgrid(np.linspace(0., 2999., Nw), np.linspace(0., 1699., Nh)), axis=-1)
    v = np.concatenate(((q0 - (1499.5, 849.5))/1250., np.ones(q0.shape[:-1] + (1,))), axis=-1)
    return q0, v/np.linalg.norm(v, axis=-1, keepdims=True)


def transformed(ref, rt, p0):
    p = np.einsum("ij,...j->...i", ref_R_from_r(ref, rt[:3])[0], p0) + rt[3:]
    return p/np.linalg.norm(p, axis=-1, keepdims=True)


def rt_of(amd, Rt10):
    return amd.rt_from_Rt(Rt10)


# ------------------------------------------------------- without a GPU ---
def test_sample_imager(amd):
    q = amd.sample_imager(7, 5, 640, 480)
    assert q.shape == (5, 7, 2) and q.flags["C_CONTIGUOUS"]
    assert np.array_equal(q[0, 0], (0., 0.)) and np.array_equal(q[-1, -1], (639., 479.))
    assert np.array_equal(q[0, :, 0], np.linspace(0, 639, 7)) and np.array_equal(q[:, 0, 1], np.linspace(0, 479, 5))
    assert (q[:, :, 0] == q[:1, :, 0]).all() and (q[:, :, 1] == q[:, :1, 1]).all()
    assert amd.sample_imager(60, None, 6000, 3376).shape == (int(round(3376/6000*60)), 60, 2)
    assert amd.sample_imager(50, None, 4000, 2200).shape == (28, 50, 2)


def _pinhole(amd, W=640, H=480, f=500.):
    return amd.cameramodel(intrinsics=("LENSMODEL_PINHOLE", np.array((f, f, (W - 1)/2., (H - 1)/2.))), imagersize=(W, H))


def _cahvore(amd, E=(0.01, 0.02, 0.03), W=640, H=480):
    intr = np.array((500., 500., (W - 1)/2., (H - 1)/2., 0.01, -0.02, 0.03, 0.001, -0.002) + tuple(E))
    return amd.cameramodel(intrinsics=("LENSMODEL_CAHVORE_linearity=0.37", intr), imagersize=(W, H))


def test_refusals_before_any_device_work(amd, monkeypatch):
    """the reference's refusals, with its messages, raised before anything is made on the device"""
    import mrcal_amd.resident as resident
    import mrcal_amd.model_analysis as ma
    def no_device(*a, **k): raise AssertionError("device work before the refusal")
    monkeypatch.setattr(resident.Problem, "__init__", no_device)
    monkeypatch.setattr(ma._DiffContext, "__init__", no_device)
    monkeypatch.setattr(ma, "_implied_rt10", no_device)
    monkeypatch.setattr(ma.ProjectionUncertainty, "__init__", no_device)
    monkeypatch.setattr(amd._api, "unproject", no_device)
    monkeypatch.setattr(amd._api, "project", no_device)
    m = _pinhole(amd)
    with pytest.raises(Exception, match="At least 2 models are required to compute the diff"):
        amd.projection_diff((m,))
    with pytest.raises(Exception, match="A given implied_Rt10 is currently supported ONLY if exactly 2 models are being compared"):
        amd.projection_diff((m, m, m), implied_Rt10=amd.identity_Rt())
    with pytest.raises(Exception, match="The diff function needs all the imager dimensions to match"):
        amd.projection_diff((m, _pinhole(amd, W=641)), use_uncertainties=False)
    with pytest.raises(Exception, match="Model 1 is noncentral, so I can only evaluate the diff at infinity"):
        amd.projection_diff((m, _cahvore(amd)), distance=3., use_uncertainties=False)
    with pytest.raises(Exception, match="I have a noncentral model. No usable uncertainties for those yet"):
        amd.projection_diff((_cahvore(amd), m), use_uncertainties=True)
    with pytest.raises(Exception, match="implied_Rt10 must have shape"):
        amd.projection_diff((m, m), implied_Rt10=np.eye(3))
    # (a CAHVORE model that is central already is no reason to refuse: it goes on to the device)
    with pytest.raises(AssertionError, match="device work"):
        amd.projection_diff((m, _cahvore(amd, E=(0., 0., 0.))), distance=3., use_uncertainties=False)


def test_input_shapes_refused(amd):
    q0, v = vector_grid(6, 4)
    with pytest.raises(Exception, match="v1 must have shape"):
        amd.implied_Rt10__from_unprojections(q0, v, v[:3])
    with pytest.raises(Exception, match="p0 must have shape"):
        amd.implied_Rt10__from_unprojections(q0, v[:3], v)
    with pytest.raises(Exception, match="weights must have the shape"):
        amd.implied_Rt10__from_unprojections(q0, v, v, weights=np.ones((3, 6)))


@pytest.mark.parametrize("atinfinity", (True, False))
def test_checker_jacobian_against_central_differences(ref_api, atinfinity):
    q0, v0 = vector_grid(7, 5)
    rng = np.random.RandomState(3)
    p0 = v0[None]*np.array((1., 5.))[:, None, None, None] if not atinfinity else v0[None]
    v1 = transformed(ref_api, RT_TRUE*3., v0 if atinfinity else v0*2.)
    w = 0.5 + rng.random_sample(p0.shape[:-1])
    p0, v1, w = flatten_inputs(q0, p0, v1, w)
    n = 3 if atinfinity else 6
    rt = np.concatenate((rng.random_sample(n)*1e-2, np.zeros(6 - n)))
    x, J = residual_jacobian(ref_api, rt, p0, v1, w, atinfinity)
    assert np.allclose(x, residual_of_Rt(ref_R_from_r(ref_api, rt[:3])[0], rt[3:], p0, v1, w, atinfinity).ravel(), rtol=0, atol=1e-15)
    h = 1e-6
    for k in range(n):
        d = np.zeros(6); d[k] = h
        Jk = (residual_jacobian(ref_api, rt + d, p0, v1, w, atinfinity)[0] -
              residual_jacobian(ref_api, rt - d, p0, v1, w, atinfinity)[0])/(2.*h)
        # (central differences of x ~ 1e-4: truncation h^2 |x'''| ~ 1e-12, rounding eps |x|/h ~ 1e-14)
        assert np.abs(Jk - J[:, k]).max() < 1e-9*max(1., np.abs(J[:, k]).max())


# ------------------------------------------------------------------ GPU ---
@pytest.fixture(scope="module")
def misfit_case(ref_api):
    """the 30 x 17 grid with a smooth misfit of 1e-4, a region of gross misfit and non-uniform weights: (q0, v0, v1 at
    infinity, v1 for p0 = 2 v0, weights)"""
    q0, v0 = vector_grid()
    x, y = v0[..., 0], v0[..., 1]
    bump = 1e-4*np.stack((np.sin(3.*x), np.cos(2.*y), np.sin(x + y)), axis=-1)
    gross = (x > 0.45) & (y > 0.15)
    out = []
    for p0 in (v0, 2.*v0):
        v1 = transformed(ref_api, RT_TRUE if p0 is not v0 else RT_TRUE*(1, 1, 1, 0, 0, 0), p0) + bump
        v1[gross] = transformed(ref_api, np.array((0.2, -0.25, 0.1, 0., 0., 0.)), v1[gross])
        out.append(v1/np.linalg.norm(v1, axis=-1, keepdims=True))
    weights = 0.5 + 1.5*(0.5 + 0.5*np.sin(2.*x)*np.cos(3.*y))
    assert 20 < np.count_nonzero(gross) < 100
    return q0, v0, out[0], out[1], weights


@pytest.mark.gpu
def test_exact_recovery(amd, ref_api):
    """510 points (not a multiple of 64); the device's largest parameter error against the largest of the checker's"""
    q0, v0 = vector_grid()
    assert v0.shape == (17, 30, 3)
    # (a) at infinity
    v1 = transformed(ref_api, RT_TRUE*(1, 1, 1, 0, 0, 0), v0)
    Rt = amd.implied_Rt10__from_unprojections(q0, v0, v1)
    assert np.array_equal(Rt[3], np.zeros(3))
    err = np.abs(rt_of(amd, Rt)[:3] - RT_TRUE[:3]).max()
    cut = flatten_inputs(q0, v0, v1, None)
    errc = max(np.abs(checker_fit(ref_api, *cut, True, s)[:3] - RT_TRUE[:3]).max() for s in SEEDS)
    print(f"exact recovery at infinity: device {err:.3g}, checker's worst {errc:.3g}")
    assert err <= errc
    # (b) two distances: the points that camera 1 sees at distances 1 and 5 along its grid of unit vectors
    p0, v1 = exact_two_distances(ref_api, v0)
    Rt = amd.implied_Rt10__from_unprojections(q0, p0, v1, atinfinity=False)
    err = np.abs(rt_of(amd, Rt) - RT_TRUE).max()
    cut = flatten_inputs(q0, p0, v1, None)
    errc = max(np.abs(checker_fit(ref_api, *cut, False, s) - RT_TRUE).max() for s in SEEDS)
    print(f"exact recovery at distances 1 and 5: device {err:.3g}, checker's worst {errc:.3g}")
    assert err <= errc


@pytest.mark.gpu
@pytest.mark.parametrize("atinfinity", (True, False))
def test_same_cost_as_the_reference_solver(amd, ref_api, misfit_case, atinfinity):
    q0, v0, v1_inf, v1_fin, weights = misfit_case
    p0, v1 = (v0, v1_inf) if atinfinity else (2.*v0, v1_fin)
    Rt = amd.implied_Rt10__from_unprojections(q0, p0, v1, weights=weights, atinfinity=atinfinity)
    cut = flatten_inputs(q0, p0, v1, weights)
    # (the gross region is in the linear part of the Huber loss, the rest in the quadratic part)
    x = residual_of_Rt(Rt[:3], Rt[3], *cut, atinfinity)
    assert np.count_nonzero(np.abs(x) > C_HUBER) > 20 and np.count_nonzero(np.abs(x) < C_HUBER) > 250
    assert_cost_no_worse(ref_api, Rt, *cut, atinfinity, label=f"misfit atinfinity={atinfinity}")


@pytest.mark.gpu
def test_sizes_and_sanitising(amd, ref_api):
    import mrcal_amd.model_analysis as ma
    # 5 points, fewer than a wavefront: a grid point and its four neighbours
    q0, v0 = vector_grid()
    v1 = transformed(ref_api, RT_TRUE*(1, 1, 1, 0, 0, 0), v0)
    fc, fr = q0[8, 14], 110.
    assert np.count_nonzero(np.sum((q0 - fc)**2, axis=-1) < fr*fr) == 5
    rt, report = ma._implied_rt10(q0, v0, v1, None, True, fc, fr)
    assert report["Nused"] == 5 and report["status"] in (0, 1, 3) and 1 <= report["Nevaluations"] <= 400
    Rt = amd.implied_Rt10__from_unprojections(q0, v0, v1, focus_center=fc, focus_radius=fr)
    assert np.array_equal(Rt[:3], amd.R_from_r(rt[:3]))
    assert_cost_no_worse(ref_api, Rt, *flatten_inputs(q0, v0, v1, None, fc, fr), True, seeds=(0,), label="5 points")
    # 2 points
    fc2 = (q0[8, 14] + q0[8, 15])/2.
    assert np.count_nonzero(np.sum((q0 - fc2)**2, axis=-1) < 60.*60.) == 2
    with pytest.raises(Exception, match="Focus region contained too few points"):
        amd.implied_Rt10__from_unprojections(q0, v0, v1, focus_center=fc2, focus_radius=60.)

    # 50 x 28 x 2 distances = 2800 points: more than one pass of the workgroup
    q0, v0 = vector_grid(50, 28)
    p0, v1 = exact_two_distances(ref_api, v0)
    x, y = v0[..., 0], v0[..., 1]
    weights = np.stack((1. + 0.5*np.sin(3.*x), 1. + 0.5*np.cos(2.*y)))
    Rt = amd.implied_Rt10__from_unprojections(q0, p0, v1, weights=weights, atinfinity=False)
    assert np.abs(rt_of(amd, Rt) - RT_TRUE).max() < 1e-6
    assert_cost_no_worse(ref_api, Rt, *flatten_inputs(q0, p0, v1, weights), False, seeds=(0,), label="2800 points")
    # the same bits on a second call
    assert np.array_equal(Rt, amd.implied_Rt10__from_unprojections(q0, p0, v1, weights=weights, atinfinity=False))
    # NaN and inf sprinkled in: the fit on the cleaned arrays, to the bit
    rng = np.random.RandomState(5)
    p0d, v1d, wd = p0.copy(), v1.copy(), weights.copy()
    for a, bad in ((p0d, np.nan), (p0d, np.inf), (v1d, np.nan), (v1d, -np.inf), (wd, np.nan), (wd, np.inf)):
        a.reshape(-1)[rng.choice(a.size, 9, replace=False)] = bad
    p0c, v1c, wc = p0d.copy(), v1d.copy(), wd.copy()
    wc[~np.isfinite(wc)] = 0.
    wc[~np.isfinite(p0c).all(axis=-1)] = 0.
    wc[:, ~np.isfinite(v1c).all(axis=-1)] = 0.
    p0c[~np.isfinite(p0c)] = 0.
    v1c[~np.isfinite(v1c)] = 0.
    assert np.count_nonzero(wc == 0.) >= 40
    Rtd = amd.implied_Rt10__from_unprojections(q0, p0d, v1d, weights=wd, atinfinity=False)
    Rtc = amd.implied_Rt10__from_unprojections(q0, p0c, v1c, weights=wc, atinfinity=False)
    assert np.isfinite(Rtd).all() and np.array_equal(Rtd, Rtc)
    assert np.abs(rt_of(amd, Rtd) - RT_TRUE).max() < 1e-6


def exact_two_distances(ref, v1, distances=(1., 5.)):
    """p0 (M,Nh,Nw,3) and the unit vectors v1 with v1 = normalize(R p0 + t) for every distance: the points camera 1 sees
    at the distances along v1, in camera 0's frame"""
    R = ref_R_from_r(ref, RT_TRUE[:3])[0]
    p0 = np.stack([np.einsum("ji,...j->...i", R, d*v1 - RT_TRUE[3:]) for d in distances])
    return p0, v1


# ---- the reference's own test (test/test-projection-diff.py), its fixtures and thresholds
@pytest.fixture(scope="module")
def cam0(amd):
    return (amd.cameramodel(os.path.join(GOLDEN_DIR, "cam0.opencv8.cameramodel")),
            amd.cameramodel(os.path.join(GOLDEN_DIR, "cam0.splined.cameramodel")))


def rotation_deg(Rt):
    return np.arccos(np.clip((np.trace(Rt[:3]) - 1.)/2., -1., 1.))*180./np.pi


@pytest.mark.gpu
@pytest.mark.parametrize("distance", (None, 3.))
def test_reference_test_model_against_itself(amd, cam0, distance):
    splined = cam0[1]
    difflen, diff, q0, Rt10 = amd.projection_diff((splined, splined), gridn_width=50, distance=distance, use_uncertainties=False)
    W, H = splined.imagersize()
    assert difflen.shape == (int(round(H/W*50)), 50) and diff.shape == difflen.shape + (2,) and q0.shape == diff.shape
    worst = np.nanmax(difflen)
    print(f"model against itself, distance {distance}: worst difflen {worst:.3g} px, rotation {rotation_deg(Rt10):.3g} deg, "
          f"|t| {np.linalg.norm(Rt10[3]):.3g}")
    assert np.count_nonzero(np.isfinite(difflen)) > 0.9*difflen.size
    # the reference's thresholds
    assert worst < 0.08 and rotation_deg(Rt10) < 0.01 and np.linalg.norm(Rt10[3]) < 0.01
    # ... and ours: the start is exact
    assert np.array_equal(Rt10, amd.identity_Rt())
    assert worst < 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("focus_radius", (800, 366))
def test_reference_test_opencv8_against_splined(amd, cam0, focus_radius):
    difflen, diff, q0, Rt10 = amd.projection_diff(cam0, gridn_width=50, distance=5, use_uncertainties=False, focus_radius=focus_radius)
    ic = np.array(difflen.shape)//2
    print(f"OPENCV8 against splined, focus_radius {focus_radius}: centre difflen {difflen[ic[0], ic[1]]:.3g} px")
    assert difflen[ic[0], ic[1]] < 0.1


@pytest.mark.gpu
def test_reference_test_shifted_focal_length(amd, cam0):
    shifted = amd.cameramodel(cam0[0])
    lensmodel, intrinsics = shifted.intrinsics()
    intrinsics = np.array(intrinsics)
    intrinsics[0] *= 1.0001
    intrinsics[1] *= 1.0002
    shifted.intrinsics(intrinsics=(lensmodel, intrinsics))
    difflen, diff, q0, Rt10 = amd.projection_diff((cam0[0], shifted), gridn_width=50, distance=50000, use_uncertainties=False,
                                                  focus_radius=1500)
    ic = np.array(difflen.shape)//2
    print(f"shifted focal length at 50 km: centre {difflen[ic[0], ic[1]]:.3g} px, mean {np.mean(difflen):.3g} px, "
          f"|t| {np.linalg.norm(Rt10[3]):.4g} m")
    assert difflen[ic[0], ic[1]] < 2e-2 and np.mean(difflen) < 0.2
    # (the fit moved the origin: the rehearsal and the reference's solver both had 5.8 m)
    assert 3. < np.linalg.norm(Rt10[3]) < 9.


# ---- the diff without the fit
RT_GIVEN = np.array((0.01, -0.02, 0.015, 0.03, -0.01, 0.02))


def _diff_models(amd, cam0):
    W, H = (int(x) for x in cam0[0].imagersize())
    c = ((W - 1)/2., (H - 1)/2.)
    cahvore = amd.cameramodel(intrinsics=("LENSMODEL_CAHVORE_linearity=0.37",
                                          np.array((1700., 1705., c[0] + 3., c[1] - 2., 0.01, -0.02, 0.03, 0.001, -0.002, 0.01, 0.02, 0.03))),
                              imagersize=(W, H))
    stereographic = amd.cameramodel(intrinsics=("LENSMODEL_STEREOGRAPHIC", np.array((1750., 1755., c[0] - 5., c[1] + 4.))),
                                    imagersize=(W, H))
    return dict(opencv8=cam0[0], splined=cam0[1], cahvore=cahvore, stereographic=stereographic)


@pytest.mark.gpu
@pytest.mark.parametrize("pair,distance", ((("opencv8", "splined"), 5.), (("splined", "opencv8"), (1., 5., 40.)),
                                           (("opencv8", "cahvore"), None), (("cahvore", "stereographic"), None),
                                           (("stereographic", "opencv8"), (3.,)), (("opencv8", "stereographic"), None)))
def test_diff_with_a_given_transformation(amd, ref_api, cam0, pair, distance):
    models = [_diff_models(amd, cam0)[name] for name in pair]
    Rt = amd.Rt_from_rt(RT_GIVEN)
    difflen, diff, q0, Rt10 = amd.projection_diff(models, implied_Rt10=Rt, gridn_width=24, distance=distance, use_uncertainties=False)
    assert np.array_equal(Rt10, Rt)
    W, H = models[0].imagersize()
    assert np.array_equal(q0, amd.sample_imager(24, None, W, H)) and q0.shape == (13, 24, 2)
    intr = []
    for m in models:
        lensmodel, i = m.intrinsics()
        i = np.array(i)
        if lensmodel.startswith("LENSMODEL_CAHVORE"): i[-3:] = 0.
        intr.append((lensmodel, i))
    v0 = ref_api.unproject(q0, *intr[0], normalize=True)
    d = np.ones(1) if distance is None else np.atleast_1d(np.array(distance, dtype=float))
    p = v0*d[:, None, None, None]
    want = ref_api.project(np.einsum("ij,...j->...i", Rt[:3], p) + Rt[3], *intr[1]) - q0
    iterable = distance is not None and np.ndim(distance) > 0
    if not iterable: want = want[0]
    assert diff.shape == want.shape and difflen.shape == want.shape[:-1]
    ok = np.isfinite(want).all(axis=-1) & np.isfinite(diff).all(axis=-1)
    assert np.count_nonzero(ok) > 0.85*ok.size
    # (q1 = q0 + diff is what was projected: the bar of the projection tests is on the pixels)
    e = relative_error((diff + q0)[ok], (want + q0)[ok]).max()
    print(f"{pair} distance {distance}: q1 relative error {e:.3g}")
    assert e < 1e-6
    assert np.allclose(difflen[ok], np.linalg.norm(diff[ok], axis=-1), rtol=1e-14, atol=0)


# ---- with uncertainties
@pytest.fixture(scope="module")
def real_models(amd):
    return [amd.cameramodel(os.path.join(GOLDEN_DIR, name + ".cameramodel")) for name in ("real_opencv8-0", "real_splined-0")]


@pytest.mark.gpu
def test_with_uncertainties_against_the_public_primitives(amd, ref_api, real_models):
    distance = (1., 5.)
    report = {}
    import mrcal_amd.model_analysis as ma
    difflen, diff, q0, Rt10 = ma._projection_diff(real_models, None, report, gridn_width=12, distance=distance)
    for a, b in zip((difflen, diff, q0, Rt10), amd.projection_diff(real_models, gridn_width=12, distance=distance)):
        assert np.array_equal(a, b, equal_nan=True)
    assert q0.shape == (8, 12, 2) and diff.shape == (2, 8, 12, 2) and difflen.shape == (2, 8, 12) and Rt10.shape == (4, 3)
    W, H = (int(x) for x in real_models[0].imagersize())
    v, q = amd.sample_imager_unproject(12, None, W, H, [m.intrinsics()[0] for m in real_models],
                                       [m.intrinsics()[1] for m in real_models], normalize=True)
    assert np.array_equal(q, q0) and v.shape == (2, 8, 12, 3)
    d = np.array(distance)[:, None, None, None]
    u = []
    for i, m in enumerate(real_models):
        with amd.ProjectionUncertainty(m) as pu:
            u.append(pu.evaluate(v[i]*d, what="worstdirection-stdev"))
    weights = 1./(u[0]*u[1])
    weights *= weights
    fc, fr = ((W - 1.)/2., (H - 1.)/2.), float(max(W, H)*100.)
    Rt = amd.implied_Rt10__from_unprojections(q0, v[0]*d, v[1], weights=weights, atinfinity=False, focus_center=fc, focus_radius=fr)
    assert np.array_equal(Rt10, Rt)
    want = amd.project(amd.transform_point_Rt(Rt, v[0]*d), *real_models[1].intrinsics()) - q0
    ok = np.isfinite(want).all(axis=-1)
    assert np.count_nonzero(ok) > 0.9*ok.size and not np.isfinite(diff[~ok]).any()
    print(f"with uncertainties: diff against the composition {np.abs(diff[ok] - want[ok]).max():.3g} px, "
          f"evaluations {report['Nevaluations']}, status {report['status']}")
    assert np.abs(diff[ok] - want[ok]).max() < 1e-9
    assert_cost_no_worse(ref_api, Rt10, *flatten_inputs(q0, v[0]*d, v[1], weights, fc, fr), False, label="real models, weighted")


@pytest.mark.gpu
def test_uncertainties_unavailable_warns_and_goes_on(amd, cam0, capsys):
    want = amd.projection_diff(cam0, gridn_width=12, distance=5., use_uncertainties=False, focus_radius=800.)
    capsys.readouterr()
    got = amd.projection_diff(cam0, gridn_width=12, distance=5., use_uncertainties=True, focus_radius=800.)
    err = capsys.readouterr().err
    assert "WARNING: projection_diff() was asked to use uncertainties, but they aren't available/couldn't be computed. " \
           "Falling back on the region-based-only logic. Caught exception: optimization_inputs are unavailable" in err
    for a, b in zip(got, want):
        assert np.array_equal(a, b, equal_nan=True)


# ---- three models
@pytest.mark.gpu
def test_three_models(amd, cam0):
    shifted = amd.cameramodel(cam0[0])
    lensmodel, intrinsics = shifted.intrinsics()
    intrinsics = np.array(intrinsics)
    intrinsics[:2] *= (1.0003, 1.0001)
    intrinsics[2:4] += (0.7, -0.4)
    shifted.intrinsics(intrinsics=(lensmodel, intrinsics))
    kw = dict(gridn_width=20, distance=(2., 10.), use_uncertainties=False, focus_radius=700)
    difflen, diff, q0, Rt10 = amd.projection_diff((cam0[0], cam0[1], shifted), **kw)
    assert diff is None and Rt10.shape == (2, 4, 3) and difflen.shape == (2, 11, 20)
    two = [amd.projection_diff((cam0[0], m), **kw) for m in (cam0[1], shifted)]
    for i in range(2):
        assert np.array_equal(Rt10[i], two[i][3])
        assert np.array_equal(q0, two[i][2])
    want = np.sqrt((two[0][0]**2 + two[1][0]**2)/2.)
    ok = np.isfinite(want)
    assert np.count_nonzero(ok) > 0.9*ok.size
    assert np.allclose(difflen[ok], want[ok], rtol=1e-12, atol=1e-12)
    assert not np.array_equal(Rt10[0], Rt10[1])
