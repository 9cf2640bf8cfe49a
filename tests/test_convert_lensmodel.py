"""fit_lensmodel() and convert_lensmodel(): the reference's mrcal-convert-lensmodel, the sampled fit on the device
(csrc/lensfit.hip; include/mrcal_amd.h, "lens-model fit").

The checker (tests/convert_lensmodel_checker.py) is the reference's own sampled problem handed to the reference's compiled
library through the ref_api fixture: x and J anywhere from its optimizer_callback(), solves from its optimize().
Without a GPU: the grid and radius selection, the starts, hypothesis_board_corner_positions(), the tool's refusals.
On the GPU: the cost at a start for every lens model, zero-residual recovery, stationarity and parity with the
reference's solver, the batch, convert_lensmodel() end to end in both modes, and the buffers given back."""
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR, relative_error
from mrcal_amd.synthetic import make_calibration_problem, copy_inputs, intrinsics_for, IMAGERSIZE, CAM_OPENCV8
from mrcal_amd.poseutils import (transform_point_rt, Rt_from_rt, rt_from_Rt, compose_Rt, identity_Rt, compose_rt)
import convert_lensmodel_checker as chk

W, H = IMAGERSIZE
SPLINED_SMALL = "LENSMODEL_SPLINED_STEREOGRAPHIC_order=3_Nx=8_Ny=6_fov_x_deg=80"
# every row of the lens table (csrc/lens_dispatch.hpp); CAHVORE at linearity 0 and 0.3
LENS_TABLE = ("LENSMODEL_PINHOLE", "LENSMODEL_STEREOGRAPHIC", "LENSMODEL_LONLAT", "LENSMODEL_LATLON", "LENSMODEL_OPENCV4",
              "LENSMODEL_OPENCV5", "LENSMODEL_OPENCV8", "LENSMODEL_OPENCV12", "LENSMODEL_CAHVOR",
              "LENSMODEL_CAHVORE_linearity=0.00", "LENSMODEL_CAHVORE_linearity=0.30")
# a stereographic camera that sees +-35 degrees across the imager's width: 2 tan(35 deg/2) f = W/2
STEREOGRAPHIC_35 = np.array((3170., 3170., (W - 1)/2., (H - 1)/2.))


def wide_points(N, seed):
    """N points over +-45 x +-31 degrees, alternately 2 m and 20 m away"""
    rng = np.random.default_rng(seed)
    v = np.column_stack((rng.uniform(-1., 1., N), rng.uniform(-.6, .6, N), np.ones(N)))
    return v*np.where(np.arange(N) % 2, 2., 20.)[:, None]


def shapes(plan):
    """N with 2N in {NP, C-2, C, C+2, 3C+2} (NP odd: the next even number), and one N below 32"""
    NP, C = max(plan["NP1"], plan["NP2"]), plan["chunk_rows"]
    return sorted({(NP + 1)//2, (C - 2)//2, C//2, (C + 2)//2, (3*C + 2)//2, 17})


# ------------------------------------------------------------------------------------------------ without a GPU ---
@pytest.mark.parametrize("radius", (700., -300., 0, None))
@pytest.mark.parametrize("where", (None, (2100., 1000.)))
def test_grid_and_radius_selection(radius, where):
    """mrcal-convert-lensmodel:636-681 against its numpy restatement in the checker"""
    from mrcal_amd.lensmodel_conversion import _sample_grid
    dims = np.array((W, H), dtype=np.int32)
    off_centre = where is not None and (radius is None or radius < 0)
    if off_centre:
        with pytest.raises(Exception, match="A radius <0 is only implemented if we're focusing on the imager center"):
            _sample_grid(dims, (30, 20), np.array(where), radius)
        return
    got = _sample_grid(dims, (30, 20), None if where is None else np.array(where), radius)
    want = chk.sample_grid(dims, (30, 20), where, radius)
    assert got.shape == want.shape and got.shape[1] == 2 and np.array_equal(got, want)
    if radius == 0:
        assert len(got) == 600
    else:
        assert 0 < len(got) < 600
    if radius is None:
        # a quarter of the smaller dimension off each corner: the half diagonal less 550
        assert np.array_equal(got, chk.sample_grid(dims, (30, 20), None, -550))
    # x fastest, then y: the reference's meshgrid order
    full = _sample_grid(dims, (4, 3), None, 0)
    assert np.array_equal(full[:5], ((0., 0.), ((W - 1)/3., 0.), (2*(W - 1)/3., 0.), (W - 1., 0.), (0., (H - 1)/2.)))
    # where at the centre is where not given
    assert np.array_equal(_sample_grid(dims, (30, 20), np.array(((W - 1)/2., (H - 1)/2.)), -300.), _sample_grid(dims, (30, 20), None, -300.))


@pytest.mark.parametrize("lensmodel,Nd", (("LENSMODEL_OPENCV4", 4), ("LENSMODEL_OPENCV8", 8), ("LENSMODEL_OPENCV12", 12), ("LENSMODEL_CAHVOR", 5)))
def test_starts(lensmodel, Nd):
    """mrcal-convert-lensmodel:727-731, 786: shape, amplitudes, the rational terms' extra 1e-3, one generator a seed"""
    from mrcal_amd.lensmodel_conversion import _starts
    core = np.array((1700., 1710., 1999., 1100.))
    Nt = 64
    intr, rt = _starts(lensmodel, core, Nd, Nt, 3, None, True)
    assert intr.shape == (Nt, 4 + Nd) and rt.shape == (Nt, 6)
    assert np.array_equal(intr[:, :4], np.tile(core, (Nt, 1)))
    rational = np.zeros(Nd, dtype=bool)
    if lensmodel in ("LENSMODEL_OPENCV8", "LENSMODEL_OPENCV12"): rational[5:8] = True
    plain = intr[:, 4:][:, ~rational]
    assert np.all(np.abs(plain) <= 0.5e-3) and np.abs(plain).max() > 0.4e-3 and plain.min() < 0 < plain.max()
    if rational.any():
        r = intr[:, 4:][:, rational]
        assert np.all(np.abs(r) <= 0.5e-6) and np.abs(r).max() > 0.4e-6
    assert np.all(np.abs(rt) <= 0.5e-6) and np.abs(rt).max() > 0.4e-6
    # the draws, in the tool's order: a trial's distortions, then its pose
    rng = np.random.default_rng(3)
    for i in range(2):
        d = (rng.random(Nd) - 0.5)*1e-3
        d[rational] *= 1e-3
        assert np.array_equal(intr[i, 4:], d)
        assert np.array_equal(rt[i], (rng.random(6) - 0.5)*1e-6)
    # the same seed: the same starts; another: others; without the pose: none is drawn
    again, rt_again = _starts(lensmodel, core, Nd, Nt, 3, None, True)
    assert np.array_equal(intr, again) and np.array_equal(rt, rt_again)
    other, _ = _starts(lensmodel, core, Nd, Nt, 4, None, True)
    assert not np.array_equal(intr, other)
    nopose, none = _starts(lensmodel, core, Nd, 2, 3, None, False)
    assert none is None and np.array_equal(nopose[0], intr[0]) and not np.array_equal(nopose[1], intr[1])
    # distortion_seeds are taken as they are: no scaling of the rational terms
    given = np.arange(3*Nd, dtype=float).reshape(3, Nd)*1e-2
    intr, rt = _starts(lensmodel, core, Nd, 3, 3, given, True)
    assert np.array_equal(intr[:, 4:], given) and np.array_equal(intr[:, :4], np.tile(core, (3, 1)))
    assert np.array_equal(rt[0], (np.random.default_rng(3).random(6) - 0.5)*1e-6)
    with pytest.raises(Exception, match="distortion_seeds must have shape"):
        _starts(lensmodel, core, Nd, 3, 3, given[:2], True)


def test_hypothesis_board_corner_positions(amd, ref_api):
    """The corners projected through the reference are where its callback says the hypothesis is: observation +
    residual/weight. Rounding only: 1e-9 px"""
    oi, _ = make_calibration_problem(ref_api, Ncameras=2, Nframes=4, lensmodel="LENSMODEL_OPENCV4", object_width_n=5,
                                     object_height_n=4, seed=2)
    obs = oi["observations_board"]
    obs[1, 2, 1:3, 2] = -1.
    obs[5, 0, 4, 2] = -1.
    _, x, _, _ = ref_api.optimizer_callback(no_jacobian=True, no_factorization=True, **oi)
    Nb = ref_api.num_measurements_boards(**oi)
    xb = x[ref_api.measurement_index_boards(0, **oi):][:Nb].reshape(obs.shape[:-1] + (2,))
    inl = obs[..., 2] > 0
    assert np.count_nonzero(~inl) > 0
    pall, pcam, pin, pout = amd.hypothesis_board_corner_positions(**oi)
    assert pall.shape == obs.shape[:-1] + (3,) and pcam is pall
    assert np.array_equal(pin, pall[inl]) and np.array_equal(pout, pall[~inl])
    icam = oi["indices_frame_camintrinsics_camextrinsics"][:, 1]
    q = np.stack([ref_api.project(pall[i], oi["lensmodel"], oi["intrinsics"][icam[i]]) for i in range(len(pall))])
    want = obs[..., :2] + xb/obs[..., 2:3]
    err = np.abs(q - want)[inl].max()
    print("hypothesis_board_corner_positions(): projected corners differ from the reference's hypothesis by", err, "px")
    assert err < 1e-9
    # one camera, and inliers picked by the caller
    for ic in (0, 1):
        mine = icam == ic
        _, pcam, pin, pout = amd.hypothesis_board_corner_positions(ic, **oi)
        assert np.array_equal(pcam, pall[mine])
        assert np.array_equal(pin, pall[inl & mine[:, None, None]]) and np.array_equal(pout, pall[~inl & mine[:, None, None]])
    pick = np.zeros(inl.shape, dtype=bool); pick[1, 2, 3] = pick[0, 0, 0] = True
    keep = pick.copy()
    _, _, pin, _ = amd.hypothesis_board_corner_positions(int(icam[1]), idx_inliers=pick, **oi)
    assert np.array_equal(pin, pall[keep & (icam == icam[1])[:, None, None]])
    with pytest.raises(Exception, match="No board observations available"):
        amd.hypothesis_board_corner_positions(**{**oi, "observations_board": None})


def test_refusals_before_any_device_work(amd, monkeypatch):
    """the tool's failure modes, with its messages, raised before anything is made on the device"""
    import mrcal_amd.lensmodel_conversion as lc
    def no_device(*a, **k): raise AssertionError("device work before the refusal")
    monkeypatch.setattr(lc.LensFitter, "__init__", no_device)
    monkeypatch.setattr(amd._api, "optimize", no_device)
    monkeypatch.setattr(amd._api, "unproject", no_device)
    m = amd.cameramodel(os.path.join(GOLDEN_DIR, "real_opencv8-0.cameramodel"))
    assert m.optimization_inputs() is not None
    with pytest.raises(Exception, match="--sampled without --intrinsics-only REQUIRES --distance"):
        amd.convert_lensmodel(m, "LENSMODEL_OPENCV4", sampled=True)
    with pytest.raises(Exception, match="--intrinsics-only requires --sampled"):
        amd.convert_lensmodel(m, "LENSMODEL_OPENCV4", sampled=False, intrinsics_only=True)
    m0 = amd.cameramodel(m); m0.optimization_inputs_reset()
    with pytest.raises(Exception, match="optimization_inputs not available in this model, so only sampled fits are possible. Pass --sampled"):
        amd.convert_lensmodel(m0, "LENSMODEL_OPENCV4", sampled=False)
    # (without optimization_inputs the default is the sampled fit)
    with pytest.raises(Exception, match="--sampled without --intrinsics-only REQUIRES --distance"):
        amd.convert_lensmodel(m0, "LENSMODEL_OPENCV4")
    with pytest.raises(Exception, match="Unknown lens model: 'LENSMODEL_BOGUS'"):
        amd.convert_lensmodel(m, "LENSMODEL_BOGUS", sampled=True, intrinsics_only=True)
    with pytest.raises(Exception, match="All values in --distances must be finite and > 0"):
        amd.convert_lensmodel(m, "LENSMODEL_OPENCV4", sampled=True, distance=(1., -2.))
    with pytest.raises(Exception, match="A radius <0 is only implemented if we're focusing on the imager center"):
        amd.convert_lensmodel(m, "LENSMODEL_OPENCV4", sampled=True, intrinsics_only=True, where=(100., 100.), radius=-100)
    # the same model: nothing to do, as the tool has it
    same, info = amd.convert_lensmodel(m, m.intrinsics()[0], sampled=True, intrinsics_only=True)
    assert np.array_equal(same.intrinsics()[1], m.intrinsics()[1]) and info["rms_reproj_error__pixels"][0] == 0
    # (what is in order goes on to the device)
    with pytest.raises(AssertionError, match="device work"):
        amd.convert_lensmodel(m, "LENSMODEL_OPENCV4", sampled=True, intrinsics_only=True)


def test_moved_camera_warning_texts():
    """mrcal-convert-lensmodel:819-831: more than 1 cm, and the hint only for a sampled fit with distances given"""
    from mrcal_amd.lensmodel_conversion import _moved_warning
    near = Rt_from_rt(np.array((0.3, -0.2, 0.1, 0.006, -0.006, 0.005)))      # 9.8 mm
    far  = Rt_from_rt(np.array((0.001, 0.002, 0., 0.03, -0.04, 0.12)))       # 130 mm
    assert _moved_warning(identity_Rt(), True) is None and _moved_warning(near, True) is None and _moved_warning(near, False) is None
    text = "## WARNING: fitted camera moved by 0.130m. This is probably aphysically high, and something is wrong."
    assert _moved_warning(far, False) == text
    assert _moved_warning(far, True) == text + " Pass both a high and a low --distance?"


def test_a_best_trial_that_did_not_converge_is_reported(amd, monkeypatch):
    """info['warning_status']: None for a converged best trial, a text naming the status otherwise"""
    import mrcal_amd.lensmodel_conversion as lc
    m = amd.cameramodel(os.path.join(GOLDEN_DIR, "real_opencv8-0.cameramodel"))
    def fake_unproject(q, lensmodel, intrinsics, normalize=False):
        v = np.column_stack(((q - 3000.)/5000., np.ones(len(q))))
        return v/np.linalg.norm(v, axis=-1, keepdims=True)
    monkeypatch.setattr(amd._api, "unproject", fake_unproject)
    for status, text in ((0, None), (1, "bound on evaluations reached"), (3, "stalled")):
        def fake_fit(p, q, lensmodel, seeds, **kw):
            Nt = len(seeds)
            return dict(intrinsics=seeds.copy(), rt_cam_ref=np.zeros((Nt, 6)), cost=np.full(Nt, 8.), rms_reproj_error__pixels=np.array((2., 1.5))[:Nt],
                        Nevaluations=np.full(Nt, 7, dtype=np.int32), status=np.array((0, status), dtype=np.int32)[:Nt], ibest=1)
        monkeypatch.setattr(lc, "fit_lensmodel", fake_fit)
        _, info = amd.convert_lensmodel(m, "LENSMODEL_OPENCV4", sampled=True, intrinsics_only=True, num_trials=2)
        if text is None:
            assert info["warning_status"] is None
        else:
            assert info["warning_status"].startswith(f"## WARNING: the best trial did not converge (status {status}: {text}) and ended at rms 1.500 pixels.")


# --------------------------------------------------------------------------------------------------- on the GPU ---
@pytest.fixture(scope="module")
def fitter(amd):
    f = amd.LensFitter()
    yield f
    f.close()


@pytest.mark.gpu
@pytest.mark.parametrize("lensmodel", LENS_TABLE)
def test_cost_is_the_references(amd, ref_api, fitter, lensmodel):
    """One evaluation at the start: the cost is the reference's x.x there, and the rms its definition. A difference of
    summation order only: relative 1e-10, what tests/test_solver_parity.py holds norm2_x to. Regularization on and
    off, with and without weights, with a w <= 0 point, a w = 0 point and NaN points present, with and without the
    pose and the core, at every N the chunking takes another path at"""
    truth = intrinsics_for(lensmodel, 1)[0]
    rng = np.random.default_rng(11)
    start = truth.copy()
    start[:4] += rng.uniform(-5, 5, 4)
    start[4:] += rng.uniform(-2e-3, 2e-3, len(truth) - 4)
    rt_start = np.array((0.01, -0.02, 0.015, 0.03, -0.01, 0.02))
    worst = 0.0
    for core, pose in ((True, False), (True, True), (False, True), (False, False)):
        if not core and not pose and len(truth) == 4: continue       # nothing to fit: refused (tests/test_lensfit_plan.py)
        plan = amd.fit_lensmodel_plan(lensmodel, 1000, optimize_core=core, optimize_extrinsics=pose)
        for N in shapes(plan):
            p = wide_points(N, N)
            q = ref_api.project(p, lensmodel, truth) + rng.uniform(-3, 3, (N, 2))
            for bad in (False, True):
                if bad and N < 17: continue
                w = None
                pp, qq = p.copy(), q.copy()
                if bad:
                    w = rng.uniform(0.5, 2., N)
                    w[3], w[4] = -1., 0.
                    pp[5, 1] = np.nan
                    qq[7, 0] = np.nan
                    w[9] = np.nan
                for reg in (True, False):
                    r = fitter.fit(pp, qq, lensmodel, start, imagersize=(W, H), weights=w, rt_seed=rt_start if pose else None,
                                   optimize_core=core, optimize_extrinsics=pose, do_apply_regularization=reg, max_evaluations=1)
                    C = chk.CheckerInputs(ref_api, pp, qq, w, lensmodel, start, rt_start if pose else None, imagersize=(W, H),
                                          optimize_core=core, apply_regularization=reg)
                    cost, rms = C.cost()
                    assert r["status"][0] == 1 and r["ibest"] == 0
                    assert r["Nevaluations"][0] == ((2 if pose and plan["NP1"] > 0 else 1))
                    assert np.array_equal(r["intrinsics"][0], start)
                    if pose: assert np.array_equal(r["rt_cam_ref"][0], rt_start)
                    e = max(abs(r["cost"][0] - cost)/cost, abs(r["rms_reproj_error__pixels"][0] - rms)/rms)
                    worst = max(worst, e)
                    assert e < 1e-10, (core, pose, N, bad, reg, r["cost"][0], cost)
    print(f"{lensmodel}: cost and rms at a start differ from the reference's by at most {worst:.3g} (relative)")


@pytest.mark.gpu
@pytest.mark.parametrize("lensmodel,pose", (("LENSMODEL_OPENCV4", True), ("LENSMODEL_OPENCV8", True), ("LENSMODEL_STEREOGRAPHIC", True),
                                            ("LENSMODEL_OPENCV4", False), ("LENSMODEL_OPENCV8", False), ("LENSMODEL_CAHVOR", False)))
def test_zero_residual_recovery(amd, ref_api, fitter, lensmodel, pose):
    """q = project(T p) of a known intrinsics vector, fitted with the same model type from the core plus seeds of 1e-3,
    no regularization: the minimum is exactly 0. Converged, rms < 1e-6 px, and the known T (2 degrees, 3 cm; points at
    two distances) comes back to 1e-6. Projections round at about 1e-12 px and Gauss-Newton converges quadratically on
    a zero-residual problem: a termination above 1e-6 px is a defect.
    OPENCV4, OPENCV8 and STEREOGRAPHIC with the pose; these and CAHVOR also with T the identity and the intrinsics
    alone. CAHVOR WITH the pose is not asserted: after stage 1 has fitted the rotation away with the distortion terms,
    the reference's own two solves from these starts end at 3 to 11 px, and this iteration at 6e-13 to 7 px depending
    on N: the trial is one of several for such a target, which is what num_trials is for"""
    truth = intrinsics_for(lensmodel, 1)[0]
    T = np.array((0.02, -0.025, 0.01, 0.02, -0.02, 0.01)) if pose else None
    assert not pose or (abs(np.linalg.norm(T[:3])*180/np.pi - 2.) < 0.1 and abs(np.linalg.norm(T[3:]) - 0.03) < 1e-12)
    plan = amd.fit_lensmodel_plan(lensmodel, 1000, optimize_extrinsics=pose)
    for N in (17, (plan["chunk_rows"] + 2)//2, (3*plan["chunk_rows"] + 2)//2):
        p = wide_points(N, 2)
        q = ref_api.project(transform_point_rt(T, p) if pose else p, lensmodel, truth)
        seed = truth.copy(); seed[4:] = 1e-3
        r = fitter.fit(p, q, lensmodel, seed, imagersize=(W, H), rt_seed=np.full(6, 1e-7) if pose else None,
                       optimize_extrinsics=pose, do_apply_regularization=False)
        rms = r["rms_reproj_error__pixels"][0]
        print(f"{lensmodel} N={N} pose={pose}: status {r['status'][0]}, rms {rms:.3g} px after {r['Nevaluations'][0]} evaluations" +
              (f", T off by {np.abs(r['rt_cam_ref'][0] - T).max():.3g}" if pose else ""))
        assert r["status"][0] == 0
        assert rms < 1e-6
        assert relative_error(r["cost"][0], rms*rms*2*N) < 1e-12
        if pose:
            assert np.abs(r["rt_cam_ref"][0] - T).max() < 1e-6
        else:
            assert np.array_equal(r["rt_cam_ref"][0], np.zeros(6))


def parity_case(ref_api, lens_from, intrinsics_from, distances):
    """the (9,7) grid of the tool's default radius, unprojected by the reference through the from-model"""
    from mrcal_amd.lensmodel_conversion import _sample_grid
    q = _sample_grid(np.array((W, H)), (9, 7), None, None)
    v = ref_api.unproject(q, lens_from, intrinsics_from, normalize=True)
    d = np.array(distances, dtype=float)
    return (v[None]*d[:, None, None]).reshape(-1, 3), np.tile(q, (len(d), 1))


@pytest.mark.gpu
@pytest.mark.parametrize("lens_from,lens_to", (("LENSMODEL_OPENCV8", "LENSMODEL_OPENCV4"), ("LENSMODEL_OPENCV8", "LENSMODEL_OPENCV5"),
                                               ("LENSMODEL_STEREOGRAPHIC", "LENSMODEL_OPENCV4")))
@pytest.mark.parametrize("distances", ((10.,), (1., 1000.)))
def test_stationarity_and_parity_with_the_references_solver(amd, ref_api, fitter, lens_from, lens_to, distances):
    """Non-zero residual, one minimum: a mildly distorted OPENCV8 camera as OPENCV4 and OPENCV5, a stereographic one
    (+-35 degrees) as OPENCV4, from distortions of zero, regularization on. One distance: the intrinsics alone; two: then
    the pose. cost_dev <= cost_ref (1 + 1e-6), cost_ref what ref_api.optimize() reaches from the same starts (it
    converges on all six); and |J^T x|_inf/(|J|_F |x|) from the reference's J and x at the
    device's solution no more than 10 times what it is at the reference's.
    The figures measured on the MI355X are in DESIGN.md section 9, f16"""
    intrinsics_from = CAM_OPENCV8[0] if lens_from == "LENSMODEL_OPENCV8" else STEREOGRAPHIC_35
    p, q = parity_case(ref_api, lens_from, intrinsics_from, distances)
    Nd = amd.lensmodel_num_params(lens_to) - 4
    seed = np.concatenate((intrinsics_from[:4], np.zeros(Nd)))
    pose = len(distances) > 1
    rt0 = np.full(6, 1e-7)
    r = fitter.fit(p, q, lens_to, seed, imagersize=(W, H), rt_seed=rt0 if pose else None, optimize_extrinsics=pose)
    assert r["status"][0] == 0
    # the reference: stage 1, and from ITS result stage 2
    C1 = chk.CheckerInputs(ref_api, p, q, None, lens_to, seed, None, imagersize=(W, H))
    _, i_ref, _ = C1.optimize()
    C, rt_ref = C1, None
    if pose:
        C = chk.CheckerInputs(ref_api, p, q, None, lens_to, i_ref, rt0, imagersize=(W, H))
        _, i_ref, rt_ref = C.optimize()
    cost_ref, _ = C.cost(i_ref, rt_ref)
    rt_dev = r["rt_cam_ref"][0] if pose else None
    cost_dev, rms_dev = C.cost(r["intrinsics"][0], rt_dev)
    s_dev, s_ref = C.stationarity(r["intrinsics"][0], rt_dev), C.stationarity(i_ref, rt_ref)
    print(f"{lens_from} as {lens_to}, distances {distances}: cost dev {cost_dev:.15g} ref {cost_ref:.15g} (dev/ref - 1 = {cost_dev/cost_ref - 1:.3g}), "
          f"stationarity dev {s_dev:.3g} ref {s_ref:.3g}, {r['Nevaluations'][0]} evaluations")
    # what the device reports is the reference's cost at the device's solution
    assert relative_error(r["cost"][0], cost_dev) < 1e-10 and relative_error(r["rms_reproj_error__pixels"][0], rms_dev) < 1e-10
    assert cost_dev <= cost_ref*(1 + 1e-6)
    assert s_dev <= 10*s_ref


@pytest.mark.gpu
def test_batch(amd, ref_api, fitter):
    """Three trials in one launch: each the bits of the same start run alone, the best the lowest rms, a second call the
    same bits, and a trial with a NaN in its start reported and never chosen"""
    p, q = parity_case(ref_api, "LENSMODEL_OPENCV8", CAM_OPENCV8[0], (1., 1000.))
    core = CAM_OPENCV8[0][:4]
    dseeds = np.array(((0., 0., 0., 0., 0., 0., 0., 0.), (1e-4, -2e-4, 3e-5, 1e-5, 2e-4, 1e-7, -2e-7, 1e-7), (-3e-4, 1e-4, -2e-5, 4e-5, -1e-4, 2e-7, 1e-7, -3e-7)))
    seeds = np.column_stack((np.tile(core, (3, 1)), dseeds))
    rts = (np.random.default_rng(5).random((3, 6)) - 0.5)*1e-6
    kw = dict(imagersize=(W, H), optimize_extrinsics=True)
    fields = ("intrinsics", "rt_cam_ref", "cost", "rms_reproj_error__pixels", "Nevaluations", "status")
    both = fitter.fit(p, q, "LENSMODEL_OPENCV8", seeds, rt_seed=rts, **kw)
    for i in range(3):
        alone = fitter.fit(p, q, "LENSMODEL_OPENCV8", seeds[i:i + 1], rt_seed=rts[i:i + 1], **kw)
        for k in fields:
            assert np.array_equal(both[k][i], alone[k][0]), (i, k)
        assert alone["ibest"] == 0
    rms = both["rms_reproj_error__pixels"]
    print("batch: rms", rms, "status", both["status"], "evaluations", both["Nevaluations"])
    assert np.all(np.isfinite(rms)) and both["ibest"] == int(np.argmin(rms))
    again = amd.fit_lensmodel(p, q, "LENSMODEL_OPENCV8", seeds, rt_seed=rts, **kw)
    for k in fields: assert np.array_equal(both[k], again[k]), k
    assert again["ibest"] == both["ibest"]
    # a start with a NaN: stalled, its rms not finite, never the best - wherever it stands
    for ibad in (0, 2):
        s = seeds.copy(); s[ibad, 5] = np.nan
        r = fitter.fit(p, q, "LENSMODEL_OPENCV8", s, rt_seed=rts, **kw)
        assert r["status"][ibad] == 3 and not np.isfinite(r["rms_reproj_error__pixels"][ibad])
        good = [i for i in range(3) if i != ibad]
        assert r["ibest"] == good[int(np.argmin(r["rms_reproj_error__pixels"][good]))]
        for i in good:
            for k in fields: assert np.array_equal(r[k][i], both[k][i]), (ibad, i, k)
    s = seeds[:1].copy(); s[0, 0] = np.nan
    assert fitter.fit(p, q, "LENSMODEL_OPENCV8", s, rt_seed=rts[:1], **kw)["ibest"] == -1
    # too few points that take part: status 2
    w = np.zeros(len(p)); w[:5] = 1.
    r = fitter.fit(p, q, "LENSMODEL_OPENCV8", seeds, rt_seed=rts, weights=w, **kw)
    assert np.all(r["status"] == 2) and r["ibest"] == -1


@pytest.fixture(scope="module")
def real_model(amd):
    return amd.cameramodel(os.path.join(GOLDEN_DIR, "real_opencv8-0.cameramodel"))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ("intrinsics_only", "distances"))
def test_convert_sampled_end_to_end(amd, ref_api, real_model, mode):
    from mrcal_amd.lensmodel_conversion import _sample_grid, _starts
    m = amd.cameramodel(real_model)
    rt_model = np.array((0.01, 0.02, -0.015, 0.1, -0.2, 0.05))
    m.rt_cam_ref(rt_model)
    intrinsics_only = mode == "intrinsics_only"
    kw = dict(intrinsics_only=True) if intrinsics_only else dict(distance=(1., 1e3))
    m_to, info = amd.convert_lensmodel(m, "LENSMODEL_OPENCV4", sampled=True, num_trials=3, seed=7, **kw)
    assert m_to.intrinsics()[0] == "LENSMODEL_OPENCV4" and np.array_equal(m_to.imagersize(), m.imagersize())
    # the same sampled points through fit_lensmodel()
    dims = m.imagersize()
    q = _sample_grid(dims, (30, 20), None, None)
    v = amd.unproject(q, *m.intrinsics(), normalize=True)
    d = np.array((10.,) if intrinsics_only else (1., 1e3))
    p, qq = (v[None]*d[:, None, None]).reshape(-1, 3), np.tile(q, (len(d), 1))
    assert np.isfinite(p).all() and info["Npoints"] == len(p)
    seeds, rts = _starts("LENSMODEL_OPENCV4", m.intrinsics()[1][:4], 4, 3, 7, None, not intrinsics_only)
    fit = amd.fit_lensmodel(p, qq, "LENSMODEL_OPENCV4", seeds, imagersize=dims, weights=np.ones(len(p)), rt_seed=rts,
                            optimize_extrinsics=not intrinsics_only)
    for k in ("rms_reproj_error__pixels", "status", "Nevaluations", "cost"):
        assert np.array_equal(info[k], fit[k]), k
    assert info["ibest"] == fit["ibest"] == int(np.argmin(fit["rms_reproj_error__pixels"])) and np.all(fit["status"] == 0)
    assert np.array_equal(m_to.intrinsics()[1], fit["intrinsics"][fit["ibest"]])
    print(f"real_opencv8-0 as OPENCV4, {mode}: rms {info['rms_reproj_error__pixels']}, evaluations {info['Nevaluations']}")
    if intrinsics_only:
        assert np.array_equal(info["implied_Rt10"], identity_Rt()) and info["warning"] is None
    else:
        assert np.array_equal(info["implied_Rt10"], Rt_from_rt(fit["rt_cam_ref"][fit["ibest"]]))
    # (the model keeps rt: the Rt handed to it comes back through r_from_R and R_from_r, rounded)
    assert np.abs(m_to.Rt_cam_ref() - compose_Rt(info["implied_Rt10"], Rt_from_rt(rt_model))).max() < 1e-12
    # what is reported is the reference's cost at the model that came back
    C = chk.CheckerInputs(ref_api, p, qq, None, "LENSMODEL_OPENCV4", m_to.intrinsics()[1],
                          None if intrinsics_only else fit["rt_cam_ref"][fit["ibest"]], imagersize=dims)
    assert relative_error(C.cost()[1], info["rms_reproj_error__pixels"][info["ibest"]]) < 1e-10


@pytest.mark.gpu
def test_convert_sampled_warnings_come_with_info(amd, real_model):
    """what convert_lensmodel() hands on is what _moved_warning() makes of the fitted pose (its texts: the CPU test)"""
    from mrcal_amd.lensmodel_conversion import _moved_warning
    m_to, info = amd.convert_lensmodel(real_model, "LENSMODEL_PINHOLE", sampled=True, distance=(0.5,), gridn=(9, 7))
    assert info["warning"] == _moved_warning(info["implied_Rt10"], True)
    assert (info["warning_status"] is None) == (info["status"][info["ibest"]] == 0)


@pytest.mark.gpu
@pytest.mark.parametrize("intrinsics_only", (True, False))
def test_convert_sampled_splined_target(amd, ref_api, real_model, intrinsics_only):
    """A splined target is the reference's problem handed to optimize(), core locked: its rms is that of ref_api.optimize()
    of the same inputs to relative 1e-4 (what test_optimize_matches_checker holds solves to; outlier rejection is off)"""
    from mrcal_amd.lensmodel_conversion import _sample_grid, _starts, _sampled_inputs
    kw = dict(intrinsics_only=True) if intrinsics_only else dict(distance=(1., 1e3))
    m_to, info = amd.convert_lensmodel(real_model, SPLINED_SMALL, sampled=True, gridn=(12, 9), seed=1, **kw)
    assert m_to.intrinsics()[0] == SPLINED_SMALL and info["ibest"] == 0
    dims = real_model.imagersize()
    q = _sample_grid(dims, (12, 9), None, None)
    v = amd.unproject(q, *real_model.intrinsics(), normalize=True)
    d = np.array((10.,) if intrinsics_only else (1., 1e3))
    p, qq = (v[None]*d[:, None, None]).reshape(-1, 3), np.tile(q, (len(d), 1))
    Nd = amd.lensmodel_num_params(SPLINED_SMALL) - 4
    seeds, rts = _starts(SPLINED_SMALL, real_model.intrinsics()[1][:4], Nd, 1, 1, None, not intrinsics_only)
    oi = _sampled_inputs(p, qq, np.ones(len(p)), SPLINED_SMALL, seeds[0], dims, None, False)
    stats = ref_api.optimize(**oi)
    if not intrinsics_only:
        oi = _sampled_inputs(p, qq, np.ones(len(p)), SPLINED_SMALL, oi["intrinsics"][0], dims, rts[0], False)
        stats = ref_api.optimize(**oi)
    got, want = info["rms_reproj_error__pixels"][0], stats["rms_reproj_error__pixels"]
    print(f"splined target, intrinsics_only={intrinsics_only}: rms {got} (ours) {want} (reference)")
    assert relative_error(got, want, eps=0) < 1e-4
    # the core is locked
    assert np.array_equal(m_to.intrinsics()[1][:4], real_model.intrinsics()[1][:4])


@pytest.fixture(scope="module")
def solved_problem(amd):
    oi, _ = make_calibration_problem(amd._api, Ncameras=2, Nframes=6, lensmodel="LENSMODEL_OPENCV4", seed=4)
    amd.optimize(**oi)
    return oi


@pytest.mark.gpu
@pytest.mark.parametrize("monocular", (False, True))
def test_convert_from_optimization_inputs(amd, ref_api, solved_problem, monocular):
    """sampled=False: the tool's four stages through optimize() end where the same stages through ref_api.optimize()
    from the same starts end: rms_reproj_error__pixels to relative 1e-4. monocular leaves one camera at the reference
    with the frames re-based; implied_Rt10 is the Procrustes fit of the board's corners before and after"""
    from mrcal_amd.lensmodel_conversion import _convert_stages, _monocular_inputs
    icam = 1
    m = amd.cameramodel(optimization_inputs=copy_inputs(solved_problem), icam_intrinsics=icam)
    dseeds = np.array(((1e-6, -1e-6, 5e-7, -5e-7, 1e-6), (-1e-6, 1e-6, -5e-7, 5e-7, -1e-6)))
    if monocular: dseeds = dseeds[icam:icam + 1]
    m_to, info = amd.convert_lensmodel(m, "LENSMODEL_OPENCV5", sampled=False, monocular=monocular, distortion_seeds=dseeds)
    oi_to = info["optimization_inputs"]
    assert m_to.intrinsics()[0] == "LENSMODEL_OPENCV5" and oi_to["lensmodel"] == "LENSMODEL_OPENCV5"
    # the checker: the same stages, the reference's solver
    oi_ref = copy_inputs(solved_problem)
    if monocular: oi_ref = _monocular_inputs(oi_ref, icam)
    before = copy_inputs(oi_ref)
    stats = _convert_stages(oi_ref, "LENSMODEL_OPENCV5", 5, 0, dseeds, ref_api.optimize)
    got, want = info["rms_reproj_error__pixels"][0], stats["rms_reproj_error__pixels"]
    print(f"sampled=False, monocular={monocular}: rms {got} (ours) {want} (reference)")
    assert relative_error(got, want, eps=0) < 1e-4
    ic = 0 if monocular else icam
    if monocular:
        assert len(oi_to["intrinsics"]) == 1 and oi_to["rt_cam_ref"].shape == (0, 6)
        sel = solved_problem["indices_frame_camintrinsics_camextrinsics"][:, 1] == icam
        ifce = oi_to["indices_frame_camintrinsics_camextrinsics"]
        assert len(ifce) == np.count_nonzero(sel) and np.all(ifce[:, 1] == 0) and np.all(ifce[:, 2] == -1)
        assert np.array_equal(ifce[:, 0], np.arange(len(ifce)))
        # the frames re-based to the camera: before the stages they are rt_cam_ref composed with the frames it saw
        frames = solved_problem["indices_frame_camintrinsics_camextrinsics"][sel, 0]
        assert np.allclose(before["rt_ref_frame"], compose_rt(solved_problem["rt_cam_ref"][icam - 1], solved_problem["rt_ref_frame"][frames]),
                           rtol=0, atol=1e-12)
        assert m_to.icam_intrinsics() == 0
    # implied_Rt10: the Procrustes fit of the CHECKER's board points, before and after
    inl = oi_ref["observations_board"][..., 2] > 0
    assert np.array_equal(inl, oi_to["observations_board"][..., 2] > 0)
    p_before = amd.hypothesis_board_corner_positions(ic, idx_inliers=inl.copy(), **before)[-2]
    p_after  = amd.hypothesis_board_corner_positions(ic, idx_inliers=inl.copy(), **oi_ref)[-2]
    want_Rt = amd.align_procrustes_points_Rt01(p_after, p_before)
    # (two solvers of the same problem: test_optimize_matches_checker holds their states to each other by
    #  relative_error(eps=1e-3) < 1e-3, and the board's corners and their fit move with the states)
    dRt = relative_error(info["implied_Rt10"], want_Rt, eps=1e-3).max()
    print(f"    implied_Rt10 against the fit of the checker's board points: {dRt:.3g}")
    assert dRt < 1e-3
    # ... and to the bit the fit of the corners of the inputs it was made from
    mine = copy_inputs(solved_problem)
    if monocular: mine = _monocular_inputs(mine, icam)
    own = amd.align_procrustes_points_Rt01(amd.hypothesis_board_corner_positions(ic, idx_inliers=inl.copy(), **oi_to)[-2],
                                           amd.hypothesis_board_corner_positions(ic, idx_inliers=inl.copy(), **mine)[-2])
    assert np.array_equal(info["implied_Rt10"], own)
    assert np.abs(m_to.Rt_cam_ref() - compose_Rt(info["implied_Rt10"], Rt_from_rt(m.rt_cam_ref()))).max() < 1e-12


@pytest.mark.gpu
def test_device_buffers_are_given_back(amd, ref_api, real_model):
    live = amd.device_buffers_live()
    p, q = parity_case(ref_api, "LENSMODEL_OPENCV8", CAM_OPENCV8[0], (10.,))
    seed = np.concatenate((CAM_OPENCV8[0][:4], np.zeros(4)))
    amd.fit_lensmodel(p, q, "LENSMODEL_OPENCV4", seed, imagersize=(W, H))
    assert amd.device_buffers_live() == live
    with amd.LensFitter() as f:
        f.fit(p, q, "LENSMODEL_OPENCV4", seed, imagersize=(W, H))
        # more points, more trials: the buffers are exchanged, not added to
        held = amd.device_buffers_live()
        assert held > live
        f.fit(np.tile(p, (3, 1)), np.tile(q, (3, 1)), "LENSMODEL_OPENCV4", np.tile(seed, (4, 1)), imagersize=(W, H))
        assert amd.device_buffers_live() == held
        with pytest.raises(Exception, match="splined model"):
            f.fit(p, q, SPLINED_SMALL, np.zeros(4 + 96), imagersize=(W, H))
        assert amd.device_buffers_live() == held
    assert amd.device_buffers_live() == live
    amd.convert_lensmodel(real_model, "LENSMODEL_OPENCV4", sampled=True, intrinsics_only=True, gridn=(9, 7))
    assert amd.device_buffers_live() == live
