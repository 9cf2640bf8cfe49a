"""The dog-leg step on the GPU against dense numpy linear algebra and against
the CPU checker (the reference's mrcal_optimize() driving the restated
libdogleg, oracle/dogleg_restated.c).

The iteration TRAJECTORY of the real libdogleg+CHOLMOD cannot be pinned (they
are not available, see oracle/dogleg_restated.c); what is checked:
  - the normal equations JtJ, Jt x assembled on the GPU == those computed from
    the returned J with scipy (structure-independent check of the Gram path)
  - the Gauss-Newton step == numpy.linalg.solve on the dense JtJ, as the
    reference's test/test-CHOLMOD-factorization.py checks its solve
  - optimize() converges to the same optimum as the checker: packed state
    within the solver's own update_threshold (1e-7 in packed units, looser by
    conditioning), residuals within 1e-6 relative, same outliers"""
import numpy as np
import pytest

from conftest import relative_error
from mrcal_amd.synthetic import make_calibration_problem, copy_inputs, CONFIG2_LENSMODEL

pytestmark = pytest.mark.gpu


def dense_normal(J, x):
    Jd = J.toarray()
    return Jd.T @ Jd, Jd.T @ x


def blocks_to_dense(ne, Nstate):
    """reassembles the solver's block form into the dense (Nstate,Nstate) JtJ: S index s is state s below
    S_split and s + S_shift from there on, E index e is state E_state0 + e (Problem.partition())"""
    Nc, NE, Nfb = ne["Nc"], ne["NE"], ne["Nfb"]
    s = np.arange(Nc)
    sidx = np.where(s < ne["S_split"], s, s + ne["S_shift"]).astype(int)
    E0 = ne["E_state0"]
    N = np.zeros((Nstate, Nstate))
    N[np.ix_(sidx, sidx)] = ne["A"]
    for e in range(NE):
        N[E0+e, sidx] = ne["Bt"][e]
        N[sidx, E0+e] = ne["Bt"][e]
    for b in range(ne["NEb"]):
        if b < Nfb: e0, de = 6*b, 6
        else:       e0, de = 6*Nfb + 3*(b-Nfb), 3
        N[E0+e0:E0+e0+de, E0+e0:E0+e0+de] = ne["D"][b,:de,:de]
    return N


def _with_points(oi, rng, Npoints=5, Npoints_fixed=1):
    from test_callback_parity import _with_points as f
    return f(oi, rng, Npoints, Npoints_fixed)


@pytest.mark.parametrize("lensmodel", ("LENSMODEL_PINHOLE", "LENSMODEL_STEREOGRAPHIC", "LENSMODEL_OPENCV4",
                                       "LENSMODEL_OPENCV5", "LENSMODEL_OPENCV12", "LENSMODEL_CAHVOR",
                                       "LENSMODEL_CAHVORE_linearity=0.34"))
@pytest.mark.parametrize("frames_opt", (True, False))
def test_normal_equations_lens_models(amd, lensmodel, frames_opt):
    """every shape of the Gram (5, 6, 7, 8 column blocks: problem.hpp) and both
    copy-out paths (fused with the Gram for the usual rows, stand-alone otherwise),
    on boards of 100 and of 35 corners"""
    from mrcal_amd.resident import Problem
    for W, H in ((10,10), (7,5)):
        oi, _ = make_calibration_problem(amd._api, Ncameras=2, Nframes=5, lensmodel=lensmodel,
                                         object_width_n=W, object_height_n=H, seed=23)
        oi["do_optimize_frames"] = frames_opt
        with Problem(**oi) as p:
            ne = p.normal_equations()
            J, x = p.J(), p.x()
        N, g = dense_normal(J, x)
        N_gpu = blocks_to_dense(ne, p.Nstate)
        scale = np.abs(N).max()
        assert np.abs(N_gpu - N).max() < 1e-10*scale, f"{lensmodel} {W}x{H}"
        assert np.abs(ne["g"] - g).max() < 1e-10*np.abs(g).max()
        assert abs(ne["norm2_x"] - x @ x) < 1e-10*(x @ x)


@pytest.mark.parametrize("grid", ("order=3_Nx=11_Ny=8", "order=2_Nx=16_Ny=12", "order=3_Nx=40_Ny=30"))
@pytest.mark.parametrize("frames_opt,core_opt", ((True, True), (True, False), (False, True)))
def test_normal_equations_splined(amd, grid, frames_opt, core_opt):
    """the splined assembly (assembly_splined.hip assemble_splined_kernel): coarse
    grids, where every observation's knot set fits the local tile, and a fine one
    where the near boards overflow it and go row by row"""
    from mrcal_amd.resident import Problem
    oi, _ = make_calibration_problem(amd._api, Ncameras=2, Nframes=6,
                                     lensmodel=f"LENSMODEL_SPLINED_STEREOGRAPHIC_{grid}_fov_x_deg=120",
                                     object_width_n=10, object_height_n=10, seed=29)
    oi["do_optimize_frames"] = frames_opt
    oi["do_optimize_intrinsics_core"] = core_opt
    oi["observations_board"][3,2:4,1:5,2] = -1.   # some input outliers
    with Problem(**oi) as p:
        ne = p.normal_equations()
        J, x = p.J(), p.x()
    N, g = dense_normal(J, x)
    N_gpu = blocks_to_dense(ne, p.Nstate)
    scale = np.abs(N).max()
    assert np.abs(N_gpu - N).max() < 1e-10*scale
    assert np.abs(ne["g"] - g).max() < 1e-10*np.abs(g).max()
    assert abs(ne["norm2_x"] - x @ x) < 1e-10*(x @ x)


@pytest.mark.parametrize("W,H,distance", ((7, 5, 4.0), (9, 11, 4.0), (9, 11, 1.3), (3, 2, 2.0), (17, 15, 2.0), (17, 15, -1.6)))
def test_normal_equations_splined_board_sizes(amd, W, H, distance):
    """boards whose corner count is not a multiple of 4 (the Gram's k-steps), smaller than a wave, larger than the local
    tile's rows (255 corners: more than one chunk of rows a pass), far and close: the normal equations against JtJ"""
    from mrcal_amd.resident import Problem
    oi, _ = make_calibration_problem(amd._api, Ncameras=2, Nframes=5,
                                     lensmodel="LENSMODEL_SPLINED_STEREOGRAPHIC_order=3_Nx=30_Ny=20_fov_x_deg=120",
                                     object_width_n=W, object_height_n=H, seed=37, board_distance=abs(distance),
                                     object_spacing=0.1 if (W < 12 or distance < 0) else 0.06)    # (< 0: sub-boxes AND chunks of rows)
    oi["do_optimize_intrinsics_core"] = False
    with Problem(**oi) as p:
        ne = p.normal_equations()
        J, x = p.J(), p.x()
        ne2 = p.normal_equations()
    N, g = dense_normal(J, x)
    N_gpu = blocks_to_dense(ne, p.Nstate)
    assert np.abs(N_gpu - N).max() < 1e-10*np.abs(N).max()
    assert np.abs(ne["g"] - g).max() < 1e-10*np.abs(g).max()
    assert abs(ne["norm2_x"] - x @ x) < 1e-10*(x @ x)
    for k in ("A", "Bt", "D", "g"):
        assert np.array_equal(ne[k], ne2[k]), k


@pytest.mark.parametrize("distance,grid", ((1.2, "order=3_Nx=30_Ny=20"), (2.0, "order=3_Nx=30_Ny=20"), (1.5, "order=2_Nx=24_Ny=18"),
                                           (2.5, "order=3_Nx=40_Ny=30"), (-1.4, "order=3_Nx=30_Ny=20")))
def test_normal_equations_splined_closeups(amd, distance, grid):
    """Boards close to the camera: an observation's box of control points (15 x 15 of a 30 x 20 grid at 1.2 m, 18 across under a board twice the size) does
    not fit the assembly's local tile of 109, and is cut into sub-boxes that overlap by the spline's order, each a
    pass over the corners it owns (solver_kernels.hpp SPL_MAXSUB; until round 4 such observations went row by row
    with floating-point atomics). The normal equations against JtJ, and the same bits twice"""
    from mrcal_amd.resident import Problem
    oi, _ = make_calibration_problem(amd._api, Ncameras=2, Nframes=6,
                                     lensmodel=f"LENSMODEL_SPLINED_STEREOGRAPHIC_{grid}_fov_x_deg=120",
                                     object_width_n=10, object_height_n=10, seed=31, board_distance=abs(distance),
                                     object_spacing=0.2 if distance < 0 else 0.1)       # (< 0: a board twice the size)
    oi["do_optimize_intrinsics_core"] = False
    oi["observations_board"][2,1:3,4:6,2] = -1.   # some input outliers
    with Problem(**oi) as p:
        ne = p.normal_equations()
        J, x = p.J(), p.x()
        ne2 = p.normal_equations()
    # (the boxes of the observations: what this test is about)
    Nx = int(grid.split("Nx=")[1].split("_")[0])
    Jd = J.toarray()
    NPTS = 100
    i0 = p.Nstate - p.Nstate     # (the control points follow the locked core: state index 0 on)
    boxes = []
    for o in range(oi["indices_frame_camintrinsics_camextrinsics"].shape[0]):
        rows = Jd[2*NPTS*o:2*NPTS*(o+1)]
        icam = oi["indices_frame_camintrinsics_camextrinsics"][o,1]
        nk = (oi["intrinsics"].shape[1] - 4)//2
        cols = np.nonzero(np.abs(rows[:, icam*2*nk:(icam+1)*2*nk]).sum(axis=0))[0]//2
        if len(cols): boxes.append((cols % Nx).max() - (cols % Nx).min() + 1) ; boxes.append((cols // Nx).max() - (cols // Nx).min() + 1)
    print(f"distance {distance} {grid}: the observations' boxes are up to {max(boxes)} control points across")
    N, g = dense_normal(J, x)
    N_gpu = blocks_to_dense(ne, p.Nstate)
    scale = np.abs(N).max()
    assert np.abs(N_gpu - N).max() < 1e-10*scale
    assert np.abs(ne["g"] - g).max() < 1e-10*np.abs(g).max()
    assert abs(ne["norm2_x"] - x @ x) < 1e-10*(x @ x)
    for k in ("A", "Bt", "D", "g"):
        assert np.array_equal(ne[k], ne2[k]), k


def test_normal_equations_splined_with_points(amd):
    """a splined model with discrete points beside the boards: the points' rows add to the camera block with
    atomics (the generic rows), so the gather of the staged board Grams stays on the main stream, in front of them"""
    from mrcal_amd.resident import Problem
    oi, _ = make_calibration_problem(amd._api, Ncameras=2, Nframes=6,
                                     lensmodel="LENSMODEL_SPLINED_STEREOGRAPHIC_order=3_Nx=11_Ny=8_fov_x_deg=120",
                                     object_width_n=10, object_height_n=10, seed=29)
    oi["do_optimize_intrinsics_core"] = False
    oi = _with_points(oi, np.random.RandomState(3))
    # (points where this lens model sees them)
    oi["observations_point"][:,:2] = np.random.RandomState(4).uniform(700, 1300, size=oi["observations_point"][:,:2].shape)
    with Problem(**oi) as p:
        ne = p.normal_equations()
        J, x = p.J(), p.x()
        d = p.gauss_newton_step()
    N, g = dense_normal(J, x)
    N_gpu = blocks_to_dense(ne, p.Nstate)
    assert np.abs(N_gpu - N).max() < 1e-10*np.abs(N).max()
    assert np.abs(ne["g"] - g).max() < 1e-10*np.abs(g).max()
    assert abs(ne["norm2_x"] - x @ x) < 1e-10*(x @ x)
    assert np.abs(N @ d + g).max() < 1e-6*max(np.abs(g).max(), 1.0)


def _same_normal_equations_three_times(p):
    runs = [p.normal_equations() for _ in range(3)]
    for r in runs[1:]:
        for k in ("A", "Bt", "D", "g"):
            assert np.array_equal(r[k], runs[0][k]), k
        assert r["norm2_x"] == runs[0]["norm2_x"]
    return runs[0]


def test_splined_points_with_optimized_distortions_are_bit_reproducible(amd):
    """Round 5, the first of the two places where the order of floating-point atomics still showed: discrete points under
    a splined model whose control points are optimized (a point row's 16 patch columns move with every evaluation: no
    fixed-order plan). Their rows now go through sums in which no addition rounds (solver_kernels.hpp ReproStep): the
    normal equations against JtJ, the same bits three times, and the same solve twice"""
    from mrcal_amd.resident import Problem
    oi, _ = make_calibration_problem(amd._api, Ncameras=2, Nframes=6,
                                     lensmodel="LENSMODEL_SPLINED_STEREOGRAPHIC_order=3_Nx=16_Ny=12_fov_x_deg=120",
                                     object_width_n=10, object_height_n=10, seed=29)
    oi["do_optimize_intrinsics_core"] = False
    oi = _with_points(oi, np.random.RandomState(3), Npoints=40)
    oi["observations_point"][:,:2] = np.random.RandomState(4).uniform(700, 3300, size=oi["observations_point"][:,:2].shape)
    oi["observations_point"][:,1]  = np.random.RandomState(5).uniform(500, 1700, size=oi["observations_point"].shape[0])
    assert oi["do_optimize_intrinsics_distortions"]
    with Problem(**copy_inputs(oi)) as p:
        ne = _same_normal_equations_three_times(p)
        J, x = p.J(), p.x()
    N, g = dense_normal(J, x)
    N_gpu = blocks_to_dense(ne, p.Nstate)
    assert np.abs(N_gpu - N).max() < 1e-10*np.abs(N).max()
    assert np.abs(ne["g"] - g).max() < 1e-10*np.abs(g).max()
    assert abs(ne["norm2_x"] - x @ x) < 1e-10*(x @ x)
    runs = []
    for i in range(2):
        with Problem(**copy_inputs(oi)) as p:
            s = p.solve()
            runs.append((s["Niterations"], s["Nevaluations"], s["norm2_x"], p.b_packed()))
    assert runs[0][:3] == runs[1][:3] and np.array_equal(runs[0][3], runs[1][3])
    assert runs[0][0] > 3


def test_splined_board_over_more_than_twelve_sub_boxes_is_bit_reproducible(amd):
    """... and the second: a board observation whose box of control points is past the assembly's twelve sub-boxes - a
    40 x 30 grid under a board that fills the imager. Its rows took the row-by-row atomics until round 5; now the same
    pre-rounded sums: JtJ, the same bits three times, the same solve twice"""
    from mrcal_amd.resident import Problem
    LM, W, H, SP = "LENSMODEL_SPLINED_STEREOGRAPHIC_order=3_Nx=40_Ny=30_fov_x_deg=120", 15, 7, 0.15
    oi, truth = make_calibration_problem(amd._api, Ncameras=1, Nframes=5, lensmodel=LM,
                                         object_width_n=W, object_height_n=H, seed=31, object_spacing=SP)
    oi["do_optimize_intrinsics_core"] = False
    # frame 0: the board square in front of the camera, 0.75 m away - 2.1 m wide: all but the edge of the imager
    rt0 = np.array((0.02, -0.03, 0.01, -(W-1)*SP/2., -(H-1)*SP/2., 0.75))
    obs1 = np.zeros((1, H, W, 3)); obs1[...,2] = 1.
    q = amd._api.optimizer_callback(intrinsics=truth["intrinsics"], rt_cam_ref=truth["rt_cam_ref"], rt_ref_frame=rt0[None],
                                    observations_board=obs1, indices_frame_camintrinsics_camextrinsics=np.array(((0,0,-1),), dtype=np.int32),
                                    lensmodel=LM, imagersizes=oi["imagersizes"], calobject_warp=truth["calobject_warp"],
                                    calibration_object_spacing=SP, do_optimize_calobject_warp=False, do_apply_regularization=False,
                                    no_jacobian=True, no_factorization=True)[1][:2*W*H].reshape(H, W, 2)
    assert q[...,0].min() > 0 and q[...,0].max() < 3999 and q[...,1].min() > 0 and q[...,1].max() < 2199
    oi["observations_board"][0,:,:,:2] = q + np.random.RandomState(6).normal(0, 0.3, q.shape)
    oi["rt_ref_frame"][0] = rt0 + np.array((1e-3, -1e-3, 1e-3, 5e-3, -5e-3, 5e-3))
    oi["observations_board"][2,1:3,4:6,2] = -1.
    with Problem(**copy_inputs(oi)) as p:
        ne = _same_normal_equations_three_times(p)
        J, x = p.J(), p.x()
    # the boxes: at least one observation must be past 12 sub-boxes of <= 10 x 10 that overlap by 3 (more than 31 x 24)
    Nx, NPTS = 40, W*H
    big = 0
    Jc = J.tocsr()
    for o in range(oi["indices_frame_camintrinsics_camextrinsics"].shape[0]):
        rows = Jc[2*NPTS*o:2*NPTS*(o+1)]
        cols = np.unique(rows.indices[rows.indices < 2*40*30])//2
        if len(cols):
            w, h = (cols % Nx).max() - (cols % Nx).min() + 1, (cols // Nx).max() - (cols // Nx).min() + 1
            nsx, nsy = max(1, (w - 3 + 6)//7), max(1, (h - 3 + 6)//7)
            big = max(big, nsx*nsy)
    assert big > 12, f"the largest observation takes {big} sub-boxes: the test does not reach the rows it is about"
    N, g = dense_normal(J, x)
    N_gpu = blocks_to_dense(ne, p.Nstate)
    assert np.abs(N_gpu - N).max() < 1e-10*np.abs(N).max()
    assert np.abs(ne["g"] - g).max() < 1e-10*np.abs(g).max()
    assert abs(ne["norm2_x"] - x @ x) < 1e-10*(x @ x)
    runs = []
    for i in range(2):
        with Problem(**copy_inputs(oi)) as p:
            s = p.solve()
            runs.append((s["Niterations"], s["Nevaluations"], s["norm2_x"], p.b_packed()))
    assert runs[0][:3] == runs[1][:3] and np.array_equal(runs[0][3], runs[1][3])


@pytest.mark.parametrize("case", ("boards", "boards+points", "no-extrinsics-opt", "monocular"))
def test_normal_equations_match_JtJ(amd, case):
    from mrcal_amd.resident import Problem
    rng = np.random.RandomState(2)
    Ncam = 1 if case == "monocular" else 3
    oi, _ = make_calibration_problem(amd._api, Ncameras=Ncam, Nframes=6, lensmodel="LENSMODEL_OPENCV8",
                                     object_width_n=10, object_height_n=10, seed=21)
    if case == "boards+points":
        oi = _with_points(oi, rng)
    if case == "no-extrinsics-opt":
        oi["do_optimize_extrinsics"] = False
        oi["do_optimize_calobject_warp"] = False
    oi["observations_board"][2,3:5,1:4,2] = -1.   # some input outliers
    with Problem(**oi) as p:
        ne = p.normal_equations()
        J, x = p.J(), p.x()
    N, g = dense_normal(J, x)
    N_gpu = blocks_to_dense(ne, p.Nstate)
    scale = np.abs(N).max()
    assert np.abs(N_gpu - N).max() < 1e-10*scale
    assert np.abs(ne["g"] - g).max() < 1e-10*np.abs(g).max()
    assert abs(ne["norm2_x"] - x @ x) < 1e-10*(x @ x)


# camera blocks of 30 (one LDS-resident Cholesky), 212 (past the LDS kernel: the
# panel-by-panel Cholesky in HBM, three full 64-column panels and a partial one)
# and 780 variables (splined: 13 panels)
# ... and the panel edges of the LDS kernel (panels of 16): camera blocks of exactly 16 and 32
# variables, one past (18), one short of three panels (46), a big one that still fits the LDS (170),
# and 178 = 14 x 13 - 4 (OPENCV4, 13 cameras): the largest the kept factor's LDS triangular solve takes, of the <= 180 the
# LDS Cholesky factors (every size between: tests/test_factorization_sizes.py)
@pytest.mark.parametrize("lensmodel,Ncam,Nf,W,H", (("LENSMODEL_OPENCV4", 2, 8, 8, 7),
                                                   ("LENSMODEL_PINHOLE", 2, 8, 8, 7),
                                                   ("LENSMODEL_OPENCV8", 2, 8, 8, 7),
                                                   ("LENSMODEL_OPENCV12", 1, 8, 8, 7),
                                                   ("LENSMODEL_PINHOLE", 5, 8, 8, 7),
                                                   ("LENSMODEL_OPENCV12", 8, 6, 10, 10),
                                                   ("LENSMODEL_OPENCV8", 12, 6, 10, 10),
                                                   ("LENSMODEL_OPENCV4", 13, 4, 8, 7),
                                                   # whole panels of the launch-per-panel Cholesky: 192 = 3 x 64, 256 = 4 x 64
                                                   ("LENSMODEL_OPENCV4", 14, 6, 8, 7),
                                                   ("LENSMODEL_PINHOLE", 26, 5, 8, 7),
                                                   ("LENSMODEL_SPLINED_STEREOGRAPHIC_order=3_Nx=16_Ny=12_fov_x_deg=120", 2, 40, 10, 10)))
def test_gauss_newton_step_matches_dense_solve(amd, lensmodel, Ncam, Nf, W, H):
    from mrcal_amd.resident import Problem
    oi, _ = make_calibration_problem(amd._api, Ncameras=Ncam, Nframes=Nf, lensmodel=lensmodel,
                                     object_width_n=W, object_height_n=H, seed=4)
    with Problem(**oi) as p:
        d = p.gauss_newton_step()
        J, x = p.J(), p.x()
    N, g = dense_normal(J, x)
    d_ref = -np.linalg.solve(N, g)
    # what the solve can deliver is set by the conditioning of JtJ: compare through
    # the residual of the normal equations as well as entry by entry
    assert np.abs(N @ d + g).max() < 1e-7*max(np.abs(g).max(), 1.0)
    # entry by entry: 1e-6, or what the conditioning leaves of a double-precision solve (either one's)
    tol = max(1e-6, 10.*np.linalg.cond(N)*np.finfo(float).eps)
    assert relative_error(d, d_ref, eps=1e-9*np.abs(d_ref).max()).max() < tol


def _solve_both(amd, ref_api, oi):
    oa, orr = copy_inputs(oi), copy_inputs(oi)
    sa = amd.optimize(**oa)
    sr = ref_api.optimize(**orr)
    return oa, sa, orr, sr


# CAHVOR: the optical-axis angles trade off against the centre pixel almost
# exactly; along that valley the two solvers stop up to ~1e-3 packed units apart
@pytest.mark.parametrize("lensmodel,Ncam,Nf,btol", (("LENSMODEL_OPENCV4", 1, 12, 2e-5),
                                                     ("LENSMODEL_OPENCV8", 3, 10, 2e-5),
                                                     ("LENSMODEL_PINHOLE", 2, 8,  2e-5),
                                                     ("LENSMODEL_CAHVOR",  2, 8,  2e-3)))
def test_optimize_matches_checker(amd, ref_api, lensmodel, Ncam, Nf, btol):
    oi, truth = make_calibration_problem(amd._api, Ncameras=Ncam, Nframes=Nf, lensmodel=lensmodel,
                                         object_width_n=10, object_height_n=10, seed=31)
    oa, sa, orr, sr = _solve_both(amd, ref_api, oi)

    assert sa["Noutliers_board"] == sr["Noutliers_board"]
    # same outliers marked in the caller's array
    assert np.array_equal(oa["observations_board"][...,2] < 0, orr["observations_board"][...,2] < 0)
    if lensmodel == "LENSMODEL_CAHVOR":
        # The valley again, seen from the other side (round 5): the two solvers are the same algorithm in different
        # arithmetic, and in CAHVOR's valley a difference in the last bit of a residual decides whether the
        # 1e-7-step termination test fires at a given trial. Until round 5 both stopped at the SAME premature point
        # (|Jt x|/(|J||x|) = 1.3e-3, rms 1.4868517); since the board kernel was recompiled for the one-launch trial
        # step (other contractions of multiply-adds, other last bits) the product walks on to the stationary point
        # (4e-11, rms 1.4868245, 1.2 packed units along the valley) where scipy finds nothing more to gain, while
        # from the checker's end it still finds 3.6e-5 (tools/exp/dbg_cahvor.py). So here the arbiter decides
        # (tests/arbiter.py): wherever the checker is NOT at a stationary point the product must be no worse
        st_a, cost_a, gain_a = _solve_report(ref_api, "product", oa, sa)
        st_r, cost_r, gain_r = _solve_report(ref_api, "checker", orr, sr)
        if st_r >= 1e-6:
            assert cost_a <= cost_r*(1. + 1e-6), (cost_a, cost_r)
            assert st_a <= st_r and gain_a <= max(gain_r, 1e-9), (st_a, st_r, gain_a, gain_r)
            assert abs(sa["rms_reproj_error__pixels"] - sr["rms_reproj_error__pixels"]) < 1e-4*sr["rms_reproj_error__pixels"]
            return
    assert abs(sa["rms_reproj_error__pixels"] - sr["rms_reproj_error__pixels"]) < \
        1e-6*sr["rms_reproj_error__pixels"]
    # the optimum. Both stop when a step is shorter than 1e-7 (packed units)
    db = np.abs(sa["b_packed"] - sr["b_packed"])
    assert db.max() < btol, f"packed state differs by {db.max()} at {db.argmax()}"
    for k in ("intrinsics", "rt_cam_ref", "rt_ref_frame", "calobject_warp"):
        if oa[k] is not None and oa[k].size:
            # weakly-determined directions (high-order distortions) stop wherever
            # the last sub-1e-7 step left them: the cost there is flat
            assert relative_error(oa[k], orr[k], eps=1e-3).max() < max(1e-3, 50*btol), k
    # residuals at the optimum (weighted pixels): both solvers stop within a
    # 1e-7 packed-units step of it, so compare absolutely
    assert np.abs(sa["x"] - sr["x"]).max() < 1e-5
    assert abs(np.linalg.norm(sa["x"]) - np.linalg.norm(sr["x"])) < 1e-7*np.linalg.norm(sr["x"])


# the partial solves every calibration starts with (mrcal-calibrate-cameras:412-460: the geometry alone, then
# geometry + core): camera blocks of 0, 6 and 4 variables
@pytest.mark.parametrize("Ncam,sel", ((1, dict(do_optimize_intrinsics_core=False, do_optimize_intrinsics_distortions=False)),
                                      (2, dict(do_optimize_intrinsics_core=False, do_optimize_intrinsics_distortions=False)),
                                      (1, dict(do_optimize_intrinsics_core=True,  do_optimize_intrinsics_distortions=False)),
                                      (2, dict(do_optimize_frames=False))))
def test_optimize_partial_selections(amd, ref_api, Ncam, sel):
    oi, truth = make_calibration_problem(amd._api, Ncameras=Ncam, Nframes=9, lensmodel="LENSMODEL_OPENCV4",
                                         object_width_n=10, object_height_n=10, seed=12, make_outliers=False)
    oi.update(sel)
    oi.update(do_optimize_calobject_warp=False, do_apply_regularization=False, do_apply_outlier_rejection=False,
              calobject_warp=None)
    oa, sa, orr, sr = _solve_both(amd, ref_api, oi)
    assert abs(sa["rms_reproj_error__pixels"] - sr["rms_reproj_error__pixels"]) < 1e-6*sr["rms_reproj_error__pixels"]
    assert np.abs(sa["b_packed"] - sr["b_packed"]).max() < 2e-5
    assert np.abs(sa["x"] - sr["x"]).max() < 1e-5


def test_optimize_recovers_truth(amd):
    """noise-free observations -> the solve must land on |x| ~ 0
    (test-basic-calibration.py:366-385 asserts |x|<1e-8 for perfect data)"""
    oi, truth = make_calibration_problem(amd._api, Ncameras=2, Nframes=10, lensmodel="LENSMODEL_OPENCV4",
                                         object_width_n=10, object_height_n=9,
                                         pixel_noise=0.0, make_outliers=False, seed=8)
    oi["do_apply_regularization"] = False
    s = amd.optimize(**oi)
    assert s["rms_reproj_error__pixels"] < 1e-6
    assert np.abs(oi["calobject_warp"] - truth["calobject_warp"]).max() < 1e-6


def _solve_report(ref_api, name, o, s):
    import arbiter
    st, cost, _ = arbiter.stationarity(ref_api, o)
    gain = arbiter.least_squares_gain(ref_api, o)
    print(f"{name}: rms {s['rms_reproj_error__pixels']:.10g}, {s['Noutliers_board']} outliers, cost {cost!r}; "
          f"|Jt x|/(|J||x|) = {st:.3g}; scipy least_squares(trf, x_scale=jac) lowers the cost by {gain:.3g} relative")
    return st, cost, gain


def _compare_splined_solves(amd, ref_api, oi, rms_tol, btol):
    """Both solves (outlier rejection as the problem says), then the arbiter (tests/arbiter.py: the reference's own
    callback + numpy + scipy.optimize.least_squares, no code of either solver) at both returned states, the
    returned outlier weights in place. Where the checker converged the product must have: same outliers, rms to
    rms_tol, stationary, and nothing left for least_squares to find (1e-9 relative). Where the checker was
    stopped by mrcal's 300-iteration limit (mrcal.c:6299) short of a stationary point, so is everybody: the two
    are then compared at the limit (same outliers, the rms to rms_tol, the product's cost no higher)"""
    oa, sa, orr, sr = _solve_both(amd, ref_api, oi)
    st_a, cost_a, gain_a = _solve_report(ref_api, "product", oa, sa)
    st_r, cost_r, gain_r = _solve_report(ref_api, "checker", orr, sr)
    assert sa["Noutliers_board"] == sr["Noutliers_board"]
    assert np.array_equal(oa["observations_board"][...,2] < 0, orr["observations_board"][...,2] < 0)
    assert abs(sa["rms_reproj_error__pixels"] - sr["rms_reproj_error__pixels"]) < rms_tol*sr["rms_reproj_error__pixels"]
    if st_r < 1e-6:
        # (_check_solve's bound on the gradient is 1e-5; the converged solves observed here sit at 1e-9 .. 1e-11)
        assert st_a < 1e-6, st_a
        assert gain_a < 1e-9, gain_a
        db = np.abs(sa["b_packed"] - sr["b_packed"])
        assert db.max() < btol, f"packed state differs by {db.max()} at {db.argmax()}"
    else:
        assert cost_a <= cost_r*(1. + 2*rms_tol), (cost_a, cost_r)
    return oa, sa


def test_optimize_splined(amd, ref_api):
    """a splined-stereographic solve (core locked, as mrcal-calibrate-cameras does for these models:
    mrcal-calibrate-cameras:641-643): the row-by-row normal equations and the large-camera-block Cholesky path,
    against the reference's mrcal_optimize() at the SAME optimum, like every other lens model.

    (Until round 4 this test could only ask for "no worse than the checker": the restated libdogleg kept the
    symbolic analysis of the FIRST Jacobian while the splined models move a row's columns with the corner
    (mrcal.c:4718-4817), read the values of later Jacobians through the stale map, declared matrices "not positive
    definite" that LAPACK factors without trouble (tools/diag_splined_pd.py, profiles/r04_splined_checker_defect.txt)
    and crawled through lambda to its iteration limit. CHOLMOD's simplicial factorization, which libdogleg selects,
    is correct for any pattern; the restatement now redoes its analysis when the pattern moved)"""
    oi, truth = make_calibration_problem(amd._api, Ncameras=1, Nframes=30,
                                         lensmodel="LENSMODEL_SPLINED_STEREOGRAPHIC_order=3_Nx=11_Ny=8_fov_x_deg=120",
                                         object_width_n=10, object_height_n=10, seed=33)
    oi["do_optimize_intrinsics_core"]  = False
    oi["do_apply_outlier_rejection"]   = False
    oa, sa = _compare_splined_solves(amd, ref_api, oi, rms_tol=1e-6, btol=2e-4)
    # restart from the solution: nothing left to gain
    sa2 = amd.optimize(**oa)
    assert abs(sa2["rms_reproj_error__pixels"] - sa["rms_reproj_error__pixels"]) < 1e-7*sa["rms_reproj_error__pixels"]


@pytest.mark.timeout(900)
def test_optimize_splined_closeups(amd, ref_api):
    """A splined solve whose boards are close to the camera (1.5 m: an observation covers up to ~15 x 15 of the 30 x 20
    control points, more than the assembly's local tile holds: the sub-boxes of solver_kernels.hpp) against the
    reference's mrcal_optimize() at the same optimum - and again from the same inputs: the same bits (these
    observations went row by row with floating-point atomics until round 4)"""
    oi, truth = make_calibration_problem(amd._api, Ncameras=1, Nframes=40,
                                         lensmodel="LENSMODEL_SPLINED_STEREOGRAPHIC_order=3_Nx=30_Ny=20_fov_x_deg=120",
                                         object_width_n=10, object_height_n=10, seed=35, board_distance=1.5)
    oi["do_optimize_intrinsics_core"]  = False
    oi["do_apply_outlier_rejection"]   = False
    oa, sa = _compare_splined_solves(amd, ref_api, oi, rms_tol=1e-6, btol=5e-3)
    ob = copy_inputs(oi)
    sb = amd.optimize(**ob)
    assert sb["rms_reproj_error__pixels"] == sa["rms_reproj_error__pixels"]
    for k in ("intrinsics", "rt_ref_frame", "calobject_warp"):
        assert np.array_equal(np.asarray(oa[k]), np.asarray(ob[k])), k


@pytest.mark.timeout(900)
@pytest.mark.parametrize("seed,icase", ((23, 22), (11, 29), (11, 120)))
def test_optimize_splined_disputed_fuzz_cases(amd, ref_api, seed, icase):
    """The splined problems of the round-3 fuzz sweeps on which product and checker ended apart
    (profiles/r03_fuzz_parity.txt: 1.18 vs 1.30 px with 15 vs 11 outliers, 0.955 vs 1.187, 1.3286 vs 1.3760),
    rebuilt from the sweep's seed and the case number. With the checker's stale-analysis defect fixed (above) they
    end together; the arbiter says where each of them is"""
    import os, sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import fuzz_parity
    rng = np.random.RandomState(seed)
    for ic, what, oi, *_ in fuzz_parity.board_cases(icase + 1, rng, amd._api):
        if ic == icase: break
    print(f"sweep {seed} {what}")
    assert "SPLINED" in what
    # (observed on the GPU, product vs checker: 1.181360119 / 1.181360119 px, both stationary to 1e-9, the cost equal to 2e-11
    #  relative; 0.9552799354 / 0.9552800459 and 1.328582106 / 1.328582082, both stopped by the iteration limit. The state of
    #  case 22 - 5 boards under 88 knots x 3 cameras - differs by 1.8e-3 packed units in ONE knot value that no corner sees and
    #  the regularization alone holds: the bound on the state is 5e-3 here, the cost and the outliers are what pins the solve)
    # (round 5, -ffp-contract=on: that knot value ends 5.2e-3 away; the bound is 1e-2 now)
    _compare_splined_solves(amd, ref_api, oi, rms_tol=2e-5, btol=1e-2)


@pytest.mark.timeout(900)
def test_optimize_splined_reduced_configuration_2(amd, ref_api):
    """BASELINE.json's configuration 2 (1 camera, SPLINED_STEREOGRAPHIC 30 x 20 knots, core locked) with 200 of its
    800 frames - the camera block is the full 1200 variables: assemble_splined, the sparse SYRK, the panel-by-panel
    Cholesky -, solved with outlier rejection by the product and by the reference's mrcal_optimize() (15 s of one
    host core), then judged by the arbiter"""
    oi, _ = make_calibration_problem(amd._api, Ncameras=1, Nframes=200, object_width_n=10, object_height_n=10,
                                     lensmodel=CONFIG2_LENSMODEL,
                                     seed=4, do_optimize_intrinsics_core=False)
    assert amd.num_states(**oi) == 2*30*20 + 6*200 + 2
    _compare_splined_solves(amd, ref_api, oi, rms_tol=1e-6, btol=1e-3)


def test_solve_without_the_jacobian_stream(amd):
    """Round 6: a solve may leave the CSR values of J unwritten (nothing in the device-side dog leg reads them;
    mrcal_optimize() returns no Jacobian: /root/reference/mrcal.h:453-521). The board kernel then forms the same rows,
    residuals and Grams by the same instructions: everything a solve returns must be THE SAME BITS with the stream on
    and off - on every kind of board kernel (all variables optimized: the fused Gram + copy-out loop; a locked block:
    the general one; boards of 7x5: partial halves; discrete points and pairs beside the boards; the splined model,
    which ignores the switch) -, and J, asked for after a solve without the stream, must be the Jacobian AT the
    solution (made on demand), not what an earlier evaluation left there. The drop-in optimize() likewise, under
    set_optimize_jacobian_stream()"""
    from mrcal_amd.resident import Problem
    from test_callback_parity import _with_points
    from mrcal_amd.synthetic import make_sfm_problem
    cases = []
    for nc, nf, lm, kw in ((3, 12, "LENSMODEL_OPENCV8", {}), (2, 9, "LENSMODEL_OPENCV4", {}), (2, 7, "LENSMODEL_PINHOLE", {}),
                           (2, 10, "LENSMODEL_OPENCV5", {}), (2, 8, "LENSMODEL_CAHVOR", {}),
                           (2, 9, "LENSMODEL_OPENCV8", dict(object_width_n=7, object_height_n=5)),
                           (4, 150, "LENSMODEL_OPENCV8", {}),
                           (1, 12, "LENSMODEL_SPLINED_STEREOGRAPHIC_order=3_Nx=16_Ny=12_fov_x_deg=120", dict(do_optimize_intrinsics_core=False))):
        oi, _ = make_calibration_problem(amd._api, Ncameras=nc, Nframes=nf, lensmodel=lm, seed=5, **kw)
        cases.append((f"{nc}x{nf} {lm} {kw}", oi))
    oi, _ = make_calibration_problem(amd._api, Ncameras=3, Nframes=14, lensmodel="LENSMODEL_OPENCV8", seed=6)
    oi["do_optimize_intrinsics_distortions"] = False
    cases.append(("distortions locked", oi))
    oi, _ = make_calibration_problem(amd._api, Ncameras=3, Nframes=20, lensmodel="LENSMODEL_OPENCV8", seed=7)
    cases.append(("boards + discrete points", _with_points(oi, np.random.RandomState(1), Npoints=30, Npoints_fixed=2)))
    oi = make_sfm_problem("LENSMODEL_OPENCV4", Ncam=4, Npoints=300, seed=6, noise=0.3, Nboard_frames=20)[0]
    oi["do_apply_outlier_rejection"] = True
    cases.append(("boards + triangulated pairs", oi))

    for what, oi in cases:
        res = []
        for stream in (True, False):
            with Problem(**copy_inputs(oi)) as p:
                assert p.set_jacobian_stream(stream) is True
                s = p.solve()
                J = p.J()
                res.append((s, p.b_packed(), p.x(), J.data.copy(), p.jacobian_stream_is_optional()))
                # J is the Jacobian AT the solution: what a fresh evaluation there gives
                p.evaluate(with_jacobian=True)
                assert np.array_equal(p.J().data, J.data), what
        (s0, b0, x0, J0, opt0), (s1, b1, x1, J1, opt1) = res
        assert opt0 == opt1 == ("SPLINED" not in what), what
        for k in ("Niterations", "Nevaluations", "Nfactorizations", "Noutlier_passes", "Noutliers_board", "norm2_x",
                  "rms_reproj_error__pixels"):
            assert s0[k] == s1[k], (what, k, s0[k], s1[k])
        assert np.array_equal(b0, b1), what
        assert np.array_equal(x0, x1), what
        assert np.array_equal(J0, J1), what

    # the drop-in: by default without the stream; with it on request; the same bits
    import mrcal_amd
    oi = cases[0][1]
    outs = []
    for stream in (False, True, False):
        prev = mrcal_amd.set_optimize_jacobian_stream(stream)
        try:
            o = copy_inputs(oi)
            outs.append((amd.optimize(**o), o))
        finally:
            mrcal_amd.set_optimize_jacobian_stream(prev)
    assert mrcal_amd.set_optimize_jacobian_stream(False) is False        # (the default, and what the loop restored)
    for s, o in outs[1:]:
        assert np.array_equal(s["b_packed"], outs[0][0]["b_packed"]) and np.array_equal(s["x"], outs[0][0]["x"])
        assert s["Noutliers_board"] == outs[0][0]["Noutliers_board"]
        assert np.array_equal(o["observations_board"], outs[0][1]["observations_board"])


@pytest.mark.timeout(900)
def test_solve_through_the_explicit_inverse_matches_the_backward_sweep(amd):
    """ADVICE r4 / VERDICT r5 item 5: the big camera block's solve ends with d = -L^-T z as a product with an explicitly
    formed L^-1 (launch_cholesky_large: no backward sweep), and multiplying by an explicit inverse is not backward stable -
    its error grows with cond(L), and the splined camera blocks have cond(JtJ) ~ 1e13. Configuration 2 reduced to 200
    frames, in three processes:
      inverse    the default. The Gauss-Newton step at the seed against the blocks themselves: the residual of
                 N d = -g, relative to |N| |d|, is what a backward-stable solve leaves (a few eps) to within 1e3
      sweep      the test hook lchol_sweep: the triangular sweep of rounds 2-3 (which also turns the compaction of the
                 camera block off) from the start: the same outliers, the same optimum, the same kind of residual
      fallback   round 6's automatic fallback, its threshold raised from 1e-10 to 1e-2 by the test hook
                 lchol_fallback_log10 so that this problem (whose factors' diagonals span 1e5 - 1e7) trips it: the first pass
                 runs through the explicit inverse, the solver says so on stderr and switches the problem to the sweep
                 for the passes that follow - and the solve ends where the others end"""
    import os, subprocess, sys, json
    code = r'''
import sys, os, json, numpy as np
sys.path.insert(0, %r)
import mrcal_amd
for _kv in os.environ.get("TEST_HOOKS", "").split(","):          # (the test's own variable: hooks of the library's test API)
    if _kv: mrcal_amd.set_test_hook(_kv.split("=")[0], int(_kv.split("=")[1]))
from mrcal_amd.synthetic import make_calibration_problem, copy_inputs, CONFIG2_LENSMODEL
from mrcal_amd.resident import Problem
oi, _ = make_calibration_problem(mrcal_amd._api, Ncameras=1, Nframes=200, object_width_n=10, object_height_n=10,
                                 lensmodel=CONFIG2_LENSMODEL, seed=4, do_optimize_intrinsics_core=False)
with Problem(**copy_inputs(oi)) as p:
    d0 = p.gauss_newton_step()
    ne = p.normal_equations()
    # N d + g by blocks: N = [A B; Bt D] in (S, E) order, the state in the reference's order
    Nie, NE, Nw = ne["Nie"], ne["NE"], ne["Nwarp"]
    dS = np.concatenate((d0[:Nie], d0[Nie+NE:Nie+NE+Nw])); dE = d0[Nie:Nie+NE]
    gS = np.concatenate((ne["g"][:Nie], ne["g"][Nie+NE:Nie+NE+Nw])); gE = ne["g"][Nie:Nie+NE]
    DdE = np.einsum("bij,bj->bi", ne["D"], dE.reshape(-1, 6)).ravel()
    rS = ne["A"] @ dS + ne["Bt"].T @ dE + gS
    rE = ne["Bt"] @ dS + DdE + gE
    normN = max(np.abs(ne["A"]).max(), np.abs(ne["Bt"]).max(), np.abs(ne["D"]).max())
    resid = max(np.abs(rS).max(), np.abs(rE).max())/(normN*np.abs(d0).max()*d0.size)
    s = p.solve()
    print("RESULT " + json.dumps(dict(N=s["Niterations"], Nout=s["Noutliers_board"], rms=s["rms_reproj_error__pixels"], b=p.b_packed().tolist(),
                                      resid=resid, sweep=p.uses_sweep(), ratio=p.lchol_diag_ratio())))
''' % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))),)
    res, err = {}, {}
    for tag, env in (("inverse", {}), ("sweep", {"TEST_HOOKS": "lchol_sweep=1"}), ("fallback", {"TEST_HOOKS": "lchol_fallback_log10=-2"})):
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=800)
        assert r.returncode == 0, r.stderr[-2000:]
        res[tag] = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
        err[tag] = r.stderr
    a, b, c = res["inverse"], res["sweep"], res["fallback"]
    print(f"inverse: {a['N']} iterations, rms {a['rms']!r}, residual of the first step {a['resid']:.2e}, diagonal min/max {a['ratio']:.2e}; "
          f"sweep: {b['N']} iterations, rms {b['rms']!r}, residual {b['resid']:.2e}; fallback: {c['N']} iterations, rms {c['rms']!r}")
    assert a["sweep"] is False and b["sweep"] is True and c["sweep"] is True
    assert 1e-9 < a["ratio"] < 1e-2, a["ratio"]                 # (what the fallback's threshold is compared with: between its default and the test's)
    assert "backward sweep from here on" in err["fallback"] and "backward sweep from here on" not in err["inverse"]
    assert a["resid"] < 1e-12 and b["resid"] < 1e-12, (a["resid"], b["resid"])
    for x in (b, c):
        assert a["Nout"] == x["Nout"]
        assert abs(a["rms"] - x["rms"]) < 1e-8*x["rms"]
        assert np.abs(np.array(a["b"]) - np.array(x["b"])).max() < 1e-4


def test_nested_dissection_of_the_control_point_grid(amd):
    """The splined models with one camera (cholesky_large.hip lchol_nd_*): where the boards leave a strip of the grid worth
    having, the coupled control points are ordered [side A | side B | strip], the two sides' panels of the big Cholesky
    are factored side by side, and the solve ends with d_A = -Y_A^T (z_A + L_SA^T d_S). Configuration 2 reduced to 200
    frames, solved
      - as it is: the dissection is in use (launches provided, the final point's plan active, both sides >= a panel),
        and the plan is the one the planner restated on the host makes from the final point's Jacobian;
      - the same again: the same bits (every sum of it in a fixed order);
      - with the separator's panels past the first left to lchol_tail_kernel: the same bits;
      - with launches for ONE round where the plan needs more (the test hook nd_rounds = 1): no plan fits, every point goes the
        ordinary way THROUGH the dissection's launches - the bits of
      - the solve without the dissection (MRCAL_AMD_NO_ND=1), which the solve with it matches to what another order of
        the pivots leaves"""
    import os, subprocess, sys, json
    code = r'''
import sys, os, json, numpy as np
sys.path.insert(0, %r)
import mrcal_amd
for _kv in os.environ.get("TEST_HOOKS", "").split(","):          # (the test's own variable: hooks of the library's test API)
    if _kv: mrcal_amd.set_test_hook(_kv.split("=")[0], int(_kv.split("=")[1]))
from mrcal_amd.synthetic import make_calibration_problem, copy_inputs, CONFIG2_LENSMODEL
from mrcal_amd.resident import Problem
oi, _ = make_calibration_problem(mrcal_amd._api, Ncameras=1, Nframes=200, object_width_n=10, object_height_n=10,
                                 lensmodel=CONFIG2_LENSMODEL, seed=4, do_optimize_intrinsics_core=False)
def restated_plan(p, nd):
    # the planner of spl_compact_body() again, from the final point's Jacobian: the boxes of control points under the boards
    # (columns with a value in the board's rows), the covered rectangle of every box, the cheapest strip that fits
    lm = oi["lensmodel"]
    Nx = int(lm.split("Nx=")[1].split("_")[0]); Ny = int(lm.split("Ny=")[1].split("_")[0]); nk = Nx*Ny
    J = p.J().tocsr()
    Nc = mrcal_amd.num_states_intrinsics(**oi) + (2 if oi.get("do_optimize_calobject_warp", True) and oi.get("calobject_warp") is not None else 0)
    ncore = mrcal_amd.num_states_intrinsics(**oi) - 2*nk
    covered = np.zeros((Ny, Nx), bool); W = 0
    for o in range(oi["observations_board"].shape[0]):
        rows = J[200*o:200*(o+1)]
        idx  = rows.indices[(rows.data != 0) & (rows.indices >= ncore) & (rows.indices < ncore + 2*nk)]
        if len(idx) == 0: continue
        k = (np.unique(idx) - ncore)//2
        x, y = k %% Nx, k // Nx
        covered[y.min():y.max()+1, x.min():x.max()+1] = True
        W = max(W, int(x.max() - x.min() + 1))
    n1 = 2*int(covered.sum()) + (Nc - 2*nk)
    cnt = covered.sum(axis=0); ws = W - 1
    best = None; bestcost = -(-n1//64)
    for s0 in range(0, Nx - ws):
        ar = 2*int(cnt[:s0].sum()); br = 2*int(cnt[s0+ws:].sum()); sr = n1 - ar - br
        a, b, s = -(-ar//64), -(-br//64), -(-sr//64)
        if a < 1 or b < 1 or sr < 1: continue
        cost = max(a, b) + 1 + s
        fits = nd["rounds"] > 0 and a <= nd["rounds"] and b <= nd["rounds"] and sr <= nd["ns_max"] and 64*max(a, b) <= 1024
        if fits and cost < bestcost: bestcost = cost; best = (64*a, 64*b, sr)
    return dict(active=int(best is not None), nA=best[0] if best else 0, nB=best[1] if best else 0, nS=best[2] if best else n1)
out = []
for rep in range(2):
    with Problem(**copy_inputs(oi)) as p:
        s = p.solve()
        nd = p.dissection()
        out.append(dict(N=s["Niterations"], Nout=s["Noutliers_board"], rms=s["rms_reproj_error__pixels"], b=p.b_packed().tolist(), nd=nd,
                        restated=restated_plan(p, nd) if rep == 0 else None))
print("RESULT " + json.dumps(out))
''' % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))),)
    res = {}
    for tag, env in (("nd", {}), ("tail", {"TEST_HOOKS": "lchol_likely_panels=1"}), ("unfit", {"TEST_HOOKS": "nd_rounds=1"}), ("off", {"MRCAL_AMD_NO_ND": "1"})):
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=800)
        assert r.returncode == 0, r.stderr[-2000:]
        res[tag] = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    nd, nd2, tail, unfit, off = res["nd"][0], res["nd"][1], res["tail"][0], res["unfit"][0], res["off"][0]
    assert nd["nd"]["rounds"] >= 1 and nd["nd"]["active"] == 1 and nd["nd"]["nA"] >= 64 and nd["nd"]["nB"] >= 64 and nd["nd"]["nS"] > 0, nd["nd"]
    assert off["nd"]["rounds"] == 0 and unfit["nd"]["rounds"] == 1 and unfit["nd"]["active"] == 0
    # the device's plan at the final point = the planner restated on the host from that point's Jacobian
    for arm in (nd, unfit):
        assert {k: arm["nd"][k] for k in ("active", "nA", "nB", "nS")} == arm["restated"], (arm["nd"], arm["restated"])
    same = lambda a, b: (a["N"], a["Nout"], a["rms"]) == (b["N"], b["Nout"], b["rms"]) and a["b"] == b["b"]
    assert same(nd, nd2) and same(nd, tail)
    assert same(unfit, off)
    assert nd["Nout"] == off["Nout"] and abs(nd["rms"] - off["rms"]) < 1e-8*off["rms"]
    assert np.abs(np.array(nd["b"]) - np.array(off["b"])).max() < 1e-4


def test_factorization_launches_and_tail_kernel_give_the_same_bits(amd):
    """The splined models' compacted camera block (cholesky_large.hip LcholCompact): the size of the matrix that is
    factored follows the boards, the host provides the launches of the size the solve's first point has, and whatever a
    later point needs beyond those is done by ONE kernel with barriers over its workgroups where the launch boundaries
    would be (lchol_tail_kernel). Which of the two ways a panel is done must not show: configuration 2 reduced to 200
    frames solved as it is, with all but the first two panels left to the tail kernel (the test hook lchol_likely_panels = 2), and
    without the compaction at all (MRCAL_AMD_NO_SPL_COMPACT=1: the 1206-variable matrix, 554 pivots of which are the
    uncovered control points' own 2 x 2 blocks) - the first two to the last bit, the third to what another order of the
    pivots leaves"""
    import os, subprocess, sys, json
    code = r'''
import sys, os, json, numpy as np
sys.path.insert(0, %r)
import mrcal_amd
for _kv in os.environ.get("TEST_HOOKS", "").split(","):          # (the test's own variable: hooks of the library's test API)
    if _kv: mrcal_amd.set_test_hook(_kv.split("=")[0], int(_kv.split("=")[1]))
from mrcal_amd.synthetic import make_calibration_problem, copy_inputs, CONFIG2_LENSMODEL
from mrcal_amd.resident import Problem
oi, _ = make_calibration_problem(mrcal_amd._api, Ncameras=1, Nframes=200, object_width_n=10, object_height_n=10,
                                 lensmodel=CONFIG2_LENSMODEL, seed=4, do_optimize_intrinsics_core=False)
with Problem(**copy_inputs(oi)) as p:
    s = p.solve()
    print("RESULT " + json.dumps(dict(N=s["Niterations"], Nout=s["Noutliers_board"], rms=s["rms_reproj_error__pixels"], b=p.b_packed().tolist())))
''' % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))),)
    res = {}
    for tag, env in (("launches", {}), ("tail", {"TEST_HOOKS": "lchol_likely_panels=2"}), ("whole", {"MRCAL_AMD_NO_SPL_COMPACT": "1"})):
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=800)
        assert r.returncode == 0, r.stderr[-2000:]
        res[tag] = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    a, b, c = res["launches"], res["tail"], res["whole"]
    assert (a["N"], a["Nout"], a["rms"]) == (b["N"], b["Nout"], b["rms"]) and a["b"] == b["b"]
    assert a["Nout"] == c["Nout"] and abs(a["rms"] - c["rms"]) < 1e-8*c["rms"]
    assert np.abs(np.array(a["b"]) - np.array(c["b"])).max() < 1e-4
