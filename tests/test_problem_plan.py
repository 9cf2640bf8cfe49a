"""plan_problem() (csrc/problem_plan.cpp) - the host function that decides, before anything touches the device, which
observations a shard owns, the measurement layout local to it, every observation's record with its CSR offsets, Nnz,
the board kernel's LDS size and the elimination partition - checked on the CPU through its dev export
mrcal_amd_debug_plan_problem(): no GPU needed.

The inputs are marshalled the way resident.Problem marshals them (_api._ingest, _api._common_args). The expected values
come from the reference's own code (oracle/_ref, bound as in test_layout.py) or from arithmetic written out here; never
from a second call into the library under test.

One known difference from the reference is AVOIDED here, not tested: for a triangulated pair the library counts the two
cameras' extrinsics columns only (6 + 6 at most: what its kernel writes), the reference's _mrcal_num_j_nonzero() adds
the intrinsics columns per camera as well (mrcal.c:819-843). With the intrinsics locked - the only setting either
accepts triangulated points in - the two agree, and every Nnz comparison below that has triangulated points locks them.

One GPU test at the end ties the plan to the object mrcal_amd_problem_create_sharded() builds from it."""
import ctypes as C
import numpy as np
import pytest

from mrcal_amd._cabi import Lensmodel, ProblemSelections, observation_board_dtype, _ptr

SCALARS = ("Nstate", "Nmeas", "Nmeas_boards", "Nmeas_points", "Nmeas_triangulated", "Nmeas_regularization",
           "i_meas_boards", "i_meas_points", "i_meas_triangulated", "i_meas_regularization",
           "i_state_intrinsics", "i_state_extrinsics", "i_state_frames", "i_state_points", "i_state_warp",
           "Nstate_intrinsics", "Nstate_extrinsics", "Nstate_frames", "Nstate_points", "Nstate_warp",
           "Nintr_state", "Nintr_per_row", "Nreg_percamera", "has_unity_cam01",
           "tri_o0", "tri_o1", "Nnz", "innz_reg", "lds_bytes", "board_alg_bytes", "is_leader",
           "nd_Nstate", "Nwarp", "nd_i_state_warp", "Nc", "NE", "Nfb", "Npb", "NEb", "S_split", "S_shift", "E_state0", "elim_extrinsics",
           "frame_lo", "frame_hi", "point_lo", "point_hi",
           "D_Nstate", "D_Nmeas", "D_Nobs_board", "D_Nobs_point", "D_Npairs_tri", "D_W", "D_H", "D_elim_extrinsics",
           "D_do_apply_regularization", "D_has_unity_cam01", "D_i_meas_regularization", "D_i_nnz_regularization")
STATE_LAYOUT = ("Nstate", "i_state_intrinsics", "i_state_extrinsics", "i_state_frames", "i_state_points", "i_state_warp",
                "Nstate_intrinsics", "Nstate_extrinsics", "Nstate_frames", "Nstate_points", "Nstate_warp")
BMETA = ("icam_intrinsics", "icam_extrinsics", "iframe", "nnz_per_row", "i_state_intrinsics", "i_state_extrinsics",
         "i_state_frame", "i_meas0", "i_nnz0")
PMETA = ("icam_intrinsics", "icam_extrinsics", "i_point", "nnz_per_row", "i_state_intrinsics", "i_state_extrinsics",
         "i_state_point", "i_meas0", "i_nnz0")
TMETA = ("i0", "i1", "icam_extrinsics0", "icam_extrinsics1", "i_state_extrinsics0", "i_state_extrinsics1", "i_meas", "i_nnz0")
WHOLE = dict(frames=(0, -1), points=(0, -1), tripoints=(0, -1), leader=True)
SPLINED = "LENSMODEL_SPLINED_STEREOGRAPHIC_order=3_Nx=4_Ny=3_fov_x_deg=100"


def export(amd):
    f = amd._lib.lib.mrcal_amd_debug_plan_problem
    vp = C.c_void_p
    f.restype  = C.c_int
    f.argtypes = [vp]*5 + [C.c_int]*5 + [vp, vp, C.c_int, C.c_int, vp, C.c_int, vp, vp,
                                          C.POINTER(Lensmodel), vp, ProblemSelections, C.c_double, C.c_int, C.c_int] + \
                 [C.c_int]*6 + [C.c_bool] + [C.c_int, vp, C.c_int, C.c_char_p, C.c_int]
    return f


def records(flat, names):
    return [dict(zip(names, (int(v) for v in flat[i:i + len(names)]))) for i in range(0, len(flat), len(names))]


def plan_args(amd, args, frames=(0, -1), points=(0, -1), tripoints=(0, -1), leader=True, elimination=0):
    """the plan of the create_sharded() arguments args[:24] as a dict, or the refusal's text"""
    f = export(amd)
    out = np.zeros(1 << 14, dtype=np.int64)
    err = C.create_string_buffer(1024)
    tail = [*frames, *points, *tripoints, leader, elimination]
    n = f(*args, *tail, _ptr(out), 3, err, len(err))
    if n < 0: return err.value.decode()
    assert n > 3 and not out.any()                                         # (too small a buffer: nothing is written)
    n = f(*args, *tail, _ptr(out), len(out), err, len(err))
    assert len(SCALARS) < n <= len(out)
    P = dict(zip(SCALARS, (int(v) for v in out[:len(SCALARS)])))
    at = len(SCALARS)
    for name, fields in (("board_sel", None), ("point_sel", None), ("bmeta", BMETA), ("pmeta", PMETA), ("tmeta", TMETA)):
        cnt = int(out[at])                                                 # [count | entries], list after list
        flat = out[at + 1:at + 1 + cnt]
        P[name] = [int(v) for v in flat] if fields is None else records(flat, fields)
        at += 1 + cnt
    assert at == n
    return P


def ingest(amd, oi):
    """_api._ingest(), with the triangulated observations' records filled without their vectors: those come from
    mrcal_unproject(), which needs the GPU, and the plan reads none"""
    oi = dict(oi)
    obs_tri = oi.pop("observations_point_triangulated", None)
    idx_tri = oi.pop("indices_point_triangulated_camintrinsics_camextrinsics", None)
    p = amd._api._ingest(oi, callback=False)
    if idx_tri is not None:
        p.c_tri = amd._api._fill_triangulated(obs_tri, idx_tri, None, None)
        p.Nobservations_tri = len(idx_tri)
    return p


def plan(amd, p, **kw):
    a = amd._api._common_args(p)
    # common args: ..., lensmodel, imagersizes, sel, problem_constants, spacing, W, H, verbose
    return plan_args(amd, [*a[:18], a[18], a[19], a[20], a[22], a[23], a[24]], **kw)


def case_A(lensmodel="LENSMODEL_OPENCV4", triangulated=False, **flags):
    """2 cameras, cam0 at the reference; 3 frames of a 3x2 board seen by both; 3 discrete points, the last one fixed,
    their 4 observations not sorted by point; everything optimized, regularization on.
    triangulated: + a set of 3 observations and a set of 2"""
    rng = np.random.RandomState(0)
    Nintrinsics = {"LENSMODEL_OPENCV4": 8, SPLINED: 4 + 2*4*3}[lensmodel]
    idx_board = np.array([(f, c, c - 1) for f in range(3) for c in range(2)], dtype=np.int32)
    oi = dict(lensmodel=lensmodel, intrinsics=rng.rand(2, Nintrinsics), imagersizes=np.array(((640, 480),)*2, dtype=np.int32),
              rt_cam_ref=rng.rand(1, 6), rt_ref_frame=rng.rand(3, 6), points=rng.rand(3, 3), Npoints_fixed=1,
              observations_board=rng.rand(len(idx_board), 2, 3, 3), indices_frame_camintrinsics_camextrinsics=idx_board,
              observations_point=rng.rand(4, 3),
              indices_point_camintrinsics_camextrinsics=np.array(((0, 0, -1), (1, 1, 0), (0, 1, 0), (2, 0, -1)), dtype=np.int32),
              calobject_warp=np.array((1e-3, 2e-3)), calibration_object_spacing=0.1,
              do_optimize_intrinsics_core=True, do_optimize_intrinsics_distortions=True, do_optimize_extrinsics=True,
              do_optimize_frames=True, do_optimize_calobject_warp=True, do_apply_regularization=True)
    if triangulated:
        oi["observations_point_triangulated"] = rng.rand(5, 3) + 1.
        oi["indices_point_triangulated_camintrinsics_camextrinsics"] = \
            np.array(((0, 0, -1), (0, 1, 0), (0, 1, 0), (1, 1, 0), (1, 0, -1)), dtype=np.int32)
    oi.update(flags)
    return oi


def ref_counts(ref_api, p):
    """(Nstate, Nmeas, Nnz) of the whole problem, by the reference"""
    lm  = C.byref(p.lensmodel)
    tri = (_ptr(p.c_tri), p.Nobservations_tri) if p.Nobservations_tri else (None, 0)
    dims = (p.Ncameras_intrinsics, p.Ncameras_extrinsics, p.Nframes, p.Npoints, p.Npoints_fixed)
    r = ref_api.clib
    return (r.mrcal_num_states(*dims, p.Nobservations_board, p.sel, lm),
            r.mrcal_num_measurements(p.Nobservations_board, p.Nobservations_point, *tri, p.width_n, p.height_n, *dims, p.sel, lm),
            r._mrcal_num_j_nonzero(p.Nobservations_board, p.Nobservations_point, *tri, p.width_n, p.height_n, *dims,
                                   _ptr(p.c_board), _ptr(p.c_point), p.sel, lm))


def check_offsets(P, rows_per_board):
    """each record's rows and CSR entries begin where the one before ended"""
    imeas, innz = 0, 0
    for recs, rows in ((P["bmeta"], rows_per_board), (P["pmeta"], 2)):
        for m in recs:
            assert (m["i_meas0"], m["i_nnz0"]) == (imeas, innz)
            imeas += rows; innz += rows*m["nnz_per_row"]
    for m in P["tmeta"]:
        assert (m["i_meas"], m["i_nnz0"]) == (imeas, innz)
        imeas += 1; innz += 6*(m["i_state_extrinsics0"] >= 0) + 6*(m["i_state_extrinsics1"] >= 0)
    assert (imeas, innz) == (P["i_meas_regularization"], P["innz_reg"]) == (P["D_i_meas_regularization"], P["D_i_nnz_regularization"])


def test_case_A_matches_reference(amd, ref_api):
    p = ingest(amd, case_A())
    P = plan(amd, p)
    r, lm = ref_api.clib, C.byref(p.lensmodel)
    Nob, Nop, W, H = 6, 4, 3, 2
    state = (2, 1, 3, 3, 1, Nob, p.sel, lm)
    Nstate, Nmeas, Nnz = ref_counts(ref_api, p)
    assert (P["Nstate"], P["Nmeas"], P["Nnz"]) == (Nstate, Nmeas, Nnz) == (P["D_Nstate"], P["D_Nmeas"], Nnz)
    assert P["i_meas_boards"] == r.mrcal_measurement_index_boards(0, Nob, Nop, W, H)
    assert P["i_meas_points"] == r.mrcal_measurement_index_points(0, Nob, Nop, W, H)
    assert P["i_meas_regularization"] == r.mrcal_measurement_index_regularization(None, 0, W, H, 2, 1, 3, 3, 1, Nob, Nop, p.sel, lm)
    assert P["i_meas_triangulated"] == P["i_meas_regularization"] and P["tmeta"] == [] and (P["tri_o0"], P["tri_o1"]) == (0, 0)
    assert P["board_sel"] == list(range(Nob)) and P["point_sel"] == list(range(Nop))
    # OPENCV4 with its core: 2 of the 4 core columns + 4 distortions in a row; the camera's pose unless it is the
    # reference; the frame's pose and the warp (boards), the point unless it is fixed (points)
    for j, m in enumerate(P["bmeta"]):
        f, ci, ce = (int(p.c_board[k][j]) for k in ("iframe", "icam_intrinsics", "icam_extrinsics"))
        assert (m["iframe"], m["icam_intrinsics"], m["icam_extrinsics"]) == (f, ci, ce)
        assert m["i_meas0"] == r.mrcal_measurement_index_boards(j, Nob, Nop, W, H)
        assert m["nnz_per_row"] == 6 + (6 if ce >= 0 else 0) + 6 + 2
        assert m["i_state_intrinsics"] == r.mrcal_state_index_intrinsics(ci, *state)
        assert m["i_state_extrinsics"] == (r.mrcal_state_index_extrinsics(ce, *state) if ce >= 0 else -1)
        assert m["i_state_frame"]      == r.mrcal_state_index_frames(f, *state)
    for j, m in enumerate(P["pmeta"]):
        ip, ci, ce = (int(p.c_point[k][j]) for k in ("i_point", "icam_intrinsics", "icam_extrinsics"))
        assert (m["i_point"], m["icam_intrinsics"], m["icam_extrinsics"]) == (ip, ci, ce)
        assert m["i_meas0"] == r.mrcal_measurement_index_points(j, Nob, Nop, W, H)
        assert m["nnz_per_row"] == 6 + (6 if ce >= 0 else 0) + (3 if ip < 2 else 0)
        assert m["i_state_intrinsics"] == r.mrcal_state_index_intrinsics(ci, *state)
        assert m["i_state_extrinsics"] == (r.mrcal_state_index_extrinsics(ce, *state) if ce >= 0 else -1)
        assert m["i_state_point"]      == (r.mrcal_state_index_points(ip, *state) if ip < 2 else -1)
    assert P["pmeta"][3]["i_state_point"] == -1 and P["bmeta"][0]["i_state_extrinsics"] == -1
    check_offsets(P, 2*W*H)
    # the regularization rows: one nonzero each, 4 distortions + 2 of the core per camera
    assert P["Nnz"] - P["innz_reg"] == 2*(4 + 2) and P["Nmeas_regularization"] == 2*(4 + 2)
    # the tile (64 rows x (4*ceil((4 + 4 + 15)/4) | 1) doubles) + the staged observation in whole 64-element chunks
    # + the joint pose record (84) + 4
    assert P["lds_bytes"] == 8*(64*25 + 64 + 84 + 4)
    # per corner 24 bytes read and 16 of x written, 8 per nonzero of the board rows
    assert P["board_alg_bytes"] == Nob*W*H*(24 + 16) + 8*sum(2*W*H*m["nnz_per_row"] for m in P["bmeta"])
    assert (P["is_leader"], P["D_do_apply_regularization"], P["has_unity_cam01"]) == (1, 1, 0)


def test_case_A_triangulated(amd, ref_api):
    """intrinsics locked; a set of 3 observations, then a set of 2: 3 + 1 pairs in (i0, i1) order"""
    p = ingest(amd, case_A(triangulated=True, do_optimize_intrinsics_core=False, do_optimize_intrinsics_distortions=False))
    P = plan(amd, p)
    Nob, Nop, W, H = 6, 4, 3, 2
    assert (P["Nstate"], P["Nmeas"], P["Nnz"]) == ref_counts(ref_api, p)
    assert [(m["i0"], m["i1"]) for m in P["tmeta"]] == [(0, 1), (0, 2), (1, 2), (3, 4)]
    first = [ref_api.clib.mrcal_measurement_index_points_triangulated(ip, Nob, Nop, _ptr(p.c_tri), 5, W, H) for ip in range(2)]
    assert [m["i_meas"] for m in P["tmeta"]] == [first[0], first[0] + 1, first[0] + 2, first[1]]
    assert P["i_meas_triangulated"] == first[0] and P["Nmeas_triangulated"] == 4 == P["D_Npairs_tri"]
    state = (2, 1, 3, 3, 1, Nob, p.sel, C.byref(p.lensmodel))
    ie = ref_api.clib.mrcal_state_index_extrinsics(0, *state)
    ce = [int(v) for v in p.c_tri["icam_extrinsics"]]
    for m in P["tmeta"]:
        assert (m["icam_extrinsics0"], m["icam_extrinsics1"]) == (ce[m["i0"]], ce[m["i1"]])
        assert (m["i_state_extrinsics0"], m["i_state_extrinsics1"]) == tuple(ie if c >= 0 else -1 for c in (ce[m["i0"]], ce[m["i1"]]))
    assert (P["tri_o0"], P["tri_o1"]) == (0, 5)
    check_offsets(P, 2*W*H)
    assert P["Nnz"] == P["innz_reg"] and P["Nmeas_regularization"] == 0      # (nothing to regularize)


def test_case_A_splined(amd, ref_api):
    p = ingest(amd, case_A(lensmodel=SPLINED))
    P = plan(amd, p)
    assert (P["Nstate"], P["Nmeas"], P["Nnz"]) == ref_counts(ref_api, p)
    assert P["lds_bytes"] == 0
    check_offsets(P, 12)
    # the knot rows have 2 nonzeros each, the 2 core rows of a camera 1
    assert P["Nnz"] - P["innz_reg"] == 2*(2*24 + 2) and P["Nmeas_regularization"] == 2*(24 + 2)


SHARDINGS = {
    "2": [dict(frames=(0, 2), points=(0, 2), tripoints=(0, 1), leader=True),
          dict(frames=(2, 3), points=(2, 3), tripoints=(1, 2), leader=False)],
    "3": [dict(frames=(0, 1), points=(0, 1), tripoints=(0, 1), leader=False),
          dict(frames=(1, 2), points=(1, 2), tripoints=(1, 2), leader=True),
          dict(frames=(2, 3), points=(2, 3), tripoints=(2, 2), leader=False)],
    # an empty frame range is a shard all the same; the ranges that are not given: everything with the leader
    "empty+leader": [dict(frames=(0, 0), points=(0, -1), tripoints=(0, -1), leader=False),
                     dict(frames=(0, 3), points=(0, -1), tripoints=(0, -1), leader=True)],
}

@pytest.mark.parametrize("sharding", sorted(SHARDINGS))
@pytest.mark.parametrize("triangulated", (False, True))
def test_shards_of_case_A(amd, ref_api, sharding, triangulated):
    flags = dict(do_apply_regularization_unity_cam01=True)
    if triangulated: flags.update(triangulated=True, do_optimize_intrinsics_core=False, do_optimize_intrinsics_distortions=False)
    p = ingest(amd, case_A(**flags))
    whole  = plan(amd, p)
    shards = [plan(amd, p, **s) for s in SHARDINGS[sharding]]
    assert (whole["Nstate"], whole["Nmeas"], whole["Nnz"]) == ref_counts(ref_api, p)
    assert whole["has_unity_cam01"] == 1 and whole["Nmeas_regularization"] == (1 if triangulated else 13)
    # a partition of the observations of each kind
    assert sorted(i for P in shards for i in P["board_sel"]) == list(range(6))
    assert sorted(i for P in shards for i in P["point_sel"]) == list(range(4))
    for s, P in zip(SHARDINGS[sharding], shards):
        assert P["board_sel"] == [i for i in range(6) if s["frames"][0] <= p.c_board["iframe"][i] < s["frames"][1]]
        pts = s["points"] if s["points"][1] >= 0 else ((0, 3) if s["leader"] else (0, 0))
        assert P["point_sel"] == [i for i in range(4) if pts[0] <= p.c_point["i_point"][i] < pts[1]]
    tri = sorted((P["tri_o0"], P["tri_o1"]) for P in shards if P["tri_o1"] > P["tri_o0"])
    if triangulated:
        assert tri[0][0] == 0 and tri[-1][1] == 5 and all(a[1] == b[0] for a, b in zip(tri, tri[1:]))
        assert all(t in ((0, 3), (3, 5), (0, 5)) for t in tri)                      # (whole point sets)
    else:
        assert tri == []
    for s, P in zip(SHARDINGS[sharding], shards):
        lead = 1 if s["leader"] else 0
        assert (P["is_leader"], P["has_unity_cam01"], P["D_has_unity_cam01"], P["D_do_apply_regularization"]) == (lead,)*4
        assert P["Nmeas_regularization"] == (whole["Nmeas_regularization"] if lead else 0)
        assert P["Nnz"] - P["innz_reg"] == ((whole["Nnz"] - whole["innz_reg"]) if lead else 0)
        assert {k: P[k] for k in STATE_LAYOUT} == {k: whole[k] for k in STATE_LAYOUT}
        check_offsets(P, 12)
        # the blocks the shard owns: 3 frame blocks, then the 2 variable points' (the clamps of owned_blocks())
        assert (P["Nfb"], P["Npb"], P["elim_extrinsics"]) == (3, 2, 0)
        pts = s["points"] if s["points"][1] >= 0 else ((0, 3) if lead else (0, 0))
        assert (P["frame_lo"], P["frame_hi"]) == (s["frames"][0], min(s["frames"][1], 3))
        assert (P["point_lo"], P["point_hi"]) == (3 + min(pts[0], 2), 3 + min(pts[1], 2))
    assert (whole["frame_lo"], whole["frame_hi"], whole["point_lo"], whole["point_hi"]) == (0, 3, 3, 5)
    assert sum(P["Nmeas"] for P in shards) == whole["Nmeas"]
    assert sum(P["Nnz"]   for P in shards) == whole["Nnz"]
    assert sum(P["D_Npairs_tri"] for P in shards) == whole["D_Npairs_tri"] == (4 if triangulated else 0)


def moving_camera(Nce=5, lensmodel="LENSMODEL_OPENCV4", **extra):
    """one camera that moves: Nce rt_cam_ref, one frame of a 3x2 board"""
    rng = np.random.RandomState(1)
    Nintrinsics = {"LENSMODEL_OPENCV4": 8, SPLINED: 4 + 2*4*3}[lensmodel]
    oi = dict(lensmodel=lensmodel, intrinsics=rng.rand(1, Nintrinsics), imagersizes=np.array(((640, 480),), dtype=np.int32),
              rt_cam_ref=rng.rand(Nce, 6), rt_ref_frame=rng.rand(1, 6),
              observations_board=rng.rand(Nce, 2, 3, 3),
              indices_frame_camintrinsics_camextrinsics=np.array([(0, 0, e) for e in range(Nce)], dtype=np.int32),
              calobject_warp=np.array((1e-3, 2e-3)), calibration_object_spacing=0.1,
              do_optimize_intrinsics_core=True, do_optimize_intrinsics_distortions=True, do_optimize_extrinsics=True,
              do_optimize_frames=True, do_optimize_calobject_warp=True, do_apply_regularization=True)
    oi.update(extra)
    return oi


def partition_of(P):
    return {k: P[k] for k in ("Nc", "NE", "Nfb", "Npb", "NEb", "S_split", "S_shift", "E_state0", "elim_extrinsics")}

def frames_partition(Nintr, Nextr, Nframes, Npoints_variable, Nwarp):
    """state [intrinsics | extrinsics | frames | points | warp]: the frames and points go, the warp closes up"""
    NE = 6*Nframes + 3*Npoints_variable
    return dict(Nc=Nintr + Nextr + Nwarp, NE=NE, Nfb=Nframes, Npb=Npoints_variable, NEb=Nframes + Npoints_variable,
                S_split=Nintr + Nextr, S_shift=NE, E_state0=Nintr + Nextr, elim_extrinsics=0)

def extrinsics_partition(Nintr, Nextr, Nframes, Nwarp):
    """... the extrinsics go, the frames and the warp close up"""
    return dict(Nc=Nintr + 6*Nframes + Nwarp, NE=Nextr, Nfb=Nextr//6, Npb=0, NEb=Nextr//6,
                S_split=Nintr, S_shift=Nextr, E_state0=Nintr, elim_extrinsics=1)


def test_elimination_moving_camera(amd):
    p = ingest(amd, moving_camera(5))
    fr, ex = frames_partition(8, 30, 1, 0, 2), extrinsics_partition(8, 30, 1, 2)
    assert partition_of(plan(amd, p, elimination=0)) == ex            # 5 >= 4 cameras, 30 extrinsics > 6 frame variables
    assert partition_of(plan(amd, p, elimination=1)) == fr
    assert partition_of(plan(amd, p, elimination=2)) == ex
    for policy in (0, 1, 2):
        P = plan(amd, p, elimination=policy)
        assert P["D_elim_extrinsics"] == P["elim_extrinsics"] and P["Nc"] + P["NE"] == P["Nstate"] == P["nd_Nstate"] == 46
        assert (P["Nwarp"], P["nd_i_state_warp"]) == (2, 44)
        assert (P["frame_lo"], P["frame_hi"], P["point_lo"], P["point_hi"]) == (0, P["Nfb"], P["Nfb"], P["Nfb"])
    # too few cameras for the library to choose the extrinsics by itself; they can still be asked for
    p3 = ingest(amd, moving_camera(3))
    assert partition_of(plan(amd, p3, elimination=0)) == frames_partition(8, 18, 1, 0, 2)
    assert partition_of(plan(amd, p3, elimination=2)) == extrinsics_partition(8, 18, 1, 2)


ONE_POINT = dict(points=np.ones((1, 3)), observations_point=np.ones((1, 3)),
                 indices_point_camintrinsics_camextrinsics=np.array(((0, 0, 0),), dtype=np.int32))
ONE_SET   = dict(observations_point_triangulated=np.ones((2, 3)),
                 indices_point_triangulated_camintrinsics_camextrinsics=np.array(((0, 0, 0), (0, 0, 1)), dtype=np.int32))

@pytest.mark.parametrize("what", ("point", "triangulated", "unity_cam01", "splined", "shard"))
def test_elimination_frames_only(amd, what):
    """whatever the policy: a row that touches two cameras' poses or none of a frame's, the splined models' assembly
    and the sharding know the frames partition only"""
    extra = dict(point=ONE_POINT, triangulated=ONE_SET, unity_cam01=dict(do_apply_regularization_unity_cam01=True),
                 splined=dict(lensmodel=SPLINED), shard={})[what]
    p = ingest(amd, moving_camera(5, **extra))
    Nintr = 28 if what == "splined" else 8
    expected = frames_partition(Nintr, 30, 1, 1 if what == "point" else 0, 2)
    for policy in (0, 1, 2):
        P = plan(amd, p, elimination=policy, **(dict(frames=(0, 1)) if what == "shard" else {}))
        assert partition_of(P) == expected, policy


def bare_args(Nobs, W, H, lm, sel):
    """create_sharded()'s arguments from counts alone: one camera with extrinsics, a frame per board observation, every
    pool and seed NULL - the plan reads none of them"""
    c_board = np.zeros((Nobs,), dtype=observation_board_dtype)
    c_board["iframe"] = np.arange(Nobs)
    imagersizes = np.array((640, 480), dtype=np.int32)
    return c_board, imagersizes, [None]*5 + [1, 1, Nobs, 0, 0, _ptr(c_board), None, Nobs, 0, None, 0, None, None,
                                             C.byref(lm), _ptr(imagersizes), sel, 0.1, W, H]


def test_refusals(amd):
    """the parent's messages, from the plan: no GPU call was made by then"""
    lm  = amd._lib.lensmodel("LENSMODEL_OPENCV4")
    sel = ProblemSelections.make(**{n: True for n in ProblemSelections.NAMES[:6]})
    *keep, args = bare_args(1, 0, 2, lm, sel)
    assert plan_args(amd, args) == "board observations given, but the board has no corners"
    # 100x100 corners, 2 rows each of 6 intrinsics + 6 + 6 + 2 columns: 400000 nonzeros an observation, + 6 regularization rows
    Nobs = (2**31 - 1)//400000 + 1
    *keep, args = bare_args(Nobs, 100, 100, lm, sel)
    assert plan_args(amd, args) == \
        f"Jacobian has {Nobs*400000 + 6} nonzeros: more than int32 CSR offsets can address. Shard the problem"
    # (the checks in their order: this board would not fit the LDS either, which a shard with few enough nonzeros is told)
    assert plan_args(amd, args, frames=(0, 10)) == "the board has 10000 corners and the lens model 4 distortion parameters: the LDS tile would not fit"
    # 8*(64*25 + 3*80*80 + 84 + 4) bytes = 163.2 KB > 160 KB
    *keep, args = bare_args(1, 80, 80, lm, sel)
    assert plan_args(amd, args) == "the board has 6400 corners and the lens model 4 distortion parameters: the LDS tile would not fit"


@pytest.mark.gpu
def test_created_problem_is_the_plan(amd):
    """the object create() builds holds what the plan said: case A whole and as two frame shards"""
    from mrcal_amd.resident import Problem
    oi = case_A()
    lib = amd._lib.lib
    lib.mrcal_amd_problem_shard_info.restype  = C.c_int
    lib.mrcal_amd_problem_shard_info.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_int]
    for s in (WHOLE, dict(frames=(0, 2), points=(0, -1), tripoints=(0, -1), leader=True),
                     dict(frames=(2, 3), points=(0, -1), tripoints=(0, -1), leader=False)):
        P = plan(amd, ingest(amd, oi), **s)
        with Problem(_shard=s["frames"], _leader=s["leader"], _shard_points=s["points"], _shard_tripoints=s["tripoints"], **oi) as prob:
            assert (prob.Nstate, prob.Nmeas, prob.Nnz) == (P["Nstate"], P["Nmeas"], P["Nnz"])
            assert prob.jacobian_algorithmic_bytes() == P["board_alg_bytes"]
            assert prob.partition() == dict(S_split=P["S_split"], S_shift=P["S_shift"], E_state0=P["E_state0"], eliminates="frames")
            info = (C.c_int*12)()
            assert lib.mrcal_amd_problem_shard_info(prob.handle, info, 12) == 12
            assert list(info) == [P["nd_Nstate"], P["S_split"], P["NE"], P["Nc"], P["frame_lo"], P["frame_hi"], P["is_leader"],
                                  P["D_Nobs_board"]*P["D_W"]*P["D_H"], P["Nfb"], P["Npb"], P["point_lo"], P["point_hi"]]
            prob.evaluate()
            assert prob.J().indptr[P["Nmeas"]] == P["Nnz"]
