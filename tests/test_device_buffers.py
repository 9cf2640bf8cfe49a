"""Every device and pinned-host buffer of the library belongs to an owner (csrc/device_memory.hpp) that frees it when
its object is destroyed: mrcal_amd_device_buffers_live() is back where it was after one of each kind of object that
allocates differently has been made, used and destroyed."""
import ctypes as C
import gc
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _settled(live):
    """the count once it stands still. The synthetic inputs are made with optimizer_callback(), a drop-in entry point:
    its problems are torn down by a thread of the library's own a moment after the call returns (a few ms each)"""
    n, still = live(), 0
    for _ in range(200):
        time.sleep(0.05)
        m = live()
        still = still + 1 if m == n else 0
        n = m
        if still >= 10: return n
    raise AssertionError("the count of live buffers does not come to rest")


def test_destroyed_objects_leave_no_buffer_behind(amd):
    from mrcal_amd.resident import Problem
    from mrcal_amd.parallel import partition_frames
    from mrcal_amd.synthetic import make_calibration_problem, copy_inputs, CONFIG2_LENSMODEL
    from mrcal_amd import CHOLMOD_factorization
    from test_parallel_gpu import _problem, _sfm_with_everything

    live = amd._lib.lib.mrcal_amd_device_buffers_live
    live.restype, live.argtypes = C.c_long, []

    # all inputs first: making them goes through the drop-in entry points
    oi_boards  = _problem(amd._api)                                  # boards, OPENCV8
    oi_splined = make_calibration_problem(amd._api, Ncameras=1, Nframes=200, object_width_n=10, object_height_n=10,
                                          lensmodel=CONFIG2_LENSMODEL, seed=4, do_optimize_intrinsics_core=False)[0]
    oi_sfm     = _sfm_with_everything(amd._api)                      # boards, discrete points, triangulated pairs
    gc.collect()
    n0 = _settled(live)
    seen = []

    # boards: the solver prepared, a few steps
    with Problem(**copy_inputs(oi_boards)) as p:
        assert p.run_steps(3)[0] == 3
        J = p.J()
        seen.append(live())
    assert live() == n0

    # the splined model with one camera: the compaction's and the dissection's buffers
    with Problem(**copy_inputs(oi_splined)) as p:
        assert p.run_steps(3)[0] == 3
        seen.append(live())
    assert live() == n0

    # discrete points and triangulated pairs: the plan of the rows outside the Grams
    with Problem(**copy_inputs(oi_sfm)) as p:
        p.solve()
        seen.append(live())
    assert live() == n0

    # a frame-sharded pair
    ing = amd._api._ingest(dict(oi_boards), callback=False)
    fr = partition_frames(ing.c_board["iframe"].reshape(-1,1), ing.Nframes, 2)
    shards = [Problem(_shard=fr[r], _leader=(r == 0), **copy_inputs(oi_boards)) for r in range(2)]
    for ps in shards: ps.normal_equations()
    seen.append(live())
    for ps in shards: ps.close()
    del ing
    assert live() == n0

    # a factorization of a bare matrix; the second solve needs larger batch buffers than the first
    F = CHOLMOD_factorization(J)
    F.solve_xt_JtJ_bt(np.ones((1, J.shape[1])))
    seen.append(live())
    F.solve_xt_JtJ_bt(np.ones((5, J.shape[1])))
    assert live() == seen[-1]                   # (three buffers released, three allocated)
    F._L.mrcal_amd_factorization_destroy(F._h); F._h = None
    assert live() == n0

    # projection uncertainty, evaluated at two different N: the point buffers are allocated again
    m = amd.cameramodel(optimization_inputs=copy_inputs(oi_boards), icam_intrinsics=1)
    u = amd.ProjectionUncertainty(m, observed_pixel_uncertainty=1.0)
    assert live() == n0 + 3                     # (C, the intrinsics, the pose: the problem and the factorization it was made from are gone)
    rng = np.random.RandomState(0)
    for N in (4, 9):
        u.evaluate(np.column_stack((rng.uniform(-1, 1, (N,2)), np.full((N,), 4.))))
        assert live() == n0 + 5
    u.close()

    assert all(n > n0 for n in seen), (n0, seen)
    assert live() == n0
