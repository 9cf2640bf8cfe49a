#!/usr/bin/env python3
"""Times projection uncertainty at the metric's problem (8 cameras x 1000 frames x 10x10 corners, OPENCV8, seed 0,
solved), for a 60x40 grid of the imager unprojected to 10 m, camera 3:

  (a) the reference's flow composed from the existing primitives: project(), drt_cross_reprojection__dbpacked(),
      one solve_xt_JtJ_bt() of the 2N right-hand sides, then _A_Jt_J_At__2() per point (each call uploads J).
      Too slow to run for the whole grid: --ref-points of them are timed and the per-point cost is scaled to the grid
  (b) the one-shot projection_uncertainty()
  (c) ProjectionUncertainty.evaluate() on a context made once
  (d) making that context: ProjectionUncertainty() - the problem, K, the factorization, C - then close()

(b), (c) and (d) alternate within one run, --trials times; min / median / max are printed, and one JSON line at the end.
Under rocprofv3 --kernel-trace --memory-copy-trace --stats (--no-ref) it shows the kernels and the copies of (b)/(c)."""
import argparse
import json
import os
import sys
import time
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=7)
    ap.add_argument("--ref-points", type=int, default=24)
    ap.add_argument("--no-ref", action="store_true")
    ap.add_argument("--grid", default="60x40", help="WxH points on the imager (100x100: 10^4 points)")
    args = ap.parse_args()
    import mrcal_amd as mrcal
    from mrcal_amd.synthetic import make_calibration_problem
    api = mrcal._api
    oi, _ = make_calibration_problem(api, Ncameras=8, Nframes=1000, lensmodel="LENSMODEL_OPENCV8",
                                     object_width_n=10, object_height_n=10, seed=0)
    t0 = time.perf_counter()
    mrcal.optimize(**oi)
    t_solve = time.perf_counter() - t0
    icam = 3
    model = mrcal.cameramodel(optimization_inputs=oi, icam_intrinsics=icam)
    W, H = model.imagersize()
    gw, gh = (int(n) for n in args.grid.split("x"))
    q = np.stack(np.meshgrid(np.linspace(0, W-1, gw), np.linspace(0, H-1, gh)), -1).reshape(-1, 2)
    p = mrcal.unproject(q, *model.intrinsics(), normalize=True) * 10.0
    out = dict(problem="8 cameras x 1000 frames x 10x10, OPENCV8, seed 0, solved", grid=args.grid, icam=icam,
               solve_s=t_solve)

    tb, tc, td = [], [], []
    u = mrcal.ProjectionUncertainty(model, observed_pixel_uncertainty=0.3)
    vbs, vcs = [], []
    for _ in range(args.trials):
        t0 = time.perf_counter(); vb = mrcal.projection_uncertainty(p, model, observed_pixel_uncertainty=0.3); tb.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); vc = u.evaluate(p);                                               tc.append(time.perf_counter() - t0)
        vbs.append(vb); vcs.append(vc)
        t0 = time.perf_counter(); ud = mrcal.ProjectionUncertainty(model, observed_pixel_uncertainty=0.3); td.append(time.perf_counter() - t0)
        ud.close()
    rel = lambda a, b: float(np.nanmax(np.abs(a - b)) / np.nanmax(np.abs(b)))  # (unproject() leaves NaN at a few imager corners)
    out["b_calls_identical"] = all(np.array_equal(v, vbs[0], equal_nan=True) for v in vbs)
    out["c_calls_identical"] = all(np.array_equal(v, vcs[0], equal_nan=True) for v in vcs)
    out["b_vs_c_max_rel_diff"] = max(rel(b, c) for b, c in zip(vbs, vcs))
    print(f"(b) calls identical {out['b_calls_identical']}, (c) calls identical {out['c_calls_identical']}, "
          f"(b) vs (c) max rel diff {out['b_vs_c_max_rel_diff']:.3g}")
    stat = lambda t: dict(min_ms=1e3*min(t), median_ms=1e3*float(np.median(t)), max_ms=1e3*max(t))
    out["b_one_shot"] = stat(tb)
    out["c_evaluate"] = stat(tc)
    out["d_create"] = stat(td)
    print(f"(b) one-shot projection_uncertainty(): {out['b_one_shot']}")
    print(f"(c) evaluate() on a reused context:    {out['c_evaluate']}")
    print(f"(d) ProjectionUncertainty():           {out['d_create']}")

    if not args.no_ref:
        n = args.ref_points
        t0 = time.perf_counter()
        b, x, J, F = mrcal.optimizer_callback(**oi)
        t_cb = time.perf_counter() - t0
        t0 = time.perf_counter()
        Nstate = J.shape[1]
        Nreg = api.num_measurements_regularization(**oi)
        K = mrcal.drt_cross_reprojection__dbpacked(icam_intrinsics=icam, **oi)
        api.pack_state(K, **oi)
        pp = p[:n]
        _, dq_dp, dq_di = mrcal.project(pp, oi["lensmodel"], oi["intrinsics"][icam], get_gradients=True)
        i0 = api.state_index_intrinsics(icam, **oi); Ni = api.num_intrinsics_optimization_params(**oi)
        skew = lambda v: np.array(((0, -v[2], v[1]), (v[2], 0, -v[0]), (-v[1], v[0], 0)))
        dq_db = np.zeros((n, 2, Nstate))
        dq_db[..., i0:i0+Ni] = dq_di[..., :Ni]
        for i in range(n):
            dq_db[i] += (dq_dp[i] @ skew(pp[i])) @ K[:3] - dq_dp[i] @ K[3:]
        api.unpack_state(dq_db, **oi)
        A = F.solve_xt_JtJ_bt(dq_db.reshape(-1, Nstate)).reshape(n, 2, Nstate)
        V = np.array([mrcal._A_Jt_J_At__2(A[i], J.indptr, J.indices, J.data, Nleading_rows_J=J.shape[0]-Nreg)
                      for i in range(n)]) * 0.3*0.3
        t_ref = time.perf_counter() - t0
        err = float(np.nanmax(np.abs(V - vc[:n])) / np.nanmax(np.abs(V)))
        out["a_reference_flow"] = dict(points_timed=n, optimizer_callback_s=t_cb, points_s=t_ref,
                                       per_point_ms=1e3*t_ref/n, grid_estimate_s=t_ref/n*len(p) + t_cb,
                                       max_rel_diff_vs_c=err)
        print(f"(a) reference flow: optimizer_callback {t_cb:.2f} s, {n} points {t_ref:.2f} s "
              f"-> the grid ~{out['a_reference_flow']['grid_estimate_s']:.1f} s; max rel diff vs (c) {err:.2e}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
