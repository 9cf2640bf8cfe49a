#!/usr/bin/env python3
"""Times triangulate() (leecivera_mid2):

  (a) 10^5 pixel pairs of two cameras with observation-time noise, on a Triangulation context made once and reused
  (b) the same composed of the public pieces: unproject(get_gradients = True) of each camera's pixels, numpy pose
      arithmetic, triangulate_leecivera_mid2(get_gradients = True), dp/dq Var_q dp/dq^T in numpy
  (c) 256 pairs of neighbouring cameras with calibration-time noise at the metric's problem (8 cameras x 1000 frames,
      OPENCV8, seed 0, solved): the context's construction once (the problem, the factorization, sigma), then
      triangulate() on it

(a) and (b) alternate within one run, --trials times after one warm-up; a clock around each call (every call ends in
a synchronise); min / median / max in ms, and one JSON line at the end. Records, not gates."""
import argparse
import json
import os
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def pixel_pairs(mrcal, models, pairs, seed):
    """a seeded point 2-50 m in front of each pair's first camera, seen by both, with up to 0.5 px of noise"""
    rng = np.random.default_rng(seed)
    N = len(pairs)
    a, b = np.radians(rng.uniform(-12., 12., size=(2, N)))
    p0 = np.stack((np.tan(a), np.tan(b), np.ones(N)), -1)
    p0 *= (rng.uniform(2., 50., N)/np.linalg.norm(p0, axis=-1))[:, None]
    q = np.zeros((N, 2, 2))
    kinds = sorted(set(map(tuple, pairs)))
    pairs = np.asarray(pairs)
    for c0, c1 in kinds:
        sel = np.nonzero((pairs[:, 0] == c0) & (pairs[:, 1] == c1))[0]
        Rt10 = mrcal.compose_Rt(models[c1].Rt_cam_ref(), models[c0].Rt_ref_cam())
        q[sel, 0] = mrcal.project(p0[sel], *models[c0].intrinsics())
        q[sel, 1] = mrcal.project(mrcal.transform_point_Rt(Rt10, p0[sel]), *models[c1].intrinsics())
    return q + rng.uniform(-0.5, 0.5, size=q.shape)


def composed(mrcal, q, m0, m1, stdev, correlation):
    from mrcal_amd.triangulation import _compute_Var_q_triangulation
    v0,  dv0_dq,  _ = mrcal.unproject(q[:, 0], *m0.intrinsics(), get_gradients=True)
    vl1, dvl1_dq, _ = mrcal.unproject(q[:, 1], *m1.intrinsics(), get_gradients=True)
    rt01 = mrcal.compose_rt(m0.rt_cam_ref(), m1.rt_ref_cam())
    R01 = mrcal.R_from_r(rt01[:3])
    p, dp_dv0, dp_dv1, _ = mrcal.triangulate_leecivera_mid2(v0, vl1 @ R01.T, rt01[3:], get_gradients=True)
    dp_dq = np.concatenate((dp_dv0 @ dv0_dq, dp_dv1 @ R01 @ dvl1_dq), axis=-1)
    return p, dp_dq @ _compute_Var_q_triangulation(stdev, correlation) @ np.swapaxes(dp_dq, -1, -2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=7)
    ap.add_argument("--pairs", type=int, default=100000)
    ap.add_argument("--no-calibration", action="store_true")
    args = ap.parse_args()
    import mrcal_amd as mrcal
    from mrcal_amd.synthetic import make_calibration_problem
    if not mrcal.gpu_available():
        raise RuntimeError("no HIP device visible: nothing to measure")
    stat = lambda t: dict(min_ms=1e3*min(t), median_ms=1e3*float(np.median(t)), max_ms=1e3*max(t))
    out = {}

    # (a), (b): two cameras 0.3 m apart
    oi, _ = make_calibration_problem(mrcal._api, Ncameras=2, Nframes=6, seed=1)
    models = [mrcal.cameramodel(optimization_inputs=oi, icam_intrinsics=i) for i in range(2)]
    q = pixel_pairs(mrcal, models, [(0, 1)]*args.pairs, seed=0)
    ta, tb = [], []
    with mrcal.Triangulation(models) as t:
        for trial in range(-1, args.trials):          # (-1: the warm-up)
            t0 = time.perf_counter(); got = t.triangulate(q, q_observation_stdev=0.3, q_observation_stdev_correlation=0.5); dt = time.perf_counter() - t0
            if trial >= 0: ta.append(dt)
            t0 = time.perf_counter(); ref = composed(mrcal, q, models[0], models[1], 0.3, 0.5); dt = time.perf_counter() - t0
            if trial >= 0: tb.append(dt)
    scale = np.abs(ref[1]).max(axis=(-1, -2))
    ok = scale > 0
    out["observation_noise"] = dict(pairs=args.pairs, a_triangulate_reused_context=stat(ta), b_public_pieces=stat(tb),
                                    p_a_vs_b=float(np.abs(got[0] - ref[0]).max()/np.abs(ref[0]).max()),
                                    Var_a_vs_b=float((np.abs(got[1] - ref[1]).max(axis=(-1, -2))[ok]/scale[ok]).max()),
                                    pairs_without_a_point=int(np.count_nonzero(~ok)))
    print(f"observation-time noise, {args.pairs} pairs:")
    print(f"  (a) triangulate(), context reused: {out['observation_noise']['a_triangulate_reused_context']}")
    print(f"  (b) the public pieces composed:    {out['observation_noise']['b_public_pieces']}")
    print(f"      (a) against (b): p {out['observation_noise']['p_a_vs_b']:.3g}, Var_p_observation {out['observation_noise']['Var_a_vs_b']:.3g} "
          f"of the largest entry; {out['observation_noise']['pairs_without_a_point']} pairs without a point")

    if not args.no_calibration:
        # (c): the metric's problem
        oi, _ = make_calibration_problem(mrcal._api, Ncameras=8, Nframes=1000, seed=0)
        mrcal.optimize(**oi)
        models = [mrcal.cameramodel(optimization_inputs=oi, icam_intrinsics=i) for i in range(8)]
        pairs = [(i % 7, i % 7 + 1) for i in range(256)]
        q = pixel_pairs(mrcal, models, pairs, seed=1)
        pair_models = np.array([[models[a], models[b]] for a, b in pairs], dtype=object)
        t0 = time.perf_counter()
        t = mrcal.Triangulation(pair_models, calibration=True)
        t_create = time.perf_counter() - t0
        tc = []
        for trial in range(-1, args.trials):
            t0 = time.perf_counter(); got = t.triangulate(q, q_calibration_stdev=-1.); dt = time.perf_counter() - t0
            if trial >= 0: tc.append(dt)
        V = got[1].reshape(768, 768)
        out["calibration_noise"] = dict(pairs=256, Nstate=int(mrcal.num_states(**oi)), context_ms=1e3*t_create,
                                        c_triangulate_reused_context=stat(tc), observed_pixel_uncertainty=t.observed_pixel_uncertainty,
                                        symmetric=bool(np.array_equal(V, V.T)), min_eigenvalue_over_max=float(np.linalg.eigvalsh(V)[0]/np.abs(V).max()),
                                        worst_stdev_m=float(np.sqrt(np.diag(V).max())))
        t.close()
        print(f"calibration-time noise, 256 pairs, Nstate {out['calibration_noise']['Nstate']}:")
        print(f"  the context (problem, factorization, sigma): {1e3*t_create:.1f} ms")
        print(f"  (c) triangulate(), context reused: {out['calibration_noise']['c_triangulate_reused_context']}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
