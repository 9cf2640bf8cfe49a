#!/usr/bin/env python3
"""Prints one line per case with a SHA-256 (first 32 hex digits) over the bytes of what the calibration-noise
propagation returns - projection uncertainty, triangulate() with calibration-time noise, projection_diff() with
uncertainties - and mrcal_amd_device_buffers_live() before and after the case. Two builds of the library that print the
same lines compute the same bits: run it once per build (MRCAL_AMD_LIB=<the other build>), a fresh process each, and
diff the outputs (profiles/noise_propagation_refactor.txt).

The cases are the tests' own small shapes (tests/test_projection_uncertainty.py, tests/test_triangulation.py) and, unless
--no-benchmark-problem, the benchmark's problem (8 cameras x 1000 frames x 10x10, OPENCV8, seed 0, solved)."""
import argparse
import hashlib
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

SPLINED = "LENSMODEL_SPLINED_STEREOGRAPHIC_order=3_Nx=8_Ny=6_fov_x_deg=80"
METHODS = ("cross-reprojection-ccp", "cross-reprojection-rrp-Jfp")
WHATS   = ("covariance", "worstdirection-stdev", "rms-stdev")
PAIRS3  = ((0, 1), (1, 2), (0, 2))


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:32]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-benchmark-problem", action="store_true")
    args = ap.parse_args()
    import mrcal_amd as amd
    from mrcal_amd.synthetic import make_calibration_problem, copy_inputs
    from test_projection_uncertainty import board_problem, points_problem, some_points
    from probe_triangulation import pixel_pairs
    if not amd.gpu_available():
        raise RuntimeError("no HIP device visible: nothing to probe")

    def case(name, f):
        before = amd.device_buffers_live()
        value = f()
        print(f"{name:<78s} {value} live {before} -> {amd.device_buffers_live()}", flush=True)

    def solved(oi):
        oi = copy_inputs(oi)
        amd.optimize(**oi)
        return oi

    def uncertainty_cases(tag, oi, icams, methods=METHODS, sigmas=(None, 0.5), whats=WHATS, p=None):
        p = some_points(23, seed=5) if p is None else p
        for icam in icams:
            m = amd.cameramodel(optimization_inputs=oi, icam_intrinsics=icam)
            for method in methods:
                for sigma in sigmas:
                    def f():
                        with_sigma = []
                        u = amd.ProjectionUncertainty(m, method=method, observed_pixel_uncertainty=sigma)
                        for atinfinity in (False, True):
                            for what in whats:
                                with_sigma.append(u.evaluate(p, atinfinity=atinfinity, what=what))
                        s = u.observed_pixel_uncertainty
                        u.close()
                        return sha(np.array(s), *with_sigma)
                    case(f"uncertainty {tag} icam {icam} {method} sigma {sigma}", f)

    def triangulation_cases(tag, oi, Ns, stabilize=(True, False), sigmas=(-1., 0.4), observation=(None, 0.3)):
        models = [amd.cameramodel(optimization_inputs=oi, icam_intrinsics=i) for i in range(3)]
        for N in Ns:
            pairs = [PAIRS3[i % 3] for i in range(N)] if N > 1 else [PAIRS3[1]]
            q = pixel_pairs(amd, models, pairs, seed=3000 + N)
            pair_models = np.array([[models[a], models[b]] for a, b in pairs], dtype=object)
            for stab in stabilize:
                for sigma in sigmas:
                    for obs in observation:
                        def f():
                            with amd.Triangulation(pair_models, calibration=True) as t:
                                r = t.triangulate(q, q_calibration_stdev=sigma, q_observation_stdev=obs,
                                                  q_observation_stdev_correlation=(0.5 if obs else 0.), stabilize_coords=stab)
                                return sha(np.array(t.observed_pixel_uncertainty), *r)
                        case(f"triangulate {tag} N {N} stabilize {stab} sigma {sigma} observation {obs}", f)

    oi = solved(board_problem(amd._api, Ncameras=3))
    uncertainty_cases("boards OPENCV8", oi, (0, 1, 2))
    oi4 = board_problem(amd._api, Ncameras=3, lensmodel="LENSMODEL_OPENCV4")
    oi4["do_apply_regularization"] = False
    oi4 = solved(oi4)
    uncertainty_cases("boards OPENCV4 no regularization", oi4, (0, 1))
    uncertainty_cases("points", points_problem(), (0, 2))
    uncertainty_cases("splined", board_problem(amd._api, Ncameras=2, lensmodel=SPLINED, do_optimize_intrinsics_core=False), (1,), sigmas=(0.5,))

    def tri_problem(lensmodel="LENSMODEL_OPENCV8", **flags):
        oi, _ = make_calibration_problem(amd._api, Ncameras=3, Nframes=6, lensmodel=lensmodel, seed=11)
        oi.update(flags)
        amd.optimize(**oi)
        return oi
    triangulation_cases("OPENCV8", tri_problem(), (1, 65))
    triangulation_cases("OPENCV4 no regularization", tri_problem("LENSMODEL_OPENCV4", do_apply_regularization=False), (65,), sigmas=(0.4,), observation=(None,))
    triangulation_cases("frames fixed", tri_problem(do_optimize_frames=False), (65,), sigmas=(0.4,), observation=(None,))
    triangulation_cases("splined", tri_problem(SPLINED, do_optimize_intrinsics_core=False), (3,), stabilize=(True,), sigmas=(0.4,), observation=(None,))

    # projection_diff() with uncertainties, on two small models
    oia = solved(board_problem(amd._api, Ncameras=2, seed=3))
    oib = solved(board_problem(amd._api, Ncameras=2, seed=4))
    ma, mb = (amd.cameramodel(optimization_inputs=o, icam_intrinsics=1) for o in (oia, oib))
    case("projection_diff use_uncertainties", lambda: sha(*[np.asarray(a) for a in
         amd.projection_diff((ma, mb), gridn_width=12, gridn_height=9, use_uncertainties=True, distance=(5., 50.))]))

    if not args.no_benchmark_problem:
        oi, _ = make_calibration_problem(amd._api, Ncameras=8, Nframes=1000, seed=0)
        amd.optimize(**oi)
        uncertainty_cases("benchmark problem", oi, (3,), methods=METHODS[:1], sigmas=(0.3,), whats=WHATS[:1], p=some_points(20, seed=7))
        models = [amd.cameramodel(optimization_inputs=oi, icam_intrinsics=i) for i in range(8)]
        pairs = [(i % 7, i % 7 + 1) for i in range(256)]
        q = pixel_pairs(amd, models, pairs, seed=1)
        pair_models = np.array([[models[a], models[b]] for a, b in pairs], dtype=object)
        case("triangulate benchmark problem N 256 sigma estimated",
             lambda: sha(*amd.triangulate(q, pair_models, q_calibration_stdev=-1.)))


if __name__ == "__main__":
    main()
