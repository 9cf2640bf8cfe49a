"""The measurements of DESIGN.md section 9 f15: the valid-intrinsics region at the benchmark's size.

    python profiles/f15_valid_region.py [output file]

The benchmark's problem (8 cameras x 1000 frames x 10x10 corners, LENSMODEL_OPENCV8, seed 0), solved; a 30x20 grid.
  1. device time of the binning of all 8 cameras: events around the launches of RegionalStatistics (3 warm-up runs,
     then 20; min and median)
  2. wall time of valid_intrinsics_regions() for the 8 models (1 warm-up, then 3)
  3. wall time of valid_intrinsics_mask() at 6016x4016 (2 warm-up, then 10)
  4. beside them, on this host's CPU: the numpy checker's restatement of _report_regional_statistics() for ONE camera
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mrcal_amd
from mrcal_amd.resident import Problem
from mrcal_amd.synthetic import make_calibration_problem
import valid_region_checker as chk


def main():
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None
    def say(line):
        print(line, flush=True)
        if out: out.write(line + "\n"); out.flush()

    oi, _ = make_calibration_problem(mrcal_amd._api, Ncameras=8, Nframes=1000, lensmodel="LENSMODEL_OPENCV8",
                                     object_width_n=10, object_height_n=10, seed=0)
    t0 = time.perf_counter()
    stats = mrcal_amd.optimize(**oi)
    say(f"optimize(): {time.perf_counter() - t0:.3f} s, rms {stats['rms_reproj_error__pixels']:.4f} px, "
        f"{stats['Noutliers_board']} outliers")
    gw, gh = 30, 20

    with Problem(**oi) as p:
        ms = []
        for i in range(23):
            with mrcal_amd.RegionalStatistics(oi, gw, gh, problem=p) as s:
                ms.append(s.binning_ms())
        x = p.x()
        with mrcal_amd.RegionalStatistics(oi, gw, gh, problem=p) as s:
            first = s.of_camera(0)
    ms = np.array(ms[3:])
    say(f"1. binning, 8 cameras, {gw}x{gh}, device time of the launches: min {ms.min():.4f} ms, median {np.median(ms):.4f} ms, "
        f"max {ms.max():.4f} ms over {ms.size} runs")

    t0 = time.perf_counter()
    mean, stdev, count = chk.regional_statistics(x, oi["observations_board"], oi["indices_frame_camintrinsics_camextrinsics"],
                                                 0, 4000, 2200, gw, gh)
    t_numpy = time.perf_counter() - t0
    say(f"4. the numpy checker, ONE camera, on this host: {t_numpy:.3f} s; counts equal: {np.array_equal(count, first[2])}, "
        f"max |mean - checker| {np.abs(mean - first[0]).max():.3g}")

    models = [mrcal_amd.cameramodel(optimization_inputs=oi, icam_intrinsics=i) for i in range(8)]
    walls = []
    for i in range(4):
        t0 = time.perf_counter()
        regions = mrcal_amd.valid_intrinsics_regions(models, gridn_width=gw, gridn_height=gh)
        walls.append(time.perf_counter() - t0)
    say(f"2. valid_intrinsics_regions(), 8 models: {min(walls[1:]):.3f} s (min of 3; the first call {walls[0]:.3f} s); "
        f"vertices per region: {[None if r is None else int(r.shape[0]) for r in regions]}")

    big = mrcal_amd.cameramodel(intrinsics=("LENSMODEL_PINHOLE", np.array((3000., 3000., 3007.5, 2007.5))), imagersize=(6016, 4016))
    big.valid_intrinsics_region(np.array(((400, 300), (3000, 120), (5600, 350), (5800, 2000), (5500, 3700), (3000, 3900),
                                          (500, 3650), (250, 2000)), dtype=float))
    walls = []
    for i in range(12):
        t0 = time.perf_counter()
        mask = mrcal_amd.valid_intrinsics_mask(big)
        walls.append(time.perf_counter() - t0)
    say(f"3. valid_intrinsics_mask() at 6016x4016, 9 vertices: {1e3*min(walls[2:]):.2f} ms (min of 10, wall, the copy of the "
        f"24 MB to the host included); {mask.mean():.3f} of the pixels inside")


if __name__ == "__main__":
    main()
