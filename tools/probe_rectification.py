#!/usr/bin/env python3
"""Times the rectification of a stereo pair of the real 6016x4016 calibrations (tests/golden/real_*-0.cameramodel; the
second camera is the first moved 0.3 m to the right and turned a little), OPENCV8 and splined, at the cameras' own
resolution, 160 x 110 degrees (about 23 M rectified pixels):

  (a) Rectification(models, models_rectified): both maps made on the device (a launch a camera) and kept there. The
      kernels' own durations come from a second run under `rocprofv3 --kernel-trace --stats` (tools/kernel_stats_table.py);
      this prints the bytes a launch stores, to hold against the plain-store stream of profiles/LEDGER.md (6.3-6.6 TB/s)
  (b) .rectify() of a uint8 pair, host arrays in and out (two uploads, two launches, two downloads)
  (c) rectification_maps(), the one-shot call, host array out
  (d) the same maps composed of the public pieces: numpy for the grid's vectors and the rotation, project() for the lens
      (three doubles a pixel up, two down), numpy for the cast

(c) and (d) alternate, --trials times after one warm-up; a clock around each call (every call ends in a synchronise);
min / median / max in ms, and one JSON line at the end. Records, not gates. --kernels-only: (a) alone, for the profiler"""
import argparse
import json
import os
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def composed(mrcal, models, models_rectified):
    lensmodel, (fx, fy, cx, cy) = models_rectified[0].intrinsics()
    Naz, Nel = models_rectified[0].imagersize()
    lat, lon = (np.arange(Naz) - cx)/fx, (np.arange(Nel) - cy)/fy
    v = np.empty((Nel, Naz, 3))
    v[..., 0] = np.sin(lat)
    v[..., 1] = np.cos(lat)*np.sin(lon)[:, None]
    v[..., 2] = np.cos(lat)*np.cos(lon)[:, None]
    R_rect_ref = mrcal.R_from_r(models_rectified[0].rt_cam_ref()[:3])
    maps = np.empty((2, Nel, Naz, 2), dtype=np.float32)
    for i, m in enumerate(models):
        R_cam_rect = mrcal.R_from_r(m.rt_cam_ref()[:3]) @ R_rect_ref.T
        maps[i] = mrcal.project(v @ R_cam_rect.T, *m.intrinsics())
    return maps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=3)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--scale", type=float, default=1.0, help="of the cameras' resolution (a rehearsal: 0.05)")
    args = ap.parse_args()
    import mrcal_amd as mrcal
    if not mrcal.gpu_available():
        raise RuntimeError("no HIP device visible: nothing to measure")
    stat = lambda t: dict(min_ms=1e3*min(t), median_ms=1e3*float(np.median(t)), max_ms=1e3*max(t))
    out = {}
    for name in ("opencv8", "splined"):
        model0 = mrcal.cameramodel(os.path.join(ROOT, "tests", "golden", f"real_{name}-0.cameramodel"))
        model1 = mrcal.cameramodel(model0)
        model1.rt_ref_cam(mrcal.compose_rt(model0.rt_ref_cam(), np.array((0.01, 0.02, -0.005, 0.3, 0.01, 0.02))))
        models = (model0, model1)
        models_rectified = mrcal.rectified_system(models, az_fov_deg=160, el_fov_deg=110, az_edge_margin_deg=5,
                                                  pixels_per_deg_az=-args.scale, pixels_per_deg_el=-args.scale)
        Naz, Nel = (int(x) for x in models_rectified[0].imagersize())
        W, H = (int(x) for x in model0.imagersize())
        rec = dict(rectified_imager=(Naz, Nel), bytes_stored_per_map_launch=Naz*Nel*8)
        ta, tb, tc, td = [], [], [], []
        for trial in range(-1, args.trials):
            t0 = time.perf_counter(); r = mrcal.Rectification(models, models_rectified); dt = time.perf_counter() - t0
            if trial >= 0: ta.append(dt)
            if trial < args.trials - 1: r.close()
        rec["a_both_maps_resident"] = stat(ta)
        if not args.kernels_only:
            rng = np.random.default_rng(0)
            images = [rng.integers(0, 256, size=(H, W)).astype(np.uint8) for _ in models]
            outs = (np.empty((Nel, Naz), np.uint8), np.empty((Nel, Naz), np.uint8))
            for trial in range(-1, args.trials):
                t0 = time.perf_counter(); r.rectify(*images, out=outs); dt = time.perf_counter() - t0
                if trial >= 0: tb.append(dt)
            rec["b_rectify_uint8_pair"] = stat(tb)
            for trial in range(-1, args.trials):
                t0 = time.perf_counter(); one_shot = mrcal.rectification_maps(models, models_rectified); dt = time.perf_counter() - t0
                if trial >= 0: tc.append(dt)
                t0 = time.perf_counter(); pieces = composed(mrcal, models, models_rectified); dt = time.perf_counter() - t0
                if trial >= 0: td.append(dt)
            rec["c_rectification_maps_one_shot"] = stat(tc)
            rec["d_public_pieces_composed"]      = stat(td)
            ok = np.isfinite(pieces) & (np.abs(pieces) < 1e6)
            rec["c_vs_d_unequal_share"] = float((one_shot[ok] != pieces[ok]).mean())
            rec["c_vs_d_worst_px"]      = float(np.abs(one_shot[ok] - pieces[ok]).max())
            rec["c_equals_resident_maps"] = bool(np.array_equal(one_shot, r.maps()))
        r.close()
        out[name] = rec
        print(f"{name}: rectified imager {Naz} x {Nel}, {Naz*Nel*8/1e6:.1f} MB stored a map launch")
        for k, v in rec.items():
            if k[1] == "_": print(f"  ({k[0]}) {k[2:]}: {v}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
