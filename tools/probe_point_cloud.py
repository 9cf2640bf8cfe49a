#!/usr/bin/env python3
"""Times stereo_point_cloud() at 1024 x 768 and at the real calibration's 6016 x 4016, on tools/probe_stereo_sgm.py's
pair (uint8, 128 disparities, 8 paths). The two cameras are pinhole cameras side by side whose images are rectified
already (the rectified system is the cameras' own, so the maps are the pixel grid), turned and moved in the reference
frame so that the transform of the points is a real one. Colours from image0, points in the reference frame, float32.

  (a) Rectification.point_cloud() of the matcher's disparity image, given on the host: a clock around the call, the
      three stages on the device from the events the library records, and the copy-out (the read of the N records into
      new host arrays); N as a share of the pixels
  (b) Rectification.point_cloud_of_images(): rectify, match and cloud with nothing but the inputs and the cloud crossing
  (c) the same cloud composed of today's public pieces: stereo_unproject() dense, the transform and the mask in numpy,
      the colours by project() into camera 0 and rounding; and how far (a) is from it

(a) and (b) run --trials times after one warm-up, (c) --composed-trials times; min / median / max in ms. The report
replaces what follows the marker line in --out (profiles/f12_point_cloud.txt: the resource table above the marker is
kept), and one JSON line is printed at the end. Records, not gates."""
import argparse
import json
import os
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from probe_stereo_sgm import pair, stat, fmt

MARKER = "== measured by tools/probe_point_cloud.py =="
STAGES = ("mask", "scan", "scatter")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--composed-trials", type=int, default=2)
    ap.add_argument("--disparities", type=int, default=128)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 768, 6016, 4016], help="W H [W H ...]")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f12_point_cloud.txt"))
    args = ap.parse_args()
    import mrcal_amd as mrcal
    import mrcal_amd.stereo as stereo
    if not mrcal.gpu_available():
        raise RuntimeError("no HIP device visible: nothing to measure")

    # the copy-out apart: a clock around the library's read of the records
    read_ms, library_read = [], stereo._cloud_read
    def timed_read(*a):
        t0 = time.perf_counter(); out = library_read(*a); read_ms.append(1e3*(time.perf_counter() - t0))
        return out
    stereo._cloud_read = timed_read

    D = args.disparities
    rng = np.random.default_rng(0)
    lines = [MARKER, f"uint8, {D} disparities from 0, 8 paths, the matcher's defaults; PINHOLE; colours from image0, frame 'ref', float32 points; "
                     f"{args.trials} trials after a warm-up ((c): {args.composed_trials}): min / median / max", ""]
    out = dict(disparities=D, runs=[])
    for W, H in zip(args.sizes[0::2], args.sizes[1::2]):
        image0, image1 = pair(rng, H, W)
        r, t0, baseline = np.array((0.02, -0.03, 0.01)), np.array((0.3, 0.4, -0.2)), 0.2
        models = [mrcal.cameramodel(intrinsics=('LENSMODEL_PINHOLE', np.array((float(W), float(W), (W - 1)/2., (H - 1)/2.))), imagersize=(W, H),
                                    rt_cam_ref=np.concatenate((r, t0 - np.array((x, 0., 0.))))) for x in (0., baseline)]
        models_rectified = models
        kw = dict(disparity_scale=16, disparity_min=0)
        with mrcal.Rectification(models, models_rectified) as rect:
            disparity = rect.disparity(image0, image1, disparity_max=D)
            wall, copy, stages = [], [], {k: [] for k in STAGES}
            for trial in range(-1, args.trials):
                del read_ms[:]
                t = time.perf_counter(); cloud = rect.point_cloud(disparity, image0=image0, dtype=np.float32, **kw); dt = time.perf_counter() - t
                if trial < 0: continue
                wall.append(1e3*dt); copy.append(read_ms[-1])
                for k, v in rect.point_cloud_stage_milliseconds().items(): stages[k].append(v)
            images, images_stages = [], {k: [] for k in STAGES}
            for trial in range(-1, args.trials):
                t = time.perf_counter(); cloud_b = rect.point_cloud_of_images(image0, image1, dtype=np.float32, disparity_max=D); dt = time.perf_counter() - t
                if trial < 0: continue
                images.append(1e3*dt)
                for k, v in rect.point_cloud_stage_milliseconds().items(): images_stages[k].append(v)
            same = all(a.tobytes() == b.tobytes() for a, b in zip(cloud, cloud_b))
            cloud64 = rect.point_cloud(disparity, image0=image0, **kw)

        # (c) today's public pieces
        composed = []
        Rt_ref_rect0 = models_rectified[0].Rt_ref_cam()
        Rt_cam0_rect0 = mrcal.compose_Rt(models[0].Rt_cam_ref(), Rt_ref_rect0)
        for trial in range(args.composed_trials):
            t = time.perf_counter()
            p_rect0 = mrcal.stereo_unproject(disparity, models_rectified, disparity_scale=16)      # (H,W,3), zeros where invalid
            kept = (p_rect0 != 0).any(axis=-1)
            p = p_rect0[kept]
            q = mrcal.project(p @ Rt_cam0_rect0[:3].T + Rt_cam0_rect0[3], *models[0].intrinsics())
            iq = np.floor(q + 0.5).astype(np.int64)
            inside = (iq[:, 0] >= 0) & (iq[:, 0] < W) & (iq[:, 1] >= 0) & (iq[:, 1] < H)
            points_c = (p[inside] @ Rt_ref_rect0[:3].T + Rt_ref_rect0[3]).astype(np.float32)
            color_c  = image0[iq[inside, 1], iq[inside, 0]]
            index_c  = np.flatnonzero(kept.ravel())[inside].astype(np.int32)
            composed.append(1e3*(time.perf_counter() - t))
        N = len(cloud[2])
        run = dict(width=W, height=H, N=N, share=N/float(W*H), a_call=stat(wall), a_stages={k: stat(v) for k, v in stages.items()},
                   a_copy_out=stat(copy), b_call=stat(images), b_stages={k: stat(v) for k, v in images_stages.items()},
                   b_equals_a=bool(same), c_call=stat(composed))
        # how far (a), in double, is from (c): the pixels both keep
        both, ia, ic = np.intersect1d(cloud64[2], index_c, return_indices=True)
        run["c_index_equal"] = bool(np.array_equal(cloud64[2], index_c))
        run["c_only_one_keeps"] = int(len(cloud64[2]) + len(index_c) - 2*len(both))
        run["c_points_max_diff"] = float(np.abs(cloud64[0][ia] - points_c[ic].astype(np.float64)).max()) if len(both) else 0.
        run["c_points_scale"]    = float(np.abs(cloud64[0]).max()) if N else 0.
        run["c_colors_unequal"]  = int(np.count_nonzero(cloud64[1][ia] != color_c[ic]))
        lines.append(f"{W} x {H}: N = {N}, {run['share']:.4f} of the pixels")
        lines.append(f"  (a) Rectification.point_cloud()            {fmt(run['a_call'])}")
        for k in STAGES:
            lines.append(f"        {k:<37}{fmt(run['a_stages'][k])}")
        lines.append(f"        {'copy-out of the N records':<37}{fmt(run['a_copy_out'])}")
        lines.append(f"  (b) Rectification.point_cloud_of_images()  {fmt(run['b_call'])}")
        for k in STAGES:
            lines.append(f"        {k:<37}{fmt(run['b_stages'][k])}")
        lines.append(f"      its cloud is {'the same bits as' if same else 'NOT the same as'} (a)'s")
        lines.append(f"  (c) composed of the public pieces          {fmt(run['c_call'])}")
        lines.append(f"      (a) in float64 against (c): the kept pixels are {'the same' if run['c_index_equal'] else 'NOT the same'} "
                     f"({run['c_only_one_keeps']} kept by one only); points differ by at most {run['c_points_max_diff']:.3g} "
                     f"(float32 of coordinates up to {run['c_points_scale']:.3g}); {run['c_colors_unequal']} colours differ")
        lines.append("")
        out["runs"].append(run)
    report = "\n".join(lines) + "\n"
    head = ""
    if os.path.exists(args.out):
        head = open(args.out).read().split(MARKER)[0]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f: f.write(head + report)
    print(report)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
