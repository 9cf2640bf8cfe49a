#!/usr/bin/env python3
"""Times filter_speckles() at 1024 x 768 and at the real calibration's 6016 x 4016, on the disparity image that
tools/probe_stereo_sgm.py's pair gives (uint8, 128 disparities, 8 paths) once a band of image1, the columns from W/2 to
5W/8, is uniform noise: nothing matches there, so many small regions (the band, the occlusions) and a few huge ones
(the surface either side) are both present. With cv2's recommended speckleWindowSize = 200, speckleRange = 2:

  (a) SpeckleFilter.filter() through a filter that is made once: a clock around the call (host arrays in and out), the
      device time from the events the library records, and each of the four passes
  (b) the filter as the last stage of StereoMatcherSGM.match(): the four stages as before, and the filter's time
  (c) the device's result against the checker of the tests (scipy's connected components) at --check-size and smaller

(a) and (b) run --trials times after one warm-up; min / median / max in ms. The report replaces what follows the
marker line in --out (profiles/f11_speckle_filter.txt: the resource table above the marker is kept), and one JSON line
is printed at the end. Records, not gates."""
import argparse
import json
import os
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from probe_stereo_sgm import pair, stat, fmt

MARKER = "== measured by tools/probe_speckle_filter.py =="
PASSES = ("label", "merge", "count", "apply")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--disparities", type=int, default=128)
    ap.add_argument("--window", type=int, default=200, help="speckle_window_size")
    ap.add_argument("--range", type=int, default=2, help="speckle_range")
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 768, 6016, 4016], help="W H [W H ...]")
    ap.add_argument("--check-size", type=int, default=6016*4016,
                    help="the checker runs on images of at most so many pixels (6016 x 4016: 5 s and 2 GB on the host)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f11_speckle_filter.txt"))
    args = ap.parse_args()
    import mrcal_amd as mrcal
    if not mrcal.gpu_available():
        raise RuntimeError("no HIP device visible: nothing to measure")

    D = args.disparities
    invalid, max_diff = -16, 16*args.range
    rng = np.random.default_rng(0)
    lines = [MARKER, f"uint8, {D} disparities from 0, 8 paths, the matcher's defaults; columns W/2 .. 5W/8 of image1 are noise; "
                     f"speckle_window_size = {args.window}, speckle_range = {args.range}; {args.trials} trials after a warm-up: min / median / max", ""]
    out = dict(disparities=D, window=args.window, range=args.range, runs=[])
    for W, H in zip(args.sizes[0::2], args.sizes[1::2]):
        image0, image1 = pair(rng, H, W)
        image1[:, W//2:5*W//8] = rng.integers(0, 256, size=(H, 5*W//8 - W//2), dtype=np.uint8)
        with mrcal.StereoMatcherSGM((H, W), np.uint8, disparity_max=D) as matcher:
            plain = matcher.match(image0, image1)
        kw = dict(new_value=invalid, max_speckle_size=args.window, max_diff=max_diff)
        with mrcal.SpeckleFilter((H, W)) as f:
            wall, device, passes = [], [], {k: [] for k in PASSES}
            for trial in range(-1, args.trials):
                t0 = time.perf_counter(); filtered = f.filter(plain, **kw); dt = time.perf_counter() - t0
                if trial < 0: continue
                wall.append(1e3*dt); device.append(f.milliseconds())
                for k, v in f.pass_milliseconds().items(): passes[k].append(v)
        with mrcal.StereoMatcherSGM((H, W), np.uint8, disparity_max=D, speckle_window_size=args.window, speckle_range=args.range) as matcher:
            match, stages, speckle = [], dict(census=[], paths=[], select=[], check=[]), []
            for trial in range(-1, args.trials):
                t0 = time.perf_counter(); d = matcher.match(image0, image1); dt = time.perf_counter() - t0
                if trial < 0: continue
                match.append(1e3*dt); speckle.append(matcher.speckle_milliseconds())
                for k, v in matcher.stage_milliseconds().items(): stages[k].append(v)
        same_stage = bool(np.array_equal(d, filtered))
        run = dict(width=W, height=H, valid_before=float((plain != invalid).mean()), valid_after=float((filtered != invalid).mean()),
                   a_filter=stat(wall), a_device=stat(device), a_passes={k: stat(v) for k, v in passes.items()},
                   b_match=stat(match), b_stages={k: stat(v) for k, v in stages.items()}, b_speckle=stat(speckle),
                   b_equals_a=same_stage)
        lines.append(f"{W} x {H}: {run['valid_before']:.4f} of the pixels valid before, {run['valid_after']:.4f} after")
        lines.append(f"  (a) SpeckleFilter.filter()        {fmt(run['a_filter'])}")
        lines.append(f"      on the device                 {fmt(run['a_device'])}")
        for k in PASSES:
            lines.append(f"        {k:<28}{fmt(run['a_passes'][k])}")
        lines.append(f"  (b) StereoMatcherSGM.match()      {fmt(run['b_match'])}")
        for k in ("census", "paths", "select", "check"):
            lines.append(f"        {k:<28}{fmt(run['b_stages'][k])}")
        lines.append(f"        {'speckle filter':<28}{fmt(run['b_speckle'])}")
        lines.append(f"      its result is {'the same bits as' if same_stage else 'NOT the same as'} (a)'s")
        if H*W <= args.check_size:
            import speckle_checker as chk
            t0 = time.perf_counter(); expected = chk.filter_speckles(plain, invalid, args.window, max_diff); dt = time.perf_counter() - t0
            run["c_equal"] = bool(np.array_equal(expected, filtered)); run["c_seconds"] = dt
            lines.append(f"  (c) the checker on the host: {dt:.2f} s; the device's result is {'the same bits' if run['c_equal'] else 'NOT the same'}")
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
