#!/usr/bin/env python3
"""Times stereo_matching_sgm() through a StereoMatcherSGM that is made once, uint8, at 1024 x 768 and at the real
calibration's 6016 x 4016, 128 disparities, for 4 and 8 paths (filtered noise; image1 is image0 seen through a
disparity that grows from 20 to 100 px across the image):

  (a) StereoMatcherSGM.match(): a clock around the call (host arrays in, the disparity image out)
  (b) each stage on the device, from the events the library records around them: the census of both images, the
      paths (4 or 8 launches), the selection, the left-right check; and the path updates a second, H W D paths over
      the paths' time
  (c) for orientation, the checker of the tests (numpy, int64) on the host at --host-size, and its updates a second

(a) and (b) run --trials times after one warm-up; min / median / max in ms. The report replaces what follows the
marker line in --out (profiles/f10_stereo_sgm.txt: the resource table above the marker is kept), and one JSON line is
printed at the end. Records, not gates."""
import argparse
import json
import os
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MARKER = "== measured by tools/probe_stereo_sgm.py =="


def filtered_noise(rng, shape):
    """white noise through a separable 5-tap box, stretched to 0..255"""
    a = rng.standard_normal(shape, dtype=np.float32)
    for axis in (0, 1):
        a = sum(np.roll(a, s, axis=axis) for s in range(-2, 3))/5.
    a = (a - a.min())/(a.max() - a.min())
    return np.round(a*255.).astype(np.uint8)


def pair(rng, H, W):
    image0 = filtered_noise(rng, (H, W))
    x1 = np.arange(W)
    d  = np.rint(20 + 80.*x1/W).astype(int)          # the RIGHT image's disparity at x1
    image1 = image0[:, np.minimum(x1 + d, W - 1)]
    return image0, np.ascontiguousarray(image1)


def stat(t):
    return dict(min_ms=float(min(t)), median_ms=float(np.median(t)), max_ms=float(max(t)))


def fmt(s):
    return f"{s['min_ms']:9.3f} / {s['median_ms']:9.3f} / {s['max_ms']:9.3f} ms"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--disparities", type=int, default=128)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 768, 6016, 4016], help="W H [W H ...]")
    ap.add_argument("--host-size", type=int, nargs=2, default=[256, 192], help="W H of the checker's run; 0 0: none")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f10_stereo_sgm.txt"))
    args = ap.parse_args()
    import mrcal_amd as mrcal
    if not mrcal.gpu_available():
        raise RuntimeError("no HIP device visible: nothing to measure")

    D = args.disparities
    rng = np.random.default_rng(0)
    lines = [MARKER, f"uint8, {D} disparities from 0, P1 = 10, P2 = 120, uniqueness_ratio = 10, disp12_max_diff = 1; "
                     f"{args.trials} trials after a warm-up: min / median / max", ""]
    out = dict(disparities=D, runs=[])
    for W, H in zip(args.sizes[0::2], args.sizes[1::2]):
        image0, image1 = pair(rng, H, W)
        for paths in (4, 8):
            with mrcal.StereoMatcherSGM((H, W), np.uint8, disparity_max=D, paths=paths) as matcher:
                wall, stages = [], dict(census=[], paths=[], select=[], check=[])
                for trial in range(-1, args.trials):
                    t0 = time.perf_counter(); d = matcher.match(image0, image1); dt = time.perf_counter() - t0
                    if trial < 0: continue
                    wall.append(1e3*dt)
                    for k, v in matcher.stage_milliseconds().items(): stages[k].append(v)
            updates = float(H)*W*D*paths
            run = dict(width=W, height=H, paths=paths, a_match=stat(wall), b_stages={k: stat(v) for k, v in stages.items()},
                       b_path_updates_per_s=updates/(1e-3*min(stages["paths"])), valid=float((d >= 0).mean()))
            out["runs"].append(run)
            lines.append(f"{W} x {H}, paths = {paths}: {updates:.3g} path updates; {run['valid']:.3f} of the pixels valid")
            lines.append(f"  (a) StereoMatcherSGM.match()      {fmt(run['a_match'])}")
            for k in ("census", "paths", "select", "check"):
                lines.append(f"  (b) {k:<30}{fmt(run['b_stages'][k])}")
            lines.append(f"      path updates a second        {run['b_path_updates_per_s']:.3g}")
            lines.append("")
    Wh, Hh = args.host_size
    if Wh > 0 and Hh > 0:
        import stereo_sgm_checker as chk
        image0, image1 = pair(rng, Hh, Wh)
        for paths in (4, 8):
            t0 = time.perf_counter(); expected = chk.stereo_matching_sgm(image0, image1, disparity_max=D, paths=paths); dt = time.perf_counter() - t0
            same = bool(np.array_equal(expected, mrcal.stereo_matching_sgm(image0, image1, disparity_max=D, paths=paths)))
            rate = float(Hh)*Wh*D*paths/dt
            out["runs"].append(dict(host_checker=True, width=Wh, height=Hh, paths=paths, seconds=dt, path_updates_per_s=rate, equal=same))
            lines.append(f"  (c) the checker on the host, {Wh} x {Hh}, paths = {paths}: {dt:.2f} s, {rate:.3g} path updates a second "
                         f"(everything, not the paths alone); the device's result is {'the same bits' if same else 'NOT the same'}")
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
