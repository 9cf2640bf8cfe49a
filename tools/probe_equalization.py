#!/usr/bin/env python3
"""Times the equalization at the real calibration's 6016 x 4016 (and at 1024 x 768), uint8 and uint16, on
tools/probe_stereo_sgm.py's pair (filtered noise; uint16: times 257 plus two low bits of noise):

  (a) ImageEqualizer.apply() for CLAHE (8 x 8 tiles, clip_limit 8: mrcal's) and for stretch: the three stages on the
      device from the events the library records (histogram, lut, apply; stretch: the extremes, 0, the map), a clock
      around the call (host arrays in and out), and the apply kernel's bytes a second (a pixel read and a pixel written)
  (b) Rectification.disparity(image0, image1, equalization='clahe') against the same call without the keyword, the two
      alternating: what the equalization of both raw images adds
  (c) at the first size, once: the result against the numpy checker of the tests, every pixel

(a) and (b) run --trials times after --warmup calls; min / median / max in ms. The report is written to --out and one
JSON line is printed at the end. Records, not gates."""
import argparse
import json
import os
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from probe_stereo_sgm import pair, stat, fmt

STAGES = ("histogram", "lut", "apply")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--disparities", type=int, default=128)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 768, 6016, 4016], help="W H [W H ...]")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f14_equalization.txt"))
    args = ap.parse_args()
    import mrcal_amd as mrcal
    import equalize_checker as chk
    if not mrcal.gpu_available():
        raise RuntimeError("no HIP device visible: nothing to measure")

    rng = np.random.default_rng(0)
    lines = [f"CLAHE: 8 x 8 tiles, clip_limit 8; {args.trials} trials after {args.warmup} warm-up calls: min / median / max", ""]
    out = dict(runs=[])
    checked = False
    for W, H in zip(args.sizes[0::2], args.sizes[1::2]):
        image0, image1 = pair(rng, H, W)
        for dtype in (np.uint8, np.uint16):
            if dtype is np.uint8: images = (image0, image1)
            else: images = tuple(i.astype(np.uint16)*257 + rng.integers(0, 4, size=i.shape, dtype=np.uint16) for i in (image0, image1))
            run = dict(width=W, height=H, dtype=np.dtype(dtype).name)
            lines.append(f"{W} x {H} {run['dtype']}")
            for method in ("clahe", "stretch"):
                with mrcal.ImageEqualizer((H, W), dtype, method) as e:
                    wall, stages = [], {k: [] for k in STAGES}
                    for trial in range(-args.warmup, args.trials):
                        t = time.perf_counter(); got = e.apply(images[0]); dt = time.perf_counter() - t
                        if trial < 0: continue
                        wall.append(1e3*dt)
                        for k, v in e.stage_milliseconds().items(): stages[k].append(v)
                if not checked and method == "clahe":
                    run["equals_checker"] = bool(np.array_equal(got, chk.equalize_clahe(images[0], 8.0, (8, 8))))
                    lines.append(f"  the CLAHE result {'EQUALS' if run['equals_checker'] else 'DIFFERS FROM'} the numpy checker's, every pixel")
                run[method] = dict(call=stat(wall), stages={k: stat(v) for k, v in stages.items()})
                moved = W*H*(np.dtype(dtype).itemsize + got.dtype.itemsize)
                run[method]["apply_TB_per_s"] = moved/(1e-3*np.median(stages["apply"]))/1e12
                lines.append(f"  (a) {method:<8} ImageEqualizer.apply()    {fmt(run[method]['call'])}")
                for k in STAGES:
                    lines.append(f"        {k:<33}{fmt(run[method]['stages'][k])}")
                lines.append(f"        apply: {moved/1e6:.1f} MB read and written, {run[method]['apply_TB_per_s']:.3f} TB/s at the median")
            # (b) what it adds to the resident chain
            r, t0 = np.array((0.02, -0.03, 0.01)), np.array((0.3, 0.4, -0.2))
            models = [mrcal.cameramodel(intrinsics=('LENSMODEL_PINHOLE', np.array((float(W), float(W), (W - 1)/2., (H - 1)/2.))), imagersize=(W, H),
                                        rt_cam_ref=np.concatenate((r, t0 - np.array((x, 0., 0.))))) for x in (0., 0.2)]
            with mrcal.Rectification(models, models) as rect:
                without, with_clahe = [], []
                for trial in range(-args.warmup, args.trials):
                    t = time.perf_counter(); rect.disparity(*images, disparity_max=args.disparities); a = time.perf_counter() - t
                    t = time.perf_counter(); rect.disparity(*images, disparity_max=args.disparities, equalization='clahe'); b = time.perf_counter() - t
                    if trial < 0: continue
                    without.append(1e3*a); with_clahe.append(1e3*b)
            run["disparity"] = dict(without=stat(without), with_clahe=stat(with_clahe),
                                    added_median_ms=float(np.median(np.array(with_clahe) - np.array(without))))
            lines.append(f"  (b) Rectification.disparity()          {fmt(run['disparity']['without'])}")
            lines.append(f"      ... equalization='clahe'           {fmt(run['disparity']['with_clahe'])}")
            lines.append(f"      added, the median of the pairs' differences: {run['disparity']['added_median_ms']:.3f} ms")
            lines.append("")
            out["runs"].append(run)
        checked = True
    report = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f: f.write(report)
    print(report)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
