#!/usr/bin/env python3
"""Times match_feature() at the size mrcal-triangulate meets: 256 features of one pair of 4000 x 3000 uint8 images
(filtered noise; image1 is image0 moved by a few pixels), template 41 x 41, search radius 200, TM_CCORR_NORMED, through a
FeatureMatcher that is made once:

  (a) FeatureMatcher.match() of the 256 features: a clock around the call (it ends in the copies of q1 and status)
  (b) the multiply-adds of the surfaces, 256 x 401^2 x 41^2 = 6.9e10, over (a): a floor for what the correlation kernel
      does a second. The kernel's own duration comes from a second run under the profiler, by itself:
          rocprofv3 --kernel-trace --stats -- python tools/probe_match_feature.py --kernels-only
      (tools/kernel_stats_table.py reads the result); --kernel-ms takes that number and prints the rate it implies
  (c) for comparison, the same surfaces on the host: scipy.signal.fftconvolve for IT and the window sums, the way
      cv2.matchTemplate() works (cv2 itself is not available here), for --host-features of the features

(a) runs --trials times after one warm-up; min / median / max in ms, and one JSON line at the end. Records, not gates."""
import argparse
import json
import os
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def filtered_noise(rng, shape):
    """white noise through a separable 5-tap box, stretched to 0..255: texture at the scale of a template"""
    a = rng.standard_normal(shape)
    k = np.ones(5)/5.
    a = np.apply_along_axis(lambda r: np.convolve(r, k, mode="same"), 1, a)
    a = np.apply_along_axis(lambda c: np.convolve(c, k, mode="same"), 0, a)
    a = (a - a.min())/(a.max() - a.min())
    return np.round(a*255.).astype(np.uint8)


def host_surface(cut, template):
    """TM_CCORR_NORMED by FFT, in double"""
    from scipy.signal import fftconvolve
    I, T = cut.astype(float), template.astype(float)
    IT  = fftconvolve(I, T[::-1, ::-1], mode="valid")
    SI2 = fftconvolve(I*I, np.ones(T.shape), mode="valid")
    return (IT/np.sqrt(SI2*(T*T).sum())).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--features", type=int, default=256)
    ap.add_argument("--template", type=int, default=41)
    ap.add_argument("--radius", type=int, default=200)
    ap.add_argument("--width", type=int, default=4000)
    ap.add_argument("--height", type=int, default=3000)
    ap.add_argument("--host-features", type=int, default=4)
    ap.add_argument("--kernels-only", action="store_true", help="one warm-up and one match(), for the profiler")
    ap.add_argument("--kernel-ms", type=float, default=None, help="the correlation kernel's duration from the profiler's run")
    args = ap.parse_args()
    import mrcal_amd as mrcal
    if not mrcal.gpu_available():
        raise RuntimeError("no HIP device visible: nothing to measure")

    rng = np.random.default_rng(0)
    image0 = filtered_noise(rng, (args.height, args.width))
    shift  = np.array((7, -5))
    image1 = np.roll(image0, (shift[1], shift[0]), axis=(0, 1))
    N, ts, r = args.features, args.template, args.radius
    margin = r + ts
    q0 = np.stack((rng.uniform(margin, args.width - margin, size=N), rng.uniform(margin, args.height - margin, size=N)), axis=-1)
    q1e = q0 + rng.uniform(-20, 20, size=(N, 2))
    kw = dict(q1_estimate=q1e, search_radius1=r, template_size1=ts, method=mrcal.TM_CCORR_NORMED)
    macs = float(N)*(2*r + 1)**2*ts**2

    out = dict(features=N, template=ts, radius=r, image=(args.width, args.height), multiply_adds=macs)
    stat = lambda t: dict(min_ms=1e3*min(t), median_ms=1e3*float(np.median(t)), max_ms=1e3*max(t))
    with mrcal.FeatureMatcher(image0, image1) as matcher:
        times = []
        for trial in range(-1, 1 if args.kernels_only else args.trials):
            t0 = time.perf_counter(); q1, status = matcher.match(q0, **kw); dt = time.perf_counter() - t0
            if trial >= 0: times.append(dt)
        out["a_match"] = stat(times)
        out["b_multiply_adds_per_s_over_a"] = macs/min(times)
        if args.kernel_ms is not None:
            out["b_multiply_adds_per_s_kernel"] = macs/(1e-3*args.kernel_ms)
        found = status == 0
        out["found"] = int(found.sum())
        out["worst_error_px"] = float(np.abs(q1[found] - (q0[found] + shift)).max()) if found.any() else None
        if not args.kernels_only and args.host_features > 0:
            n = min(N, args.host_features)
            q1n, statusn, diag = matcher.match(q0[:n], **{**kw, "q1_estimate": q1e[:n]}, diagnostics=True)
            th, worst = [], 0.
            for i in range(n):
                z = diag[i]["matchoutput_image"]
                tmin = np.round(q1e[i] - (ts - 1.)/2.).astype(int)
                qmin = np.maximum(tmin - r, 0)
                cut  = image1[qmin[1]:qmin[1] + z.shape[0] + ts - 1, qmin[0]:qmin[0] + z.shape[1] + ts - 1]
                t0 = time.perf_counter(); zh = host_surface(cut, diag[i]["template"]); th.append(time.perf_counter() - t0)
                worst = max(worst, float(np.abs(zh - z).max()))
            out["c_host_fftconvolve_per_feature"] = stat(th)
            out["c_host_vs_device_worst_difference"] = worst
    for k, v in out.items(): print(f"  {k}: {v}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
