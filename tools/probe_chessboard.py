#!/usr/bin/env python3
"""Times find_chessboard_corners() on a rendered board at 800 x 600 and at the real calibration's 6016 x 4016 (uint8, a
10 x 10 board turned by 7 degrees that fills most of the image, edges one pixel soft, noise of 2 grey levels).

For each size: a clock around ChessboardDetector.find_board() (upload, kernels, the copy-out of the candidates and the
lattice on the host), and the five stages the library records: upload, response, candidates (the window test, the scan
and the scatter), refine, from the device's events; grid from the host's clock. --trials runs after one warm-up:
min / median / max in ms. There is nothing to compare with: the reference runs an external detector that is not here,
and no ratio is claimed. The report replaces what follows the marker line in --out (profiles/f13_chessboard.txt: the
resource table above the marker is kept), and one JSON line is printed at the end. Records, not gates."""
import argparse
import json
import os
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MARKER = "== measured by tools/probe_chessboard.py =="
STAGES = ("upload", "response", "candidates", "refine", "grid")


def board_image(W, H, corners=10, degrees=7., noise=2., seed=0):
    """-> (uint8 image, the true corners (corners,corners,2)): squares of min(W,H)/(corners + 3) pixels about the centre"""
    square = min(W, H)/(corners + 3.)
    c, s = np.cos(np.radians(degrees)), np.sin(np.radians(degrees))
    cx, cy = (W - 1)/2., (H - 1)/2.
    rng = np.random.default_rng(seed)
    image = np.zeros((H, W), dtype=np.uint8)
    x = np.arange(W, dtype=np.float32) - cx
    for y0 in range(0, H, 256):                                 # (in bands: the whole image in float would be large)
        y = np.arange(y0, min(y0 + 256, H), dtype=np.float32)[:, None] - cy
        u, v = (c*x + s*y)/square + corners/2., (-s*x + c*y)/square + corners/2.     # (corner (i,j) at u = i + 1/2 ...)
        u, v = u - 0.5, v - 0.5
        inside = (u > -1) & (u < corners) & (v > -1) & (v < corners)
        # +-1 across an edge, over one pixel
        a, b = (np.clip(np.sin(np.pi*t)*square/np.pi, -0.5, 0.5)*2 for t in (u, v))
        level = np.where(inside, 120. - 80.*a*b, 200.) + rng.normal(0., noise, u.shape)
        image[y0:y0 + 256] = np.clip(np.rint(level), 0, 255)
    i, j = np.meshgrid(np.arange(corners) - corners/2. + 0.5, np.arange(corners) - corners/2. + 0.5)
    truth = np.stack((cx + square*(c*i - s*j), cy + square*(s*i + c*j)), axis=-1)
    return image, truth


def stat(values):
    v = sorted(values)
    return v[0], v[len(v)//2], v[-1]


def fmt(name, values):
    return f"  {name:<44s}{stat(values)[0]:10.3f} /{stat(values)[1]:10.3f} /{stat(values)[2]:10.3f} ms"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[800, 600, 6016, 4016], help="W H [W H ...]")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f13_chessboard.txt"))
    args = ap.parse_args()
    import mrcal_amd as mrcal
    if not mrcal.gpu_available():
        raise RuntimeError("no HIP device visible: nothing to measure")

    lines = [MARKER, f"uint8, a 10 x 10 board, the detector's defaults; {args.trials} trials after a warm-up: min / median / max", ""]
    out = dict(runs=[])
    for W, H in zip(args.sizes[0::2], args.sizes[1::2]):
        image, truth = board_image(W, H)
        with mrcal.ChessboardDetector(image.shape, image.dtype) as d:
            board = d.find_board(image, 10)
            if board is None:
                raise RuntimeError(f"{W} x {H}: the board was not found")
            q, _, status = d.candidates(image)
            call, stages = [], {k: [] for k in STAGES}
            for _ in range(args.trials):
                t0 = time.perf_counter(); d.find_board(image, 10); call.append(1e3*(time.perf_counter() - t0))
                for k, v in d.stage_milliseconds().items(): stages[k].append(v)
        error = np.linalg.norm(board - truth, axis=-1)
        lines += [f"{W} x {H}: {len(q)} candidates, {int((status == 0).sum())} refined; the board's corners within {error.max():.3f} px of the rendered ones (rms {np.sqrt((error**2).mean()):.3f})",
                  fmt("ChessboardDetector.find_board()", call)] + [fmt("      " + k, stages[k]) for k in STAGES] + [""]
        out["runs"].append(dict(W=W, H=H, candidates=len(q), call_ms=stat(call)[1], **{k + "_ms": stat(stages[k])[1] for k in STAGES},
                                worst_px=float(error.max())))
    head = []
    if os.path.exists(args.out):
        text = open(args.out).read()
        head = text[:text.index(MARKER)].splitlines() if MARKER in text else text.splitlines()
    with open(args.out, "w") as f:
        f.write("\n".join(head + lines) + "\n")
    print("\n".join(lines))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
