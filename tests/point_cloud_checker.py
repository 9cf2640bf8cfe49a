"""CHECKER of stereo_point_cloud(): the definition (include/mrcal_amd.h, "stereo_point_cloud") restated in numpy, in
double, and a second time as plain per-pixel loops. Test code: nothing of the product runs here.

point_cloud() asserts for itself that no pixel's range lies within 1e-9 relative of a range_min / range_max it is
given: a bound on such a tie would make the verdict a matter of rounding, and a case has to pick its bounds clear of it.
"""
import math

import numpy as np


def ranges_and_vectors(d_pixels, W, H, rectification_model, fxycxy, baseline):
    """per pixel of the (H,W) rectified image: the range (H,W) of the disparity d_pixels (H,W), in pixels, and the unit
    observation vector (H,W,3). The formulas of stereo_range() and stereo_unproject(), restated"""
    fx, fy, cx, cy = fxycxy
    x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    ux, uy = (x - cx)/fx, (y - cy)/fy
    with np.errstate(all='ignore'):
        parallax = d_pixels/fx
        if rectification_model == 'LENSMODEL_LATLON':
            r = baseline*np.cos(ux - parallax)/np.sin(parallax)
            v = np.stack((np.sin(ux), np.cos(ux)*np.sin(uy), np.cos(ux)*np.cos(uy)), axis=-1)
        elif rectification_model == 'LENSMODEL_PINHOLE':
            r = baseline/parallax*np.sqrt(ux*ux + uy*uy + 1.)
            s = 1./np.sqrt(ux*ux + uy*uy + 1.)
            v = np.stack((ux*s, uy*s, s), axis=-1)
        else:
            raise Exception(rectification_model)
    return r, v


def point_cloud(disparity, rectification_model, fxycxy, baseline, *, disparity_scale=1, disparity_scaled_min=0,
                disparity_scaled_max=None, range_min=None, range_max=None, map0=None, image0=None, Rt_out_rect0=None):
    """-> points (N,3) float64, color (N,) or (N,3) or None, index (N,) int32, and the ranges (N,) of the kept pixels.
    map0: (H,W,2) float32, taken as given. Rt_out_rect0: (4,3) or None"""
    H, W = disparity.shape
    if disparity_scaled_max is None:
        disparity_scaled_max = 0x7FFF if disparity.dtype == np.int16 else 0xFFFF
    d = disparity.astype(np.uint16).astype(np.int64)
    keep = (d > 0) & (d >= disparity_scaled_min) & (d <= disparity_scaled_max)
    r, v = ranges_and_vectors(d/float(disparity_scale), W, H, rectification_model, fxycxy, baseline)
    with np.errstate(all='ignore'):
        keep &= np.isfinite(r) & (r > 0)
        for bound in (range_min, range_max):
            if bound is not None and np.isfinite(bound) and bound > 0:
                tie = keep & (np.abs(r - bound) <= 1e-9*bound)
                assert not tie.any(), f"the range {r[tie][0]!r} of pixel {np.argwhere(tie)[0]} is on the bound {bound!r}"
        if range_min is not None: keep &= r >= range_min
        if range_max is not None: keep &= r <= range_max
    color = None
    if image0 is not None:
        assert map0.dtype == np.float32 and map0.shape == (H, W, 2)
        with np.errstate(all='ignore'):
            ix = np.floor(map0[..., 0] + np.float32(0.5))
            iy = np.floor(map0[..., 1] + np.float32(0.5))
            assert ix.dtype == np.float32
            inside = np.isfinite(ix) & np.isfinite(iy) & (ix >= 0) & (ix < image0.shape[1]) & (iy >= 0) & (iy < image0.shape[0])
        keep &= inside
        color = image0[iy[keep].astype(np.int64), ix[keep].astype(np.int64)]
    points = (r[..., None]*v)[keep]
    if Rt_out_rect0 is not None:
        points = points @ Rt_out_rect0[:3].T + Rt_out_rect0[3]
    return points, color, np.flatnonzero(keep.ravel()).astype(np.int32), r[keep]


def point_cloud_loops(disparity, rectification_model, fxycxy, baseline, *, disparity_scale=1, disparity_scaled_min=0,
                      disparity_scaled_max=None, range_min=None, range_max=None, map0=None, image0=None, Rt_out_rect0=None):
    """the same, a pixel at a time in Python floats: points, color, index"""
    H, W = disparity.shape
    fx, fy, cx, cy = (float(f) for f in fxycxy)
    if disparity_scaled_max is None:
        disparity_scaled_max = 0x7FFF if disparity.dtype == np.int16 else 0xFFFF
    points, color, index = [], [], []
    for y in range(H):
        for x in range(W):
            d = int(disparity[y, x]) & 0xFFFF
            if d <= 0 or d < disparity_scaled_min or d > disparity_scaled_max:
                continue
            ux, uy, parallax = (x - cx)/fx, (y - cy)/fy, d/float(disparity_scale)/fx
            try:
                if rectification_model == 'LENSMODEL_LATLON':
                    r = baseline*math.cos(ux - parallax)/math.sin(parallax)
                    v = (math.sin(ux), math.cos(ux)*math.sin(uy), math.cos(ux)*math.cos(uy))
                else:
                    r = baseline/parallax*math.sqrt(ux*ux + uy*uy + 1.)
                    s = 1./math.sqrt(ux*ux + uy*uy + 1.)
                    v = (ux*s, uy*s, s)
            except (ZeroDivisionError, OverflowError, ValueError):
                continue
            if not (math.isfinite(r) and r > 0):
                continue
            if (range_min is not None and not r >= range_min) or (range_max is not None and not r <= range_max):
                continue
            if image0 is not None:
                with np.errstate(all='ignore'):
                    fix = np.floor(np.float32(map0[y, x, 0]) + np.float32(0.5))
                    fiy = np.floor(np.float32(map0[y, x, 1]) + np.float32(0.5))
                if not (math.isfinite(fix) and math.isfinite(fiy) and 0 <= fix < image0.shape[1] and 0 <= fiy < image0.shape[0]):
                    continue
                color.append(image0[int(fiy), int(fix)])
            p = [r*v[0], r*v[1], r*v[2]]
            if Rt_out_rect0 is not None:
                R, t = Rt_out_rect0[:3], Rt_out_rect0[3]
                p = [float(R[k, 0])*p[0] + float(R[k, 1])*p[1] + float(R[k, 2])*p[2] + float(t[k]) for k in range(3)]
            points.append(p)
            index.append(y*W + x)
    points = np.array(points, dtype=np.float64).reshape(-1, 3)
    if image0 is None: color = None
    else:              color = np.array(color, dtype=image0.dtype).reshape((-1,) + image0.shape[2:])
    return points, color, np.array(index, dtype=np.int32)
