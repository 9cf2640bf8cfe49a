"""The definition of the anti-aliasing Gaussian pre-filter (include/mrcal_amd.h, "smoothing"), restated twice: vectorised
numpy (smooth) and plain loops (smooth_loops). The kernel of csrc/smooth.hip must EQUAL them in every pixel. Also the
taps (weights) and the sigma that 'auto' picks for a map (antialias_sigma). A plain module: the tests import it. No
cv2, and no claim of equality with cv2.GaussianBlur()."""
import math

import numpy as np


def weights(sigma):
    """[w_0, ..., w_R] of one axis, Python ints"""
    if sigma == 0:
        return [256]
    R = math.ceil(3*sigma)
    g = [math.exp(-k*k/(2*sigma*sigma)) for k in range(R + 1)]
    S = g[0] + 2*sum(g[1:])
    a = [256*gk/S for gk in g]
    w = [0]*(R + 1)
    e = 0.0
    for k in range(R, 0, -1):
        w[k] = math.floor(a[k] + e + 0.5)
        e += a[k] - w[k]
    w[0] = 256 - 2*sum(w[1:])
    return w


def _sigmas(sigma):
    return (sigma, sigma) if np.isscalar(sigma) else tuple(sigma)


def smooth(image, sigma):
    """vectorised: the image padded by replication, one shifted slice a tap. uint64 throughout"""
    sx, sy = _sigmas(sigma)
    wx, wy = weights(sx), weights(sy)
    Rx, Ry = len(wx) - 1, len(wy) - 1
    H, W = image.shape
    I = np.pad(image.astype(np.uint64), ((0, 0), (Rx, Rx)), mode='edge')
    T = np.zeros((H, W), dtype=np.uint64)
    for k in range(-Rx, Rx + 1):
        T += np.uint64(wx[abs(k)])*I[:, Rx + k: Rx + k + W]
    T = np.pad(T, ((Ry, Ry), (0, 0)), mode='edge')
    O = np.zeros((H, W), dtype=np.uint64)
    for k in range(-Ry, Ry + 1):
        O += np.uint64(wy[abs(k)])*T[Ry + k: Ry + k + H, :]
    assert int(O.max()) + 32768 < 1 << 32
    return ((O + np.uint64(32768)) >> np.uint64(16)).astype(image.dtype)


def smooth_loops(image, sigma):
    """pixel by pixel, with Python integers and the clamps written out"""
    sx, sy = _sigmas(sigma)
    wx, wy = weights(sx), weights(sy)
    Rx, Ry = len(wx) - 1, len(wy) - 1
    H, W = image.shape
    I = image.tolist()
    T = [[0]*W for _ in range(H)]
    for y in range(H):
        for x in range(W):
            T[y][x] = sum(wx[abs(k)]*I[y][min(max(x + k, 0), W - 1)] for k in range(-Rx, Rx + 1))
    O = np.zeros((H, W), dtype=image.dtype)
    for y in range(H):
        for x in range(W):
            O[y, x] = (sum(wy[abs(k)]*T[min(max(y + k, 0), H - 1)][x] for k in range(-Ry, Ry + 1)) + 32768) >> 16
    return O


def antialias_sigma(mapxy):
    """the sigma 'auto' uses for this map: 0.5 sqrt(s^2 - 1) clipped to 8, 0.0 below 0.5; s: the larger of the medians,
    over every 16th pixel in both directions, of the lengths of map[y,x+1] - map[y,x] and of map[y+1,x] - map[y,x]"""
    H, W = mapxy.shape[:2]
    across, down = [], []
    for y in range(0, H, 16):
        for x in range(0, W, 16):
            here = mapxy[y, x].astype(np.float64)
            if x + 1 < W:
                across.append(float(np.hypot(*(mapxy[y, x + 1].astype(np.float64) - here))))
            if y + 1 < H:
                down.append(float(np.hypot(*(mapxy[y + 1, x].astype(np.float64) - here))))
    medians = []
    for steps in (across, down):
        steps = [s for s in steps if math.isfinite(s)]
        medians.append(float(np.median(steps)) if steps else 0.0)
    s = max(medians)
    if s <= 1.0:
        return 0.0
    sigma = min(0.5*math.sqrt(s*s - 1.0), 8.0)
    return sigma if sigma >= 0.5 else 0.0
