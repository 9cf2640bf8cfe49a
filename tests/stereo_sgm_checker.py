"""stereo_matching_sgm() restated: the six steps of include/mrcal_amd.h ("stereo_matching_sgm") in numpy on int64, and
once more as plain per-pixel, per-disparity Python loops that the numpy form is held to on a tiny volume.

The numpy form: the census by shifted comparisons of the edge-padded image, the recurrence vectorised over everything
but the path's own axis, the selection by argmin (which returns the first minimum). No file outside the repository is
read, and nothing here is shared with the library."""
import numpy as np

SCALE = 16
RX, RY = 4, 3               # the census window: 9 wide, 7 tall
COST_OUTSIDE = 62
NO_PART = 1 << 20           # what a neighbour that takes no part holds: larger than any L + P2
# (dx,dy); the first four are paths = 4
DIRECTIONS = ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, 1), (1, -1), (-1, -1))

_POPCOUNT8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.int64)


def popcount(a):
    """of every uint64 of a"""
    return _POPCOUNT8[np.ascontiguousarray(a).view(np.uint8).reshape(a.shape + (8,))].sum(axis=-1)


def census(image):
    """uint64 (H,W): bit = neighbour < centre over the window, the centre left out, coordinates clamped"""
    H, W = image.shape
    padded = np.pad(image.astype(np.int64), ((RY, RY), (RX, RX)), mode="edge")
    out = np.zeros((H, W), dtype=np.uint64)
    for dy in range(2*RY + 1):
        for dx in range(2*RX + 1):
            if dy == RY and dx == RX: continue
            out = (out << np.uint64(1)) | (padded[dy:dy + H, dx:dx + W] < image).astype(np.uint64)
    return out


def cost_volume(census0, census1, disparity_min, D):
    """int64 (H,W,D)"""
    H, W = census0.shape
    C = np.full((H, W, D), COST_OUTSIDE, dtype=np.int64)
    x = np.arange(W)
    for i in range(D):
        xr = x - (disparity_min + i)
        inside = (xr >= 0) & (xr < W)
        if inside.any():
            C[:, inside, i] = popcount(census0[:, inside] ^ census1[:, xr[inside]])
    return C


def _step(C, before, P1, P2):
    """one step of the recurrence for any number of paths at once: C, before (...,D)"""
    m = before.min(axis=-1, keepdims=True)
    pad = np.full(before.shape[:-1] + (1,), NO_PART, dtype=np.int64)
    down = np.concatenate((pad, before[..., :-1]), axis=-1) + P1
    up   = np.concatenate((before[..., 1:], pad), axis=-1) + P1
    return C + np.minimum(np.minimum(before, m + P2), np.minimum(down, up)) - m


def aggregate(C, P1, P2, paths):
    """S = sum over the directions of L_r: int64 (H,W,D)"""
    H, W, D = C.shape
    S = np.zeros_like(C)
    for dx, dy in DIRECTIONS[:paths]:
        L = np.empty_like(C)
        if dy == 0:
            xs = range(W) if dx > 0 else range(W - 1, -1, -1)
            for n, x in enumerate(xs):
                L[:, x] = C[:, x] if n == 0 else _step(C[:, x], L[:, x - dx], P1, P2)
        else:
            ys = range(H) if dy > 0 else range(H - 1, -1, -1)
            for n, y in enumerate(ys):
                if n == 0:
                    L[y] = C[y]
                    continue
                before = L[y - dy]
                if dx == 0:
                    L[y] = _step(C[y], before, P1, P2)
                elif dx > 0:        # the predecessor of x is x - 1: x = 0 has none
                    L[y, 0]  = C[y, 0]
                    L[y, 1:] = _step(C[y, 1:], before[:-1], P1, P2)
                else:
                    L[y, -1]  = C[y, -1]
                    L[y, :-1] = _step(C[y, :-1], before[1:], P1, P2)
        S += L
    return S


def select(S, disparity_min, uniqueness_ratio, disp12_max_diff):
    """-> disparity int16 (H,W), and the intermediates"""
    H, W, D = S.shape
    istar = S.argmin(axis=-1)                   # (the first of equal minima)
    smin  = np.take_along_axis(S, istar[..., None], axis=-1)[..., 0]
    i = np.arange(D)
    far = np.abs(i - istar[..., None]) > 1
    unique = ~(far & (S*(100 - uniqueness_ratio) < smin[..., None]*100)).any(axis=-1)
    inner = (istar > 0) & (istar < D - 1)
    a = np.take_along_axis(S, np.clip(istar - 1, 0, D - 1)[..., None], axis=-1)[..., 0]
    c = np.take_along_axis(S, np.clip(istar + 1, 0, D - 1)[..., None], axis=-1)[..., 0]
    den = np.maximum(a + c - 2*smin, 1)
    numerator = (a - c)*SCALE + den
    scaled = SCALE*istar + np.where(inner, numerator // (2*den), 0)        # (// is a floor)

    # the right image: T(y,x1,i) = S(y, x1 + d, i)
    x = np.arange(W)
    T = np.full_like(S, np.iinfo(np.int64).max)
    for k in range(D):
        xl = x + disparity_min + k
        inside = (xl >= 0) & (xl < W)
        if inside.any(): T[:, inside, k] = S[:, xl[inside], k]
    iright = T.argmin(axis=-1)

    valid = unique.copy()
    if disp12_max_diff >= 0:
        x1 = x[np.newaxis, :] - (disparity_min + istar)
        inside = (x1 >= 0) & (x1 < W)
        i1 = np.take_along_axis(iright, np.clip(x1, 0, W - 1), axis=1)
        valid &= inside & (np.abs(i1 - istar) <= disp12_max_diff)
    disparity = np.where(valid, SCALE*disparity_min + scaled, SCALE*(disparity_min - 1)).astype(np.int16)
    return disparity, dict(istar=istar, iright=iright, unique=unique, inner=inner, numerator=numerator, den=den, valid=valid)


def stereo_matching_sgm(image0, image1, *, disparity_min=0, disparity_max, P1=10, P2=120, paths=8, uniqueness_ratio=10,
                        disp12_max_diff=1, intermediates=False):
    D = disparity_max - disparity_min
    C = cost_volume(census(image0), census(image1), disparity_min, D)
    S = aggregate(C, P1, P2, paths)
    disparity, inter = select(S, disparity_min, uniqueness_ratio, disp12_max_diff)
    if intermediates:
        inter["S"] = S
        return disparity, inter
    return disparity


# ------------------------------------------------------------------------------------------------- plain loops ---
def stereo_matching_sgm_loops(image0, image1, *, disparity_min=0, disparity_max, P1=10, P2=120, paths=8,
                              uniqueness_ratio=10, disp12_max_diff=1):
    """the definition, a pixel and a disparity at a time, in Python integers"""
    H, W = image0.shape
    D = disparity_max - disparity_min
    im = [[[int(v) for v in row] for row in image] for image in (image0, image1)]

    def census_at(image, y, x):
        bits = []
        for dy in range(-RY, RY + 1):
            for dx in range(-RX, RX + 1):
                if dy == 0 and dx == 0: continue
                yy, xx = min(max(y + dy, 0), H - 1), min(max(x + dx, 0), W - 1)
                bits.append(image[yy][xx] < image[y][x])
        return bits
    cen = [[[census_at(image, y, x) for x in range(W)] for y in range(H)] for image in im]

    def cost(y, x, i):
        xr = x - (disparity_min + i)
        if xr < 0 or xr >= W: return COST_OUTSIDE
        return sum(1 for b0, b1 in zip(cen[0][y][x], cen[1][y][xr]) if b0 != b1)

    S = [[[0]*D for x in range(W)] for y in range(H)]
    for dx, dy in DIRECTIONS[:paths]:
        L = [[None]*W for y in range(H)]
        for y in (range(H) if dy >= 0 else range(H - 1, -1, -1)):
            for x in (range(W) if dx >= 0 else range(W - 1, -1, -1)):
                yb, xb = y - dy, x - dx
                if yb < 0 or yb >= H or xb < 0 or xb >= W:
                    L[y][x] = [cost(y, x, i) for i in range(D)]
                    continue
                before = L[yb][xb]
                m = min(before)
                now = []
                for i in range(D):
                    candidates = [before[i], m + P2]
                    if i - 1 >= 0: candidates.append(before[i - 1] + P1)
                    if i + 1 < D:  candidates.append(before[i + 1] + P1)
                    now.append(cost(y, x, i) + min(candidates) - m)
                L[y][x] = now
        for y in range(H):
            for x in range(W):
                for i in range(D): S[y][x][i] += L[y][x][i]

    def first_minimum(values):
        best = None
        for i, v in values:
            if best is None or v < best[1]: best = (i, v)
        return best

    out = np.zeros((H, W), dtype=np.int16)
    for y in range(H):
        for x in range(W):
            s = S[y][x]
            istar, smin = first_minimum(enumerate(s))
            valid = not any(abs(i - istar) > 1 and s[i]*(100 - uniqueness_ratio) < smin*100 for i in range(D))
            scaled = SCALE*istar
            if 0 < istar < D - 1:
                a, c = s[istar - 1], s[istar + 1]
                den = max(a + c - 2*smin, 1)
                scaled += ((a - c)*SCALE + den) // (2*den)      # (Python's // is a floor)
            if valid and disp12_max_diff >= 0:
                x1 = x - (disparity_min + istar)
                if x1 < 0 or x1 >= W: valid = False
                else:
                    i1, _ = first_minimum((i, S[y][x1 + disparity_min + i][i]) for i in range(D)
                                          if 0 <= x1 + disparity_min + i < W)
                    valid = abs(i1 - istar) <= disp12_max_diff
            out[y, x] = SCALE*disparity_min + scaled if valid else SCALE*(disparity_min - 1)
    return out
