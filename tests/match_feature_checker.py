"""CHECKER for match_feature(): numpy written for the tests, following the definition of a match in
include/mrcal_amd.h ("match_feature"), not the product's code. The window sums of integer images are exact integers
(int64 sliding sums by cumulative sums); those of float images are double. The six formulas are evaluated in double in
the order the definition gives and rounded to float32. The subpixel step is the reference's own: numpy.linalg.lstsq
on the 3x3 entries around the optimum. No cv2."""
import numpy as np

TM_SQDIFF, TM_SQDIFF_NORMED, TM_CCORR, TM_CCORR_NORMED, TM_CCOEFF, TM_CCOEFF_NORMED = range(6)
METHODS = (TM_SQDIFF, TM_SQDIFF_NORMED, TM_CCORR, TM_CCORR_NORMED, TM_CCOEFF, TM_CCOEFF_NORMED)


def apply_homography(H, q):
    q = np.asarray(q, dtype=float)
    x, y = q[..., 0], q[..., 1]
    d = (H[2, 0]*x + H[2, 1]*y) + H[2, 2]
    return np.stack((((H[0, 0]*x + H[0, 1]*y) + H[0, 2])/d, ((H[1, 0]*x + H[1, 1]*y) + H[1, 2])/d), axis=-1)


def pixel_grid(x0, y0, w, h):
    """(h,w,2): the integer pixels (x0..x0+w-1, y0..y0+h-1), in double"""
    return np.stack(np.meshgrid(np.arange(x0, x0 + w, dtype=float), np.arange(y0, y0 + h, dtype=float)), axis=-1)


def remap(image, mapxy):
    """bilinear, 0 outside, in float32 as transform_image() defines it; integers rounded to nearest (halves to even)"""
    H, W = image.shape
    m = mapxy.astype(np.float32)
    x, y = m[..., 0], m[..., 1]
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = (x - x0).astype(np.float32), (y - y0).astype(np.float32)
    ix, iy = x0.astype(np.int64), y0.astype(np.int64)
    def at(iy, ix):
        inside = (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)
        return np.where(inside, image[np.clip(iy, 0, H-1), np.clip(ix, 0, W-1)], 0).astype(np.float32)
    one = np.float32(1)
    v = (one - fy)*((one - fx)*at(iy, ix) + fx*at(iy, ix+1)) + fy*((one - fx)*at(iy+1, ix) + fx*at(iy+1, ix+1))
    v = np.where((fx == 0) & (fy == 0), at(iy, ix), v)
    if image.dtype == np.float32: return v.astype(np.float32)
    return np.clip(np.rint(v), 0, np.iinfo(image.dtype).max).astype(image.dtype)


def window_sums(a, tw, th):
    """the sum of a over every (th,tw) window: (H-th+1, W-tw+1), in a's dtype (int64: exact)"""
    c = np.zeros((a.shape[0] + 1, a.shape[1] + 1), dtype=a.dtype)
    c[1:, 1:] = np.cumsum(np.cumsum(a, axis=0), axis=1)
    return c[th:, tw:] - c[:-th, tw:] - c[th:, :-tw] + c[:-th, :-tw]


def sums(cut, template):
    """IT, SI, SI2 (arrays over the surface), ST, ST2, N: int64 for integer images, double otherwise"""
    th, tw = template.shape
    acc = np.int64 if cut.dtype.kind == 'u' else np.float64
    I, T = cut.astype(acc), template.astype(acc)
    oh, ow = cut.shape[0] - th + 1, cut.shape[1] - tw + 1
    IT, SI, SI2 = (np.zeros((oh, ow), dtype=acc) for i in range(3))
    # (doubles: row by row, left to right, the fixed order of the definition; cumulative sums of doubles would cancel)
    for dy in range(th):
        for dx in range(tw):
            w = I[dy:dy+oh, dx:dx+ow]
            IT += w*T[dy, dx]
            if acc is np.float64:
                SI  += w
                SI2 += w*w
    if acc is np.int64:
        SI, SI2 = window_sums(I, tw, th), window_sums(I*I, tw, th)
    return IT, SI, SI2, T.sum(), (T*T).sum(), tw*th


def score(method, IT, SI, SI2, ST, ST2, N):
    """the formula in double, rounded to float32"""
    IT, SI, SI2 = (np.asarray(a, dtype=np.float64) for a in (IT, SI, SI2))
    ST, ST2, N = float(ST), float(ST2), float(N)
    with np.errstate(divide="ignore", invalid="ignore"):
        if method == TM_CCORR:
            z = IT
        elif method in (TM_SQDIFF, TM_SQDIFF_NORMED):
            z = (SI2 - 2.*IT) + ST2
            if method == TM_SQDIFF_NORMED:
                den = np.sqrt(SI2*ST2)
                z = np.where(den > 0, z/den, 1.)
        elif method == TM_CCORR_NORMED:
            den = np.sqrt(SI2*ST2)
            z = np.where(den > 0, IT/den, 0.)
        else:
            z = IT - SI*ST/N
            if method == TM_CCOEFF_NORMED:
                den = np.sqrt(np.maximum(SI2 - SI*SI/N, 0.)*max(ST2 - ST*ST/N, 0.))
                z = np.where(den > 0, z/den, 0.)
    return z.astype(np.float32)


def matchoutput(cut, template, method):
    return score(method, *sums(cut, template))


def matchoutput_bruteforce(cut, template, method):
    """the same by a double loop over the surface: for the checker's own test"""
    th, tw = template.shape
    oh, ow = cut.shape[0] - th + 1, cut.shape[1] - tw + 1
    z = np.zeros((oh, ow), dtype=np.float32)
    T = template.astype(float)
    for y in range(oh):
        for x in range(ow):
            I = cut[y:y+th, x:x+tw].astype(float)
            z[y, x] = score(method, (I*T).sum(), I.sum(), (I*I).sum(), T.sum(), (T*T).sum(), tw*th)
    return z


def optimum(z, method):
    """(ox, oy): the first optimum in row-major order"""
    i = np.argmin(z.ravel()) if method in (TM_SQDIFF, TM_SQDIFF_NORMED) else np.argmax(z.ravel())
    oy, ox = np.unravel_index(i, z.shape)
    return int(ox), int(oy)


def subpixel(z, ox, oy):
    """the reference's step: (x, y, value) of the stationary point of the least-squares quadric, relative to (ox,oy);
    None on the edge"""
    if ox <= 0 or oy <= 0 or ox >= z.shape[1] - 1 or oy >= z.shape[0] - 1: return None
    x, y = np.meshgrid(np.arange(3) - 1., np.arange(3) - 1.)
    x, y = x.ravel(), y.ravel()
    M = np.stack((np.ones(9), x, y, x*x, x*y, y*y), axis=-1)
    c00, c10, c01, c20, c11, c02 = np.linalg.lstsq(M, z[oy-1:oy+2, ox-1:ox+2].ravel().astype(float), rcond=None)[0]
    det = 4.*c20*c02 - c11*c11
    x, y = -np.array((2.*c10*c02 - c01*c11, 2.*c01*c20 - c10*c11))/det
    return x, y, c00 + c10*x + c01*y + c20*x*x + c11*x*y + c02*y*y


def window(q1e, ts, radius, shape1):
    """steps 1 and 3: tmin (x,y), qmin (x,y), qmax (x,y) as integer arrays; None if the template is outside image1"""
    ts = np.asarray(ts)
    tmin = np.round(np.asarray(q1e, dtype=float) - (ts - 1.)/2.).astype(int)
    tmax = tmin + ts - 1
    size = np.array((shape1[1], shape1[0]))
    if np.any(tmin < 0) or np.any(tmax >= size): return None
    return tmin, np.maximum(tmin - radius, 0), np.minimum(tmin + radius + ts - 1, size - 1)


def template_map(H01, tmin, ts):
    """step 2: (th,tw,2) float32"""
    return apply_homography(H01, pixel_grid(tmin[0], tmin[1], ts[0], ts[1])).astype(np.float32)


def match(image0, image1, q0, H10, ts, radius, method, template=None):
    """the whole definition: (q1 or None, dict(matchoutput_image, template, optimum, qshift))"""
    q1e = apply_homography(H10, q0)
    tmin, qmin, qmax = window(q1e, ts, radius, image1.shape)
    if template is None:
        template = remap(image0, template_map(np.linalg.inv(H10), tmin, ts))
    z = matchoutput(image1[qmin[1]:qmax[1]+1, qmin[0]:qmax[0]+1], template, method)
    ox, oy = optimum(z, method)
    d = dict(matchoutput_image=z, template=template, optimum=(ox, oy), qshift=qmin + q1e - tmin)
    s = subpixel(z, ox, oy)
    if s is None: return None, d
    return np.array((ox + s[0], oy + s[1])) + d['qshift'], d
