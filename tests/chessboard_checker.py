"""CHECKER: parts a-d of "chessboard corners" (include/mrcal_amd.h) restated in numpy, and two renderers of boards whose
corners are known analytically. Nothing here is shared with csrc/chessboard.hip."""
import numpy as np

RING = ((5, 0), (5, 2), (3, 3), (2, 5), (0, 5), (-2, 5), (-3, 3), (-5, 2),
        (-5, 0), (-5, -2), (-3, -3), (-2, -5), (0, -5), (2, -5), (3, -3), (5, -2))
STATUS_OK, STATUS_SINGULAR, STATUS_LEFT = 0, 1, 2


def shifted(a, dx, dy):
    """out[y,x] = a[y+dy, x+dx], 0 where that is outside"""
    H, W = a.shape
    out = np.zeros_like(a)
    ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
    xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
    out[yd, xd] = a[ys, xs]
    return out


def blur(image):
    """a: the integer [1 2 1] x [1 2 1] sum (0 outside the image, which no response that is defined reads)"""
    I = image.astype(np.int64)
    rows = shifted(I, -1, 0) + 2*I + shifted(I, 1, 0)
    return shifted(rows, 0, -1) + 2*rows + shifted(rows, 0, 1)


def response(image):
    """b: R (H,W) int32"""
    B = blur(image)
    s = [shifted(B, dx, dy) for dx, dy in RING]
    SR = sum(np.abs((s[n] + s[n+8]) - (s[n+4] + s[n+12])) for n in range(4))
    DR = sum(np.abs(s[n] - s[n+8]) for n in range(8))
    S16 = sum(s)
    S5 = B + shifted(B, 1, 0) + shifted(B, -1, 0) + shifted(B, 0, 1) + shifted(B, 0, -1)
    R = 5*SR - 5*DR - np.abs(5*S16 - 16*S5)
    assert max(np.abs(x).max() for x in (5*SR, 5*DR, 5*S16, 16*S5, R)) < 1 << 27
    H, W = image.shape
    out = np.zeros((H, W), dtype=np.int32)
    out[6:H-6, 6:W-6] = R[6:H-6, 6:W-6]
    return out


def candidates(R, threshold_256=51, nms_radius=7, max_candidates=4096):
    """c: (xy (N,2) int32 in row-major order, overflow)"""
    H, W = R.shape
    Rmax = int(R.max())
    R64 = R.astype(np.int64)
    found = []
    for y, x in np.argwhere((R64 > 0) & (256*R64 > threshold_256*Rmax)):        # (argwhere: row-major)
        v, ok = R64[y, x], True
        for yy in range(max(y - nms_radius, 0), min(y + nms_radius, H - 1) + 1):
            for xx in range(max(x - nms_radius, 0), min(x + nms_radius, W - 1) + 1):
                if (yy, xx) == (y, x): continue
                after = (yy, xx) > (y, x)
                if not (R64[yy, xx] < v or (R64[yy, xx] == v and after)): ok = False
        if ok: found.append((x, y))
    xy = np.array(found, dtype=np.int32).reshape(-1, 2)
    return xy[:max_candidates], len(xy) > max_candidates


def sample(I, x, y):
    """bilinear, the coordinates clamped to the image"""
    H, W = I.shape
    x, y = np.clip(x, 0., W - 1.), np.clip(y, 0., H - 1.)
    x0, y0 = np.floor(x).astype(int), np.floor(y).astype(int)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    fx, fy = x - x0, y - y0
    top    = I[y0, x0]*(1. - fx) + I[y0, x1]*fx
    bottom = I[y1, x0]*(1. - fx) + I[y1, x1]*fx
    return top*(1. - fy) + bottom*fy


def refine(image, xy, iterations=20, stop=1e-5):
    """d: (q (N,2) float64 with NaN where it failed, status (N,) int32, the iterations each took)"""
    I = image.astype(np.float64)
    N = len(xy)
    j, i = (a.ravel().astype(float) for a in np.mgrid[-5:6, -5:6])
    w = np.exp(-(i/5.)**2)*np.exp(-(j/5.)**2)
    start = xy.astype(np.float64)
    q = start.copy()
    status = np.zeros((N,), dtype=np.int32)
    taken = np.zeros((N,), dtype=np.int32)
    live = np.ones((N,), dtype=bool)
    for _ in range(iterations):
        k = np.flatnonzero(live)
        if len(k) == 0: break
        taken[k] += 1
        px, py = q[k, 0, None] + i, q[k, 1, None] + j
        gx = (sample(I, px + 1., py) - sample(I, px - 1., py))/2.
        gy = (sample(I, px, py + 1.) - sample(I, px, py - 1.))/2.
        a, b, c = (w*gx*gx).sum(-1), (w*gx*gy).sum(-1), (w*gy*gy).sum(-1)
        bx, by = (w*gx*gx*i + w*gx*gy*j).sum(-1), (w*gx*gy*i + w*gy*gy*j).sum(-1)
        det, trace = a*c - b*b, a + c
        singular = ~(det > 1e-10*trace*trace)
        with np.errstate(all="ignore"):
            dx, dy = (c*bx - b*by)/det, (a*by - b*bx)/det
        q[k[~singular], 0] += dx[~singular]
        q[k[~singular], 1] += dy[~singular]
        left = ~singular & ~((np.abs(q[k, 0] - start[k, 0]) <= 3.5) & (np.abs(q[k, 1] - start[k, 1]) <= 3.5))
        status[k[singular]] = STATUS_SINGULAR
        status[k[left]] = STATUS_LEFT
        live[k[singular | left | (dx*dx + dy*dy < stop*stop)]] = False
    q[status != STATUS_OK] = np.nan
    return q, status, taken


def detect(image, **params):
    """a-d: (q, response of the candidates, status, overflow, R)"""
    R = response(image)
    xy, overflow = candidates(R, **params)
    q, status, _ = refine(image, xy)
    return q, R[xy[:, 1], xy[:, 0]], status, overflow, R


# ------------------------------------------------------------------------------------------------ the renderers ---
DARK, BRIGHT = 40., 200.


def board_colour(u, v, W, H):
    """the grey level at board coordinates (u,v), a square the unit: the W x H inner corners lie at the integers
    0..W-1 x 0..H-1, the (W+1) x (H+1) squares around them, and everything beyond is as bright as the bright squares"""
    inside = (u > -1.) & (u < W) & (v > -1.) & (v < H)
    dark = (np.floor(u) + np.floor(v)).astype(np.int64) % 2 == 0
    return np.where(inside & dark, DARK, BRIGHT)


def finish_image(levels, noise, seed, dtype):
    """the mean over the supersamples, noise of `noise` grey levels, rounded to the dtype"""
    levels = levels + np.random.default_rng(seed).normal(0., 1., levels.shape)*noise
    if dtype == np.uint16: levels = levels*256.
    return np.clip(np.rint(levels), 0, np.iinfo(dtype).max).astype(dtype)


def supersamples(width, height, n=4):
    """(height,width,n*n,2): the positions of the n x n samples of every pixel; pixel (x,y) is the square around (x,y)"""
    o = (np.arange(n) + 0.5)/n - 0.5
    x = np.arange(width)[None, :, None, None] + o[None, None, None, :]
    y = np.arange(height)[:, None, None, None] + o[None, None, :, None]
    x, y = np.broadcast_arrays(x, y)
    return np.stack((x, y), axis=-1).reshape(height, width, n*n, 2)


def homography(W, H, square, angle_degrees, centre, perspective):
    """board coordinates -> ideal pixels: the board's centre to `centre`, `square` pixels a square there, turned by the
    angle, and the perspective row (per pixel) on top"""
    c, s = np.cos(np.radians(angle_degrees)), np.sin(np.radians(angle_degrees))
    to_centre = np.array(((1., 0., -(W - 1)/2.), (0., 1., -(H - 1)/2.), (0., 0., 1.)))
    similarity = np.array(((square*c, -square*s, 0.), (square*s, square*c, 0.), (0., 0., 1.)))
    persp = np.array(((1., 0., 0.), (0., 1., 0.), (perspective[0], perspective[1], 1.)))
    back = np.array(((1., 0., centre[0]), (0., 1., centre[1]), (0., 0., 1.)))
    return back @ persp @ similarity @ to_centre


def apply_homography(M, p):
    h = p @ M[:2, :2].T + M[:2, 2]
    return h/(p @ M[2, :2] + M[2, 2])[..., None]


def render_numpy(W, H, *, width=800, height=600, square=30., angle=0., centre=None, perspective=(0., 0.), k1=0.,
                 focal=800., noise=0., seed=0, dtype=np.uint8):
    """-> (image, corners (H,W,2)): pure numpy. A pixel q is looked up at the ideal pixel p = c + (q - c)(1 + k1 r^2),
    r = |q - c|/focal, and p on the board through the inverse homography; the true corners come the other way, with
    the radial polynomial inverted by Newton's method"""
    centre = np.array(((width - 1)/2., (height - 1)/2.) if centre is None else centre, dtype=float)
    c = np.array(((width - 1)/2., (height - 1)/2.))
    M = homography(W, H, square, angle, centre, perspective)
    q = supersamples(width, height)
    n = (q - c)/focal
    p = c + focal*n*(1. + k1*(n*n).sum(-1, keepdims=True))
    uv = apply_homography(np.linalg.inv(M), p)
    image = finish_image(board_colour(uv[..., 0], uv[..., 1], W, H).mean(-1), noise, seed, dtype)

    board = np.stack(np.meshgrid(np.arange(W, dtype=float), np.arange(H, dtype=float)), axis=-1)
    nd = (apply_homography(M, board) - c)/focal
    rd = np.sqrt((nd*nd).sum(-1))
    r = rd.copy()
    for _ in range(50):
        r = r - (r*(1. + k1*r*r) - rd)/(1. + 3.*k1*r*r)
    assert np.all(1. + 3.*k1*r*r > 0.1) and np.allclose(r*(1. + k1*r*r), rd, atol=1e-14)
    corners = c + focal*nd*np.where(rd > 0, r/np.where(rd > 0, rd, 1.), 1.)[..., None]
    return image, corners


def render_through_lens(unproject, lensmodel, intrinsics, imagersize, Rt_cam_board_list, W, H, spacing, *, noise=0., seed=0,
                        dtype=np.uint8):
    """-> the images of the board seen from the poses, through `unproject` (the product's, on the GPU): every
    supersample is unprojected ONCE, and each pose intersects the rays with its board plane z = 0. Rt (4,3): R then t,
    board -> camera. The board's corner (i,j) is at (i,j,0) spacing"""
    width, height = imagersize
    q = supersamples(width, height)
    v = unproject(np.ascontiguousarray(q.reshape(-1, 2)), lensmodel, intrinsics).reshape(q.shape[:-1] + (3,))
    images = []
    for k, Rt in enumerate(Rt_cam_board_list):
        R, t = Rt[:3], Rt[3]
        vb, tb = v @ R, t @ R                   # (R^T v and R^T t: the ray and the camera's position, in board coordinates)
        with np.errstate(all="ignore"):
            scale = tb[2]/vb[..., 2]
            p = scale[..., None]*vb - tb
        seen = np.isfinite(scale) & (scale > 0)
        levels = np.where(seen, board_colour(p[..., 0]/spacing, p[..., 1]/spacing, W, H), BRIGHT)
        images.append(finish_image(levels.mean(-1), noise, seed + k, dtype))
    return images
