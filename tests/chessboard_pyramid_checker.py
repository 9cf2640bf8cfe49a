"""CHECKER: parts p1-p3 of "chessboard corners" (include/mrcal_amd.h: the image pyramid) restated in numpy on top of
chessboard_checker.py, and the blurred renders the pyramid is there for. Nothing here is shared with
csrc/chessboard.hip. Part e, the lattice, is host code of the product that needs no GPU: it is passed in as `grid`."""
import numpy as np

import chessboard_checker as chk

TAU = 0.3               # CB_DESCENT_AGREEMENT
MIN_SIDE = 32           # CB_MIN_SIDE


def decimate(image):
    """p1: the next level, in integers; an odd last row or column is dropped"""
    H, W = image.shape
    I = image[:H//2*2, :W//2*2].astype(np.int64)
    return ((I[0::2, 0::2] + I[0::2, 1::2] + I[1::2, 0::2] + I[1::2, 1::2] + 2) >> 2).astype(image.dtype)


def level_shape(shape, level):
    H, W = shape
    for _ in range(level):
        H, W = H//2, W//2
    return H, W


def max_levels(shape):
    """the largest pyramid_levels an image of this (H,W) allows"""
    n = 0
    while min(level_shape(shape, n + 1)) >= MIN_SIDE:
        n += 1
    return n


def pyramid(image, n):
    """levels 0..n"""
    assert n <= max_levels(image.shape)
    levels = [image]
    for _ in range(n):
        levels.append(decimate(levels[-1]))
    return levels


def up(q, times=1):
    """a point of level l + times in the pixels of level l"""
    for _ in range(times):
        q = 2.*q + 0.5
    return q


def detect_level(image, grid, W, H, **params):
    """parts a-e on one image: (board (H,W,2) or None, R, xy)"""
    R = chk.response(image)
    xy, _ = chk.candidates(R, **params)
    q, status, _ = chk.refine(image, xy)
    board = grid(q, W, H, response=R[xy[:, 1], xy[:, 0]], status=status) if len(xy) else None
    return board, R, xy


def detect_pyramid(image, W, H, n, grid, tau=TAU, **params):
    """p2 and p3 -> None, or a dict:
         corners (H,W,2) in level-0 pixels; levels (H,W) int32; detection_level; images: the levels; tried: {L: (R, xy)};
         disagreement: [(level the step went to, corner index, max(|dx|,|dy|) or NaN where the refinement failed)]"""
    images = pyramid(image, n)
    tried, board = {}, None
    for L in range(n, -1, -1):
        board, R, xy = detect_level(images[L], grid, W, H, **params)
        tried[L] = (R, xy)
        if board is not None: break
    if board is None:
        return None
    q = board.reshape(-1, 2).copy()
    level = np.full((len(q),), L, dtype=np.int32)
    disagreement = []
    for l in range(L - 1, -1, -1):
        k = np.flatnonzero(level == l + 1)
        if len(k) == 0: break
        start = up(q[k])
        refined, status, _ = chk.refine(images[l], start)
        with np.errstate(invalid="ignore"):
            delta = np.abs(refined - start).max(-1)
        disagreement += [(l, int(c), float(d)) for c, d in zip(k, delta)]
        ok = (status == chk.STATUS_OK) & (delta <= tau)
        q[k[ok]] = refined[ok]
        level[k[ok]] = l
    corners = q.copy()
    for l in range(1, L + 1):
        corners[level >= l] = up(corners[level >= l])
    return dict(corners=corners.reshape(H, W, 2), levels=level.reshape(H, W), detection_level=L, images=images,
                tried=tried, disagreement=disagreement)


# ------------------------------------------------------------------------------------------------ blurred renders ---
def gaussian_blur(image, sigma):
    """a separable Gaussian of sigma px on the rounded image, the border pixels repeated, rounded to the dtype again"""
    if sigma <= 0: return image
    r = int(np.ceil(4*sigma))
    k = np.exp(-0.5*(np.arange(-r, r + 1)/sigma)**2)
    k /= k.sum()
    I = np.pad(image.astype(np.float64), r, mode="edge")
    I = sum(k[i]*I[:, i:i + image.shape[1]] for i in range(2*r + 1))
    I = sum(k[i]*I[i:i + image.shape[0], :] for i in range(2*r + 1))
    return np.clip(np.rint(I), 0, np.iinfo(image.dtype).max).astype(image.dtype)


BOARD = (7, 5)
SIZES = {30: (480, 400), 60: (800, 640), 110: (1200, 900)}            # the square -> (width, height) of the image
SWEEP = tuple((sigma, square) for square in (30, 60) for sigma in (0., 1.5, 3., 4., 6.)) + ((0., 110), (6., 110))


def blurred_render(sigma, square, seed=None, dtype=np.uint8, angle=17., size=None):
    """-> (image, true corners (5,7,2)): a 7 x 5 board turned by 17 degrees with a slight perspective, noise of 1 grey
    level, then the blur. The seed of a case of the sweep is its place in it, from 1"""
    width, height = SIZES[square] if size is None else size
    seed = SWEEP.index((sigma, square)) + 1 if seed is None else seed
    image, truth = chk.render_numpy(*BOARD, width=width, height=height, square=float(square), angle=angle,
                                    perspective=(4e-5, -3e-5), noise=1., seed=seed, dtype=dtype)
    return gaussian_blur(image, sigma), truth


def cluttered_render():
    """the 60 px board of the sweep, blurred by 1.5 px, with things beside it that are no part of a board: single
    X corners (2 x 2 squares of 12 and of 40 px: the larger ones are candidates at the coarse levels too), dark
    rectangles and a patch of noise, in the margins the board leaves"""
    image, truth = chk.render_numpy(*BOARD, width=800, height=640, square=60., angle=17., perspective=(4e-5, -3e-5), noise=1., seed=40)
    rng = np.random.default_rng(41)
    for cx, cy, n in ((40, 80, 12), (760, 560, 12), (150, 610, 12), (60, 560, 40), (740, 80, 40)):
        image[cy - n:cy, cx - n:cx] = 40; image[cy:cy + n, cx:cx + n] = 40
    for x, y, w, h in ((700, 30, 60, 25), (20, 300, 30, 70), (730, 250, 40, 40)):
        image[y:y + h, x:x + w] = 70
    image[10:60, 300:420] = rng.integers(0, 256, size=(50, 120)).astype(np.uint8)
    return gaussian_blur(image, 1.5), truth
