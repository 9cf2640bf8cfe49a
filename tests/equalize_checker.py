"""The equalization of include/mrcal_amd.h ("equalization"), restated in numpy: CLAHE as OpenCV's clahe.cpp publishes
it, and the stretch of the reference's mrcal_image_uint8_load(). TEST-ONLY.

Two transcriptions that share nothing but the padding's numpy call:
  equalize_clahe(), clahe_luts(), equalize_stretch()     vectorised, np.float32 arrays operation by operation
  equalize_clahe_loops(), equalize_stretch_loops()       plain Python loops, pixel by pixel and bin by bin, np.float32
                                                         scalars: slow, for small images only
cv2 is no part of this project: neither is held to it."""
import numpy as np

f32 = np.float32


def hist_size_of(dtype):
    dtype = np.dtype(dtype)
    if dtype == np.uint8:  return 256
    if dtype == np.uint16: return 65536
    raise Exception(f"equalize(): images are uint8 or uint16, not {dtype}")


def padded(image, tiles):
    """the image as the tiles see it: (padded image, tw, th)"""
    tiles_x, tiles_y = tiles
    if tiles_x < 1 or tiles_y < 1:
        raise Exception(f"equalize(): tiles must be at least (1,1). Got {tiles}")
    H, W = image.shape
    if W % tiles_x == 0 and H % tiles_y == 0:
        return image, W//tiles_x, H//tiles_y
    # BOTH sides, the divisible one by a whole `tiles`
    px, py = tiles_x - W % tiles_x, tiles_y - H % tiles_y
    if px > W - 1 or py > H - 1:
        raise Exception(f"equalize(): an image of {W} x {H} pixels is too small for {tiles} tiles")
    p = np.pad(image, ((0, py), (0, px)), mode='reflect')
    return p, p.shape[1]//tiles_x, p.shape[0]//tiles_y


def clip_of(clip_limit, total, hist_size):
    """None: no clipping"""
    if clip_limit <= 0:
        return None
    return max(int(float(clip_limit)*total/hist_size), 1)


# ---------------------------------------------------------------------------------------------------- vectorised ---
def clahe_luts(image, clip_limit=8.0, tiles=(8, 8)):
    """-> (luts (tiles_y, tiles_x, histSize) of the image's dtype, tw, th, paths): paths counts the tiles in which
    'clipped', 'step>1' (residual > 0 with step > 1), 'step==1' (residual > 0 with step == 1) and 'batch' (batch > 0)
    happen"""
    hist_size = hist_size_of(image.dtype)
    p, tw, th = padded(image, tiles)
    tiles_x, tiles_y = tiles
    total = tw*th
    lut_scale = f32(hist_size - 1) / f32(total)
    clip = clip_of(clip_limit, total, hist_size)
    luts = np.zeros((tiles_y, tiles_x, hist_size), dtype=image.dtype)
    paths = dict.fromkeys(('clipped', 'step>1', 'step==1', 'batch'), 0)
    i = np.arange(hist_size, dtype=np.int64)
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            tile = p[ty*th:(ty + 1)*th, tx*tw:(tx + 1)*tw]
            h = np.bincount(tile.ravel(), minlength=hist_size).astype(np.int64)
            if clip is not None:
                clipped = int(np.maximum(h - clip, 0).sum())
                h = np.minimum(h, clip)
                batch = clipped // hist_size
                residual = clipped - batch*hist_size
                h += batch
                paths['clipped'] += clipped > 0
                paths['batch'] += batch > 0
                if residual > 0:
                    step = max(hist_size // residual, 1)
                    paths['step>1'] += step > 1
                    paths['step==1'] += step == 1
                    h[(i % step == 0) & (i // step < residual)] += 1
            s = np.cumsum(h)
            assert s[-1] == total
            lut = np.rint(s.astype(f32) * lut_scale)            # (float32 x float32, rounded once; rint: halves to even)
            luts[ty, tx] = np.clip(lut, 0, hist_size - 1).astype(image.dtype)
    return luts, tw, th, paths


def _weights(n, size, tiles):
    """for the pixels 0..n-1 along one side: (t1, t2 clamped, the weight of t1, of t2), float32 step by step"""
    inv = f32(1.0) / f32(size)
    tf = np.arange(n).astype(f32) * inv
    tf = tf - f32(0.5)
    t1 = np.floor(tf)
    a = tf - t1
    a1 = f32(1.0) - a
    assert tf.dtype == a.dtype == a1.dtype == np.float32
    t1 = t1.astype(np.int64)
    return np.maximum(t1, 0), np.minimum(t1 + 1, tiles - 1), a1, a


def equalize_clahe(image, clip_limit=8.0, tiles=(8, 8)):
    image = np.asarray(image)
    if image.ndim != 2:
        raise Exception("equalize(): grey images (H,W) only")
    hist_size = hist_size_of(image.dtype)
    luts, tw, th, _ = clahe_luts(image, clip_limit, tiles)
    H, W = image.shape
    tx1, tx2, xa1, xa = _weights(W, tw, tiles[0])
    ty1, ty2, ya1, ya = _weights(H, th, tiles[1])
    L = luts.astype(f32)
    v = image.astype(np.int64)
    Y1, Y2, X1, X2 = ty1[:, None], ty2[:, None], tx1[None, :], tx2[None, :]
    xa1, xa, ya1, ya = xa1[None, :], xa[None, :], ya1[:, None], ya[:, None]
    top = L[Y1, X1, v]*xa1
    top = top + L[Y1, X2, v]*xa
    bottom = L[Y2, X1, v]*xa1
    bottom = bottom + L[Y2, X2, v]*xa
    res = top*ya1
    res = res + bottom*ya
    assert res.dtype == np.float32
    return np.clip(np.rint(res), 0, hist_size - 1).astype(image.dtype)


def equalize_stretch(image):
    image = np.asarray(image)
    if image.ndim != 2:
        raise Exception("equalize(): grey images (H,W) only")
    hist_size_of(image.dtype)
    lo, hi = int(image.min()), int(image.max())
    if hi == lo:
        return np.zeros(image.shape, dtype=np.uint8)
    scaled = (image.astype(np.int64) - lo).astype(f32) * f32(255.)
    scaled = scaled / f32(hi - lo)
    scaled = f32(0.5) + scaled
    assert scaled.dtype == np.float32
    return np.trunc(scaled).astype(np.uint8)


# ------------------------------------------------------------------------------------------- plain Python loops ---
def _round_half_even(x):
    """of a float32 scalar, as an int: Python's round() of the exact value"""
    return int(round(float(x)))


def equalize_clahe_loops(image, clip_limit=8.0, tiles=(8, 8)):
    """clahe.cpp line by line: CLAHE_CalcLut_Body and CLAHE_Interpolation_Body"""
    image = np.asarray(image)
    hist_size = hist_size_of(image.dtype)
    tiles_x, tiles_y = tiles
    H, W = image.shape
    p, tw, th = padded(image, tiles)
    src = p.tolist()
    total = tw*th
    lut_scale = f32(hist_size - 1) / f32(total)
    clip = 0
    if clip_limit > 0.0:
        clip = int(clip_limit*total/hist_size)
        if clip < 1: clip = 1
    luts = []
    for k in range(tiles_x*tiles_y):
        ty, tx = k // tiles_x, k % tiles_x
        hist = [0]*hist_size
        for y in range(ty*th, ty*th + th):
            row = src[y]
            for x in range(tx*tw, tx*tw + tw):
                hist[row[x]] += 1
        if clip > 0:
            clipped = 0
            for i in range(hist_size):
                if hist[i] > clip:
                    clipped += hist[i] - clip
                    hist[i] = clip
            redist_batch = clipped // hist_size
            residual = clipped - redist_batch*hist_size
            for i in range(hist_size):
                hist[i] += redist_batch
            if residual != 0:
                residual_step = max(hist_size // residual, 1)
                i = 0
                while i < hist_size and residual > 0:
                    hist[i] += 1
                    i += residual_step
                    residual -= 1
        lut, s = [0]*hist_size, 0
        for i in range(hist_size):
            if hist[i] == 0 and i > 0:          # (the same sum, the same entry: 65536 bins a tile are mostly empty)
                lut[i] = lut[i-1]
                continue
            s += hist[i]
            lut[i] = min(max(_round_half_even(f32(s)*lut_scale), 0), hist_size - 1)
        luts.append(lut)

    inv_tw, inv_th = f32(1.0)/f32(tw), f32(1.0)/f32(th)
    half, one = f32(0.5), f32(1.0)
    ind1, ind2, xa_, xa1_ = [], [], [], []
    for x in range(W):
        txf = f32(x)*inv_tw - half
        tx1 = int(np.floor(txf))
        tx2 = tx1 + 1
        xa = txf - f32(tx1)
        xa_.append(xa); xa1_.append(one - xa)
        ind1.append(max(tx1, 0)); ind2.append(min(tx2, tiles_x - 1))
    out = np.zeros((H, W), dtype=image.dtype)
    pixels = image.tolist()
    for y in range(H):
        tyf = f32(y)*inv_th - half
        ty1 = int(np.floor(tyf))
        ty2 = ty1 + 1
        ya = tyf - f32(ty1)
        ya1 = one - ya
        ty1, ty2 = max(ty1, 0), min(ty2, tiles_y - 1)
        for x in range(W):
            v = pixels[y][x]
            lut_plane1, lut_plane2 = luts[ty1*tiles_x + ind1[x]], luts[ty1*tiles_x + ind2[x]]
            lut_plane3, lut_plane4 = luts[ty2*tiles_x + ind1[x]], luts[ty2*tiles_x + ind2[x]]
            a = f32(lut_plane1[v])*xa1_[x]
            b = f32(lut_plane2[v])*xa_[x]
            top = a + b
            a = f32(lut_plane3[v])*xa1_[x]
            b = f32(lut_plane4[v])*xa_[x]
            bottom = a + b
            a = top*ya1
            b = bottom*ya
            res = a + b
            assert type(res) is np.float32
            out[y, x] = min(max(_round_half_even(res), 0), hist_size - 1)
    return out


def equalize_stretch_loops(image):
    """image.c: stretch_equalization_uint8_from_uint16(), with the true extremes, and zeros for a constant image"""
    image = np.asarray(image)
    hist_size_of(image.dtype)
    pixels = image.tolist()
    lo, hi = hist_size_of(image.dtype), -1
    for row in pixels:
        for x in row:
            if x < lo: lo = x
            if x > hi: hi = x
    out = np.zeros(image.shape, dtype=np.uint8)
    if hi == lo:
        return out
    span = f32(hi - lo)
    for y, row in enumerate(pixels):
        for x, v in enumerate(row):
            a = f32(v - lo)*f32(255.)
            a = a/span
            a = f32(0.5) + a
            assert type(a) is np.float32
            out[y, x] = int(a)
    return out
