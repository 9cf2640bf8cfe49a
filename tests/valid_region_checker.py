"""CHECKERS for the valid-intrinsics region (include/mrcal_amd.h, "regional statistics" and "valid-intrinsics
region"), in plain numpy and plain loops, written from the header's text. Nothing here is the code under test.
"""
import numpy as np


def grid_height(gridn_width, gridn_height, W, H):
    return int(round(H/W*gridn_width)) if gridn_height is None else gridn_height


def regional_statistics(x, observations_board, indices_frame_camera, icam, W, H, gridn_width, gridn_height):
    """(mean, stdev, count) of camera icam, each (gridn_height,gridn_width): a loop over the cells, every cell asking every
    corner of the camera. x: the measurement vector, the boards first"""
    gridn_height = grid_height(gridn_width, gridn_height, W, H)
    obs = np.asarray(observations_board)
    xb = np.asarray(x)[:obs[..., 0].size*2].reshape(obs.shape[:-1] + (2,))
    keep = obs[..., 2] > 0.0
    keep[np.asarray(indices_frame_camera)[:, 1] != icam] = False
    err, q = xb[keep], obs[keep][:, :2]
    cx = np.linspace(0, W - 1, gridn_width)
    cy = np.linspace(0, H - 1, gridn_height)
    half_w = float(W - 1)/(gridn_width - 1)/2.
    half_h = float(H - 1)/(gridn_height - 1)/2.
    mean  = np.zeros((gridn_height, gridn_width))
    stdev = np.zeros((gridn_height, gridn_width))
    count = np.zeros((gridn_height, gridn_width), dtype=np.int64)
    for j in range(gridn_height):
        for i in range(gridn_width):
            inside = (np.abs(q[:, 0] - cx[i]) < half_w) & (np.abs(q[:, 1] - cy[j]) < half_h)
            v = err[inside].ravel()
            count[j, i] = v.size
            if v.size > 5:
                mean[j, i]  = np.mean(v)
                stdev[j, i] = np.std(v)
    return mean, stdev, count


def mask_rule(uncertainty, mean, stdev, count, thresholds, splined):
    u = np.array(uncertainty)
    u[~np.isfinite(u)] = 1e9
    mask = u < thresholds[0]
    if not splined:
        mask = mask & (mean < thresholds[1]) & (stdev < thresholds[2]) & (count > thresholds[3])
    return mask.astype(np.uint8)


# ------------------------------------------------------------------------------------------------------ the outline
# clockwise on the screen from east: E SE S SW W NW N NE
DIRECTIONS = ((1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1))


def components(mask):
    """labels (H,W), 0 = unset, 1.. in raster order of each component's first cell; 8-connected"""
    m = np.asarray(mask) != 0
    H, W = m.shape
    labels = np.zeros((H, W), dtype=int)
    n = 0
    for y in range(H):
        for x in range(W):
            if not m[y, x] or labels[y, x]: continue
            n += 1
            labels[y, x] = n
            todo = [(x, y)]
            while todo:
                cx, cy = todo.pop()
                for dx, dy in DIRECTIONS:
                    xx, yy = cx + dx, cy + dy
                    if 0 <= xx < W and 0 <= yy < H and m[yy, xx] and not labels[yy, xx]:
                        labels[yy, xx] = n
                        todo.append((xx, yy))
    return labels, n


def border_walk(member, start):
    """the cells of the outer border of a component (member: a set of (x,y)) from its first cell, and the moves"""
    cells, moves = [], []
    cur, look = start, 0
    while True:
        move = None
        for k in range(8):
            d = (look + k) % 8
            if (cur[0] + DIRECTIONS[d][0], cur[1] + DIRECTIONS[d][1]) in member:
                move = d
                break
        if move is None:
            return [cur], []
        if cur == start and moves and move == moves[0]:
            return cells, moves
        cells.append(cur)
        moves.append(move)
        cur = (cur[0] + DIRECTIONS[move][0], cur[1] + DIRECTIONS[move][1])
        look = (move + 5) % 8


def area2(vertices):
    a = 0
    n = len(vertices)
    for i in range(n):
        (x0, y0), (x1, y1) = vertices[i], vertices[(i + 1) % n]
        a += int(x0)*int(y1) - int(x1)*int(y0)
    return abs(a)


def outlines(mask):
    """per component, in raster order: (vertices [(x,y)], twice the area, the set of its cells)"""
    labels, n = components(mask)
    out = []
    for c in range(1, n + 1):
        ys, xs = np.nonzero(labels == c)
        member = set(zip(xs.tolist(), ys.tolist()))
        start = (int(xs[0]), int(ys[0]))                      # np.nonzero is in raster order
        cells, moves = border_walk(member, start)
        if moves:
            vertices = [cells[i] for i in range(len(cells)) if moves[i - 1] != moves[i]]
        else:
            vertices = cells
        out.append((vertices, area2(vertices), member))
    return out


def outline(mask):
    """(vertices (N,2) int32, twice the area) of the component with the largest area, the first among equals"""
    best = None
    for vertices, a2, _ in outlines(mask):
        if best is None or a2 > best[1]:
            best = (vertices, a2)
    if best is None:
        return np.zeros((0, 2), dtype=np.int32), 0
    return np.array(best[0], dtype=np.int32).reshape(-1, 2), best[1]


def contour_of_mask(mask, W, H):
    gh, gw = mask.shape
    v, _ = outline(mask)
    if v.shape[0] == 0: return np.zeros((0, 2))
    c = v.astype(float)
    if np.any(c[0] != c[-1]): c = np.concatenate((c, c[:1]))
    if c.shape[0] < 4: return np.zeros((0, 2))
    c[:, 0] *= float(W - 1)/(gw - 1)
    c[:, 1] *= float(H - 1)/(gh - 1)
    return np.round(c).astype(np.int32)


# ------------------------------------------------------------------------------------------ inside a closed contour
def inside_exact(px, py, vertices):
    """strictly inside by the even-odd rule, in Python's integers: px, py and the vertices are integers"""
    px, py = int(px), int(py)
    inside = False
    for e in range(len(vertices) - 1):
        x0, y0 = int(vertices[e][0]), int(vertices[e][1])
        x1, y1 = int(vertices[e + 1][0]), int(vertices[e + 1][1])
        cross = (x1 - x0)*(py - y0) - (y1 - y0)*(px - x0)
        if cross == 0 and min(x0, x1) <= px <= max(x0, x1) and min(y0, y1) <= py <= max(y0, y1):
            return False                                      # on the border
        if (y0 > py) != (y1 > py):
            if (cross > 0) == (y1 > y0):
                inside = not inside
    return inside


def inside_float(q, vertices):
    """the same for points (N,2) away from every edge, vectorised in double"""
    q = np.asarray(q, dtype=float)
    v = np.asarray(vertices, dtype=float)
    inside = np.zeros(q.shape[0], dtype=bool)
    for e in range(len(v) - 1):
        (x0, y0), (x1, y1) = v[e], v[e + 1]
        cross = (x1 - x0)*(q[:, 1] - y0) - (y1 - y0)*(q[:, 0] - x0)
        crosses = ((y0 > q[:, 1]) != (y1 > q[:, 1])) & ((cross > 0) == (y1 > y0))
        inside ^= crosses
    return inside


def distance_to_edges(q, vertices):
    """the distance of every point (N,2) to the nearest edge"""
    q = np.asarray(q, dtype=float)
    v = np.asarray(vertices, dtype=float)
    best = np.full(q.shape[0], np.inf)
    for e in range(len(v) - 1):
        a, b = v[e], v[e + 1]
        ab = b - a
        L2 = float(ab @ ab)
        t = np.zeros(q.shape[0]) if L2 == 0 else np.clip(((q - a) @ ab)/L2, 0., 1.)
        d = np.linalg.norm(q - (a + t[:, None]*ab), axis=1)
        best = np.minimum(best, d)
    return best
