"""filter_speckles() restated twice: the definition of include/mrcal_amd.h ("filter_speckles") as a graph (scipy's
connected components over the grid's edges, then a bincount), and cv2.filterSpeckles()'s scan-order flood fill for
CV_16S transcribed as plain Python loops on Python integers, which the graph form is held to. cv2 itself is not used:
"equal to cv2" rests on that transcription.

No file outside the repository is read, and nothing here is shared with the library."""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components


def filter_speckles(disparity, new_value, max_speckle_size, max_diff):
    """-> int16 (H,W), a new array"""
    assert disparity.dtype == np.int16 and disparity.ndim == 2
    H, W = disparity.shape
    v = disparity.astype(np.int64)
    part = v != new_value
    index = np.arange(H*W).reshape(H, W)
    across = part[:, 1:] & part[:, :-1] & (np.abs(v[:, 1:] - v[:, :-1]) <= max_diff)
    down   = part[1:] & part[:-1] & (np.abs(v[1:] - v[:-1]) <= max_diff)
    a = np.concatenate((index[:, 1:][across], index[1:][down]))
    b = np.concatenate((index[:, :-1][across], index[:-1][down]))
    graph = coo_matrix((np.ones(len(a), dtype=np.int8), (a, b)), shape=(H*W, H*W))
    _, component = connected_components(graph, directed=False)
    component = component.reshape(H, W)
    # the pixels that take no part are components of their own in that graph: they are not counted, and not changed
    size = np.bincount(component[part], minlength=H*W)
    out = disparity.copy()
    out[part & (size[component] <= max_speckle_size)] = new_value
    return out


def filter_speckles_loops(disparity, new_value, max_speckle_size, max_diff):
    """cv2's filterSpecklesImpl<short>: a scan in row-major order; an unlabelled pixel starts a flood fill that labels
    its region and counts it; a region of at most max_speckle_size pixels is flagged, and its pixels become new_value
    as the scan reaches them. The image is changed in place while it is scanned, as cv2 does"""
    H, W = disparity.shape
    img = [[int(x) for x in row] for row in disparity]
    labels = [[0]*W for _ in range(H)]
    small = [False]             # per label; 0 is "no label"
    for i in range(H):
        for j in range(W):
            if img[i][j] == new_value: continue
            if labels[i][j]:
                if small[labels[i][j]]: img[i][j] = new_value
                continue
            current = len(small)
            labels[i][j] = current
            stack, count = [(i, j)], 0
            while stack:
                y, x = stack.pop()
                count += 1
                here = img[y][x]
                for yn, xn in ((y + 1, x), (y - 1, x), (y, x + 1), (y, x - 1)):
                    if 0 <= yn < H and 0 <= xn < W and not labels[yn][xn] and img[yn][xn] != new_value \
                       and abs(here - img[yn][xn]) <= max_diff:
                        labels[yn][xn] = current
                        stack.append((yn, xn))
            small.append(count <= max_speckle_size)
            if small[current]: img[i][j] = new_value
    return np.array(img, dtype=np.int16)
