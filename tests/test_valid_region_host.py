"""The host units of the valid-intrinsics region, each driven by a stand-alone program with its own main that is built
with ASan and UBSan, on the CPU: the work lists of the regional statistics (csrc/regional_stats_plan.hpp) and the outline
of a mask (csrc/region_outline.cpp; the definition: include/mrcal_amd.h, "valid-intrinsics region"). The outline is held
vertex for vertex to the border follower of valid_region_checker.py, and to the properties that define it. No GPU here:
the GPU tests are in test_valid_intrinsics_region.py."""
import subprocess

import numpy as np

import hostbuild
import valid_region_checker as chk


def test_regional_stats_plan_under_the_host_sanitizers():
    hostbuild.assert_prints_ok("regional_stats_plan_check")


# --------------------------------------------------------------------------------------------------- host: outline
def named_masks():
    def blank(h=6, w=8): return np.zeros((h, w), dtype=np.uint8)
    masks = {}
    masks["empty"] = blank()
    masks["full"] = np.ones((6, 8), dtype=np.uint8)
    m = blank(); m[2, 3] = 1; masks["one cell"] = m
    m = blank(1, 7); m[0, 1:6] = 1; masks["1xN line"] = m
    m = blank(); m[1:5, 4] = 1; masks["Nx1 line"] = m
    m = blank(); m[2:4, 3:5] = 1; masks["2x2 block"] = m
    m = blank(); m[1:5, 2] = 1; m[4, 2:6] = 1; masks["L"] = m
    m = blank(); m[1:5, 1:7] = 1; m[2:4, 3:5] = 0; masks["ring"] = m
    m = blank(); m[0:2, 0:3] = 1; m[3:5, 4:7] = 1; masks["two equal blobs"] = m
    m = blank(); m[0:2, 0:2] = 1; m[2:4, 2:4] = 1; masks["diagonal touch"] = m
    m = blank(); m[2, :] = 1; m[:, 3] = 1; m[1:4, 2:5] = 1; masks["touches all four edges"] = m
    m = blank(); m[1:4, 1:4] = 1; m[2, 4:7] = 1; masks["blob with a spur"] = m
    m = blank(); m[0, 0] = 1; m[3:5, 3:6] = 1; masks["a cell before the blob"] = m
    m = blank(); m[1, 1] = 1; m[2, 2] = 1; m[1, 3] = 1; masks["V of three"] = m
    rng = np.random.default_rng(20)
    for i in range(200):
        masks[f"random {i}"] = (rng.random((20, 30)) < (0.35 + 0.4*(i % 5)/4.)).astype(np.uint8)
    return masks


def polygon_contains_or_touches(cell, vertices):
    """is the cell centre inside or on the closed polygon of the vertices (integers)"""
    closed = list(vertices) + [vertices[0]]
    x, y = cell
    for e in range(len(closed) - 1):
        (x0, y0), (x1, y1) = closed[e], closed[e + 1]
        if (x1 - x0)*(y - y0) - (y1 - y0)*(x - x0) == 0 and min(x0, x1) <= x <= max(x0, x1) and min(y0, y1) <= y <= max(y0, y1):
            return True
    return chk.inside_exact(x, y, closed)


def check_outline_properties(mask, vertices, a2):
    per_component = chk.outlines(mask)
    if not per_component:
        assert len(vertices) == 0 and a2 == 0
        return
    v = [tuple(int(c) for c in p) for p in vertices]
    chosen = [c for c in per_component if v[0] in c[2]]
    assert len(chosen) == 1
    _, _, member = chosen[0]
    # every vertex is a cell of one component
    assert all(p in member for p in v)
    n = len(v)
    if n > 1:
        steps = []
        for i in range(n):
            dx, dy = v[(i + 1) % n][0] - v[i][0], v[(i + 1) % n][1] - v[i][1]
            # consecutive vertices (the contour is closed: the last goes back to the first) differ along one of the 8 directions
            assert (dx, dy) != (0, 0) and (dx == 0 or dy == 0 or abs(dx) == abs(dy))
            steps.append((np.sign(dx), np.sign(dy)))
        # no vertex is interior to a straight run
        assert all(steps[i - 1] != steps[i] for i in range(n))
    assert chk.area2(v) == a2
    # every cell of the chosen component is inside or on the polygon
    if n >= 2:
        assert all(polygon_contains_or_touches(c, v) for c in member)
    # no other component has a larger area, and an earlier one has a smaller
    for i, (_, other_a2, other_member) in enumerate(per_component):
        assert other_a2 <= a2
        if other_member is member: break
        assert other_a2 < a2
    # the set cells of the other components are none of the chosen component's
    for _, _, other_member in per_component:
        if other_member is not member: assert not (other_member & member)


def test_outline_against_the_checker_and_its_properties(amd, tmp_path):
    from mrcal_amd.valid_region import region_outline, contour_of_mask
    masks = named_masks()
    # the stand-alone program, under the sanitizers
    exe = hostbuild.build_program("valid_region_check")
    path = tmp_path / "masks.txt"
    with open(path, "w") as f:
        for m in masks.values():
            f.write(f"{m.shape[1]} {m.shape[0]} " + " ".join(str(int(c)) for c in m.ravel()) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(masks)
    for (name, m), line in zip(masks.items(), lines):
        numbers = [int(t) for t in line.split()]
        v_exe = np.array(numbers[2:], dtype=np.int32).reshape(-1, 2)
        assert numbers[0] == v_exe.shape[0], name
        v_chk, a2_chk = chk.outline(m)
        v_lib, a2_lib = region_outline(m)
        assert np.array_equal(v_exe, v_chk) and numbers[1] == a2_chk, name
        assert np.array_equal(v_lib, v_chk) and a2_lib == a2_chk, name
        check_outline_properties(m, v_lib, a2_lib)
        assert np.array_equal(contour_of_mask(m, (4000, 2200)), chk.contour_of_mask(m, 4000, 2200)), name

    def vertices(name): return [tuple(p) for p in chk.outline(masks[name])[0].tolist()]
    assert vertices("empty") == []
    assert vertices("full") == [(0, 0), (7, 0), (7, 5), (0, 5)]
    assert vertices("one cell") == [(3, 2)]
    assert vertices("1xN line") == [(1, 0), (5, 0)]
    assert vertices("2x2 block") == [(3, 2), (4, 2), (4, 3), (3, 3)]
    assert vertices("L") == [(2, 1), (2, 3), (3, 4), (5, 4), (2, 4)]                # the inner corner is cut diagonally
    assert vertices("ring") == [(1, 1), (6, 1), (6, 4), (1, 4)]                   # the hole has no part in it
    assert vertices("two equal blobs")[0] == (0, 0)                               # the first in raster order
    assert vertices("a cell before the blob")[0] == (3, 3)                        # the larger area, not the first cell
    assert len(chk.outlines(masks["diagonal touch"])) == 1                        # one component
    assert vertices("blob with a spur") == [(1, 1), (3, 1), (4, 2), (6, 2), (4, 2), (3, 3), (1, 3)]      # out and back
    # empty regions: no cell, one cell, a line (area 0, fewer than 4 points once closed)
    for name in ("empty", "one cell", "1xN line", "Nx1 line"):
        assert contour_of_mask(masks[name], (4000, 2200)).shape == (0, 2), name
    c = contour_of_mask(masks["2x2 block"], (4000, 2200))
    assert c.dtype == np.int32 and c.shape == (5, 2) and np.array_equal(c[0], c[-1])
    # the scaling, and the rounding of a half to even: a 5-wide, 3-high grid over 7 x 4 pixels scales by 1.5 and 1.5
    m = np.zeros((3, 5), dtype=np.uint8); m[0:3, 1:4] = 1
    assert contour_of_mask(m, (7, 4)).tolist() == [[2, 0], [4, 0], [4, 3], [2, 3], [2, 0]]      # 1.5 -> 2, 4.5 -> 4
