"""plan_gen_rows() and make_dest_lists() (csrc/solver_plan.cpp) - the host functions that decide which row adds to which
entry of the normal equations, and in which order - checked on the CPU through their dev exports: no GPU needed.

The returned plan is EXECUTED here the way GenPlan documents it (solver_kernels.hpp): a chunk's partial sums are
[pairs p <= q row-major | k sums s x | sum x^2] over the chunk's rows, a destination adds its (group << 10 | position)
sources over the group's chunks. Every nonzero and every x is a small integer, so all sums are exact and the result must
EQUAL the camera-block part of J^T J, J^T x and x^T x computed densely by numpy."""
import ctypes as C
import os
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN_CHUNK, GEN_KMAX = 128, 40
LISTS = ("rows", "chunk_begin", "chunk_group", "group_k", "group_off", "spos", "scol", "dest_id", "dest_begin", "dest_src",
         "group_chunk_begin", "eb_block", "eb_begin", "eb_rows", "eb_group", "eb_epos")
COUNTS = ("Nrows", "Nchunks", "Ngroups", "stride", "kmax", "Ndest", "Neblocks")


@pytest.fixture(scope="module")
def lib():
    lib = C.CDLL(os.path.join(ROOT, "mrcal_amd", "libmrcal_amd.so"))
    pi = C.POINTER(C.c_int)
    lib.mrcal_amd_debug_plan_gen_rows.restype  = C.c_int
    lib.mrcal_amd_debug_plan_gen_rows.argtypes = [C.c_int]*5 + [pi, pi, pi, C.c_int]
    lib.mrcal_amd_debug_dest_lists.restype  = C.c_int
    lib.mrcal_amd_debug_dest_lists.argtypes = [C.c_int, pi, pi, pi, C.c_int]
    return lib


def as_ints(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    if a.size == 0: a = np.zeros(1, dtype=np.int32)
    return a, a.ctypes.data_as(C.POINTER(C.c_int))


def read_lists(out, names):
    """[count | entries] list after list"""
    d, at = {}, 0
    for name in names:
        n = int(out[at])
        d[name] = out[at + 1:at + 1 + n].copy()
        at += 1 + n
    assert at == len(out)
    return d


class State:
    """the frames partition of a state [Nshared intrinsics + extrinsics | Nfb frames | Npb points | Nwarp]"""
    def __init__(self, Nshared, Nfb, Npb, Nwarp):
        self.Nshared, self.Nfb, self.Npb, self.Nwarp = Nshared, Nfb, Npb, Nwarp
        self.NE     = 6*Nfb + 3*Npb
        self.Nc     = Nshared + Nwarp
        self.Nstate = Nshared + self.NE + Nwarp
    def frame(self, i): return [self.Nshared + 6*i + k for k in range(6)]
    def point(self, i): return [self.Nshared + 6*self.Nfb + 3*i + k for k in range(3)]
    def warp(self):     return [self.Nshared + self.NE + k for k in range(self.Nwarp)]
    def S_index(self, col):
        """state column -> camera-block index, None for a column of an eliminated block"""
        if col < self.Nshared: return col
        if col >= self.Nshared + self.NE: return col - self.NE
        return None
    def block_of(self, col):
        """(block index, its first state column, its size) of an eliminated column"""
        e = col - self.Nshared
        if e < 6*self.Nfb: return e//6, self.Nshared + 6*(e//6), 6
        i = (e - 6*self.Nfb)//3
        return self.Nfb + i, self.Nshared + 6*self.Nfb + 3*i, 3


def plan_gen_rows(lib, st, rows):
    rowptr, prowptr = as_ints(np.concatenate(([0], np.cumsum([len(r) for r in rows]))) + 7)   # (a slice: rowptr[0] != 0)
    colidx, pcolidx = as_ints([c for r in rows for c in r])
    out = np.zeros(1 << 16, dtype=np.int32)
    pout = out.ctypes.data_as(C.POINTER(C.c_int))
    n = lib.mrcal_amd_debug_plan_gen_rows(st.Nshared, st.Nfb, st.Npb, st.Nwarp, len(rows), prowptr, pcolidx, pout, 3)
    assert n > 3 and not out.any()                                         # (too small a buffer: nothing is written)
    n = lib.mrcal_amd_debug_plan_gen_rows(st.Nshared, st.Nfb, st.Npb, st.Nwarp, len(rows), prowptr, pcolidx, pout, len(out))
    assert n <= len(out)
    G = dict(zip(COUNTS, (int(v) for v in out[:len(COUNTS)])))
    G.update(read_lists(out[len(COUNTS):n], LISTS))
    return G


def check_plan(st, rows, G, rng):
    """the invariants of a plan, then its execution against numpy"""
    Nrows, Nc = len(rows), st.Nc
    assert G["Nrows"] == Nrows > 0
    assert G["Nchunks"] == len(G["chunk_group"]) == len(G["chunk_begin"]) - 1
    assert G["Ngroups"] == len(G["group_k"]) == len(G["group_off"]) == len(G["group_chunk_begin"]) - 1
    assert G["Ndest"] == len(G["dest_id"]) == len(G["dest_begin"]) - 1 and len(G["dest_src"]) == G["dest_begin"][-1]
    assert G["Neblocks"] == len(G["eb_block"]) == len(G["eb_begin"]) - 1
    assert len(G["eb_rows"]) == len(G["eb_group"]) == len(G["eb_epos"]) == G["eb_begin"][-1]
    # a row's signature, worked out here: (positions of its camera-block columns, their camera-block indices)
    def signature(r):
        cam = [(p, st.S_index(c)) for p, c in enumerate(rows[r]) if st.S_index(c) is not None]
        return tuple(p for p, s in cam), tuple(s for p, s in cam)
    kmax = max(len(signature(r)[0]) for r in range(Nrows))
    assert G["kmax"] == kmax and G["stride"] == kmax*(kmax + 1)//2 + kmax + 1
    group_sig = [(tuple(G["spos"][o:o + k]), tuple(G["scol"][o:o + k])) for k, o in zip(G["group_k"], G["group_off"])]
    assert len(set(group_sig)) == G["Ngroups"] == len(set(signature(r) for r in range(Nrows)))
    # every row once; chunks of at most GEN_CHUNK rows of ONE group; a group's chunks contiguous, its rows in row order;
    # the groups numbered as they first appear
    assert sorted(G["rows"]) == list(range(Nrows))
    assert G["chunk_begin"][0] == 0 and G["chunk_begin"][-1] == Nrows
    row_group = {}
    for c in range(G["Nchunks"]):
        b, e = G["chunk_begin"][c], G["chunk_begin"][c + 1]
        assert 0 < e - b <= GEN_CHUNK
        for r in G["rows"][b:e]:
            assert signature(r) == group_sig[G["chunk_group"][c]]
            row_group[int(r)] = int(G["chunk_group"][c])
    first = []
    for g in range(G["Ngroups"]):
        cb, ce = G["group_chunk_begin"][g], G["group_chunk_begin"][g + 1]
        assert cb < ce and all(G["chunk_group"][c] == g for c in range(cb, ce))
        rg = G["rows"][G["chunk_begin"][cb]:G["chunk_begin"][ce]]
        assert np.all(np.diff(rg) > 0)
        # (whole chunks but the group's last)
        assert all(G["chunk_begin"][c + 1] - G["chunk_begin"][c] == GEN_CHUNK for c in range(cb, ce - 1))
        first.append(rg[0])
    assert first == sorted(first)
    assert G["group_chunk_begin"][0] == 0 and G["group_chunk_begin"][-1] == G["Nchunks"]
    # the eliminated blocks: every row that touches one is in its list once, in row order
    expect = {}
    for r in range(Nrows):
        e = [(p, c) for p, c in enumerate(rows[r]) if st.S_index(c) is None]
        if not e: continue
        blk, c0, de = st.block_of(e[0][1])
        assert [c for p, c in e] == list(range(c0, c0 + de))              # (the test's own rows: one whole block)
        expect.setdefault(blk, []).append((r, row_group[r], e[0][0]))
    assert list(G["eb_block"]) == sorted(expect)
    for i, blk in enumerate(G["eb_block"]):
        b, e = G["eb_begin"][i], G["eb_begin"][i + 1]
        assert list(zip(G["eb_rows"][b:e], G["eb_group"][b:e], G["eb_epos"][b:e])) == expect[blk]
    # the finalize lists: destinations in increasing order, each one's sources in (group, position) order
    assert np.all(np.diff(G["dest_id"]) > 0) and G["dest_begin"][0] == 0
    for d in range(G["Ndest"]):
        assert np.all(np.diff(G["dest_src"][G["dest_begin"][d]:G["dest_begin"][d + 1]]) > 0)

    # ---- execution ----
    J = np.zeros((Nrows, st.Nstate), dtype=np.int64)
    vals = [rng.integers(-4, 5, size=len(r)) for r in rows]
    for r in range(Nrows): J[r, rows[r]] = vals[r]
    x = rng.integers(-4, 5, size=Nrows)
    part = np.zeros((G["Nchunks"], G["stride"]), dtype=np.int64)
    for c in range(G["Nchunks"]):
        g = G["chunk_group"][c]
        k, o = G["group_k"][g], G["group_off"][g]
        for r in G["rows"][G["chunk_begin"][c]:G["chunk_begin"][c + 1]]:
            s = [int(vals[r][p]) for p in G["spos"][o:o + k]]
            pos = 0
            for p in range(k):
                for q in range(p, k):
                    part[c, pos] += s[p]*s[q]; pos += 1
            for p in range(k):
                part[c, pos] += s[p]*int(x[r]); pos += 1
            part[c, pos] += int(x[r])**2
    got = np.zeros(Nc*Nc + Nc + 1, dtype=np.int64)
    for d in range(G["Ndest"]):
        for code in G["dest_src"][G["dest_begin"][d]:G["dest_begin"][d + 1]]:
            g, pos = code >> 10, code & 1023
            got[G["dest_id"][d]] += part[G["group_chunk_begin"][g]:G["group_chunk_begin"][g + 1], pos].sum()
    JS = J[:, [s if s < st.Nshared else s + st.NE for s in range(Nc)]]
    assert np.array_equal(got[:Nc*Nc].reshape(Nc, Nc), JS.T @ JS)          # (both triangles)
    assert np.array_equal(got[Nc*Nc:Nc*Nc + Nc], JS.T @ x)
    assert got[Nc*Nc + Nc] == x @ x


ST = State(Nshared=46, Nfb=3, Npb=5, Nwarp=2)
CAM_A = [0, 1, 2, 3, 16, 17, 18, 21]          # 8 camera-block columns: intrinsics and part of a pose
CAM_B = [8, 9, 10, 11, 22, 23, 24, 27]
def ext(i): return [16 + 6*i + k for k in range(6)]


def case_one_group(n):    return [CAM_A + ST.point(i % ST.Npb) for i in range(n)], 1
def case_interleaved():   return [(CAM_A if i % 2 == 0 else CAM_B) + ST.point(i % ST.Npb) for i in range(300)], 2
def case_positions():     return [CAM_A + ST.point(i % 3) if i % 3 else ST.point(i % 2) + CAM_A for i in range(40)], 2
def case_again_later():   return [(CAM_B if 5 <= i < 10 else CAM_A) + ST.point(0) for i in range(15)], 2
def case_pairs_12():      return [ext(i % 3) + ext(3 + i % 2) for i in range(140)], 6
def case_pairs_6():       return [ext(i % 4) for i in range(70)], 4
def case_frames_points(): return [CAM_A + ST.frame(i % ST.Nfb) if i % 4 else CAM_B[:5] + ST.warp() + ST.point(i % ST.Npb) for i in range(90)], 2

CASES = { "128": lambda: case_one_group(128), "129": lambda: case_one_group(129), "300": lambda: case_one_group(300),
          "interleaved": case_interleaved, "same columns, other positions": case_positions,
          "the same signature again later": case_again_later, "pairs, 12 columns": case_pairs_12,
          "pairs, camera at the reference": case_pairs_6, "frame and point blocks": case_frames_points }


@pytest.mark.parametrize("name", CASES)
def test_the_plan_sums_to_JtJ(lib, name):
    rows, Ngroups = CASES[name]()
    G = plan_gen_rows(lib, ST, rows)
    assert G["Ngroups"] == Ngroups
    check_plan(ST, rows, G, np.random.default_rng(len(rows)))


def test_chunks_of_the_edge_sizes(lib):
    for n, chunks in ((128, [128]), (129, [128, 1]), (300, [128, 128, 44])):
        G = plan_gen_rows(lib, ST, case_one_group(n)[0])
        assert list(np.diff(G["chunk_begin"])) == chunks


def no_plan(G):
    return all(G[k] == 0 for k in COUNTS) and all(len(G[k]) == 0 for k in LISTS)


def test_an_empty_row_range(lib):
    assert no_plan(plan_gen_rows(lib, ST, []))


GOOD = [CAM_A + ST.point(1), CAM_B + ST.frame(2)]
BAIL = { "41 camera columns":        list(range(GEN_KMAX + 1)),
         "2 of a point's 3 columns": CAM_A + ST.point(2)[:2],
         "the last 2 of a point's":  CAM_A + ST.point(2)[1:],
         "a block out of order":     CAM_A + [ST.point(2)[k] for k in (1, 0, 2)],
         "a block split":            ST.point(2)[:1] + CAM_A + ST.point(2)[1:],
         "two blocks":               CAM_A + ST.point(2) + ST.point(3),
         "a column past the state":  CAM_A + [ST.Nstate],
         "a negative column":        [-1] + CAM_A }


@pytest.mark.parametrize("name", BAIL)
def test_no_plan_is_success_with_no_rows(lib, name):
    """... and the same rows without the offending one do plan"""
    assert no_plan(plan_gen_rows(lib, ST, GOOD + [BAIL[name]] + GOOD))
    assert plan_gen_rows(lib, ST, GOOD + GOOD)["Nrows"] == 4


def test_40_camera_columns_plan(lib):
    rows = [list(range(GEN_KMAX)) + ST.point(0)]*3
    check_plan(ST, rows, plan_gen_rows(lib, ST, rows), np.random.default_rng(40))


def test_the_lds_bound_of_the_eliminated_blocks(lib):
    """gen_eblock keeps 6 Nc + 42 doubles in 64 KB: Nc = 1358 at the most. Rows without a block do not care"""
    for Nc, plans in ((1350, True), (1358, True), (1359, False), (1360, False)):
        st = State(Nshared=Nc - 2, Nfb=0, Npb=2, Nwarp=2)
        assert plan_gen_rows(lib, st, [CAM_A + st.point(1)]*3)["Nrows"] == (3 if plans else 0)
        assert plan_gen_rows(lib, st, [CAM_A]*3)["Nrows"] == 3


def test_dest_lists(lib):
    """sources per destination, in the order given -> dest_id (increasing) / dest_begin / dest_src"""
    rng = np.random.default_rng(5)
    for n in (0, 1, 500):
        dest = rng.integers(0, 60, size=n)
        code = rng.integers(0, 1 << 20, size=n)
        expect = {}
        for d, c in zip(dest, code): expect.setdefault(int(d), []).append(int(c))
        adest, pdest = as_ints(dest)
        acode, pcode = as_ints(code)
        out = np.zeros(2*n + 16, dtype=np.int32)
        m = lib.mrcal_amd_debug_dest_lists(n, pdest, pcode, out.ctypes.data_as(C.POINTER(C.c_int)), len(out))
        assert m <= len(out)
        D = read_lists(out[:m], ("dest_id", "dest_begin", "dest_src"))
        assert list(D["dest_id"]) == sorted(expect) and len(D["dest_begin"]) == len(expect) + 1 and D["dest_begin"][0] == 0
        for i, d in enumerate(D["dest_id"]):
            assert list(D["dest_src"][D["dest_begin"][i]:D["dest_begin"][i + 1]]) == expect[d]
        assert D["dest_begin"][-1] == n
