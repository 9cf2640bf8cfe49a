"""The dense and the arrowhead factorization of a bare matrix, one size at a time.

CHOLMOD_factorization(J, _partition=(Nc, Nfb, Npb, Nwarp)) takes any CSR matrix: the camera block's Cholesky (in LDS
to 180 variables, launch per panel beyond), the block elimination and SYRK in front of it, the sys= solves behind it and
the row assembly are reached here with sizes chosen one by one - every size to 200, the sizes around every multiple of
a panel beyond, the edges of the elimination's and the solves' grids - instead of the sizes a lens model and a camera
count happen to produce. The reference is a plain dense solve: with integer matrices N = JtJ, x_true and b = N x_true
are exact in doubles; with real ones N is formed in long double.

The bound of every solve here is the normwise backward error
    eta = |x N - b|_inf / (|N|_inf |x|_inf + |b|_inf)  <=  32 Nstate eps max(1, sqrt(cond2(N)))
(classical Cholesky solve: ~3 n eps; the large Cholesky's explicit inverse is allowed kappa(L) = sqrt(cond) on top,
DESIGN.md 5.3; the rest is headroom. LAPACK's cho_solve reaches 0.17 n eps on the dense family). What the GPU reaches is
printed before it is asserted, and recorded in profiles/factorization_size_sweep.txt."""
import functools
import numpy as np
import pytest
from scipy.sparse import csr_matrix

EPS = np.finfo(float).eps
LD  = np.longdouble


# ---------------------------------------------------------------- generators: seeded per case, deterministic
def _csr(indptr, indices, data, Nstate):
    return csr_matrix((np.asarray(data, dtype=float), np.asarray(indices, dtype=np.int32), np.asarray(indptr, dtype=np.int32)),
                      shape=(len(indptr) - 1, Nstate))


def _dense(J):
    """the matrix of a CSR whose explicit zeros and order are its own (nothing summed, nothing sorted)"""
    Jd = np.zeros(J.shape)
    for r in range(J.shape[0]):
        Jd[r, J.indices[J.indptr[r]:J.indptr[r+1]]] = J.data[J.indptr[r]:J.indptr[r+1]]
    return Jd


@functools.lru_cache(maxsize=4)
def dense_case(n, kind):
    """(2n+3) x n dense rows - one column list, zeros listed too: a run - then 4 I, a lane a row. The whole matrix is
    the camera block. -> J, N = JtJ (doubles, exact, for "integer"; long double for "real"), x_true (3,n), b = x_true N"""
    rng = np.random.default_rng([n, {"integer": 0, "real": 1}[kind]])
    m = 2*n + 3
    if kind == "integer":
        A      = rng.integers(-8, 9, size=(m, n)).astype(float)
        x_true = rng.integers(-9, 10, size=(3, n)).astype(float)
        x_true[np.all(x_true == 0., axis=1), 0] = 1.          # (a small n can draw a row of zeros: no solve at all)
        N      = A.T @ A + 16.*np.eye(n)                      # integers below 2^53: no product or sum rounds
        b      = x_true @ N
    else:
        A      = rng.normal(size=(m, n))
        x_true = rng.normal(size=(3, n))
        Al     = A.astype(LD)
        N      = Al.T @ Al + LD(16)*np.eye(n, dtype=LD)
        b      = (x_true.astype(LD) @ N).astype(float)
    indptr  = np.concatenate((n*np.arange(m + 1), m*n + 1 + np.arange(n)))
    indices = np.concatenate((np.tile(np.arange(n), m), np.arange(n)))
    data    = np.concatenate((A.ravel(), 4.*np.ones(n)))
    return _csr(indptr, indices, data, n), N, x_true, b


def _arrow_layout(Nc, Nfb, Npb, Nwarp):
    """state order [Nc | frames | points | warp]: (first column, width) of every eliminated block"""
    return [(Nc + 6*k, 6) for k in range(Nfb)] + [(Nc + 6*Nfb + 3*k, 3) for k in range(Npb)]


@functools.lru_cache(maxsize=4)
def arrow_case(Nc, Nfb, Npb, Nwarp):
    """per eliminated block of width w: w+4 rows of integers in the block's columns, in up to 5 random camera columns
    (all of them for every fifth block) and in the warp's; then 4 I. Integers in [-4,4]: with the 86 x 10 + 65 x 7 rows
    of the largest case in one camera column, [-8,8] would pass the condition cap of 2000.
    -> J, N (exact), x_true (3,Nstate), b"""
    rng = np.random.default_rng([Nc, Nfb, Npb, Nwarp, 7])
    Nstate = Nc + 6*Nfb + 3*Npb + Nwarp
    indptr, indices, data = [0], [], []
    for iblk, (c0, w) in enumerate(_arrow_layout(Nc, Nfb, Npb, Nwarp)):
        if iblk % 5 == 4: cam = np.arange(Nc)
        else:             cam = np.sort(rng.choice(Nc, size=rng.integers(1, min(5, Nc) + 1), replace=False))
        cols = list(cam) + list(range(c0, c0 + w)) + list(range(Nstate - Nwarp, Nstate))
        for _ in range(w + 4):
            indices += cols; data += list(rng.integers(-4, 5, size=len(cols))); indptr.append(len(indices))
    for c in range(Nstate):
        indices.append(c); data.append(4.); indptr.append(len(indices))
    J  = _csr(indptr, indices, data, Nstate)
    Jd = _dense(J)
    N  = Jd.T @ Jd
    x_true = rng.integers(-9, 10, size=(3, Nstate)).astype(float)
    x_true[np.all(x_true == 0., axis=1), 0] = 1.
    return J, N, x_true, x_true @ N


RUNS_NC, RUNS_NFB = 9, 8
def runs_case(R, tail_to_64k_plus_1=False, empty_row=False):
    """Nc = 9 and a frame block per run: R consecutive rows with one column list and REAL entries (the pre-rounded levels
    of the assembly's sums all carry something), then 3 rows with lists of their own. 5 rows of their own in front: the
    first run starts at row 5, and the runs lie across the waves' 64-row boundaries. Then 4 I.
    -> J, N = JtJ in long double"""
    rng = np.random.default_rng([R, 11])
    Nc, Nfb = RUNS_NC, RUNS_NFB
    Nstate = Nc + 6*Nfb
    indptr, indices, data = [0], [], []
    def row(cols):
        indices.extend(cols); data.extend(rng.normal(size=len(cols))); indptr.append(len(indices))
    def own_row(f):
        row(sorted(rng.choice(Nc, size=3, replace=False)) + [Nc + 6*f + k for k in sorted(rng.choice(6, size=4, replace=False))])
    for _ in range(5): own_row(0)
    for f in range(Nfb):
        cols = sorted(rng.choice(Nc, size=4, replace=False)) + [Nc + 6*f + k for k in range(6)]
        for i in range(R):
            if empty_row and f == Nfb//2 and i == R//2: indptr.append(len(indices))
            row(cols)
        for _ in range(3): own_row(f)
    for c in range(Nstate):
        indices.append(c); data.append(4.); indptr.append(len(indices))
    while tail_to_64k_plus_1 and (len(indptr) - 1) % 64 != 1: own_row(Nfb - 1)
    J  = _csr(indptr, indices, data, Nstate)
    Jl = _dense(J).astype(LD)
    return J, Jl.T @ Jl


def _runs_across_wave_boundaries(R):
    """how many of runs_case(R)'s runs have rows in two waves (64 consecutive rows each)"""
    starts = [5 + f*(R + 3) for f in range(RUNS_NFB)]
    return sum(1 for s in starts if s//64 != (s + R - 1)//64)


# ---------------------------------------------------------------- the cases
DENSE_GROUPS = { "1-50": range(1, 51), "51-100": range(51, 101), "101-150": range(101, 151), "151-200": range(151, 201),
                 "panel edges to 400": (201, 255, 256, 257, 319, 320, 321, 383, 384, 385, 400) }
ENTRY_SIZES  = (1, 2, 15, 16, 17, 31, 33, 64, 65, 129, 177, 178, 179, 180, 181, 182, 193, 257)
# (Nc, Nfb, Npb, Nwarp). The camera block is Nc + Nwarp wide: the LDS Cholesky's last sizes (178, 180), the elimination's
# and the SYRK's changes of kernel (255 | 256 | 257) are met with and without the warp. Eliminated blocks: one of either
# kind alone; 63 and 66 rows (a slab of the solve's reduction, a slice of the SYRK: 64); 64 | 129 | 151 blocks (the
# forward solve takes 64 a workgroup); 510 and 711 rows (8 slices and more)
ARROW_CASES = (
    (  1,  1,  0, 0), (  1,  0,  1, 0), (  1, 10,  1, 2), (  1, 86, 65, 0),
    ( 15, 11,  0, 0), ( 15,  0, 21, 2), ( 15, 64,  0, 0), ( 15, 10,  1, 0),
    ( 16,  0, 22, 0), ( 16, 65, 64, 2), ( 16,  1,  0, 2), ( 16, 11,  0, 0),
    ( 17,  0,  1, 2), ( 17, 85,  0, 0), ( 17,  0, 21, 0), ( 17, 65, 64, 0),
    ( 33, 64,  0, 2), ( 33, 86, 65, 0), ( 33,  0, 22, 2), ( 33, 10,  1, 0),
    (178,  1,  0, 0), (178, 65, 64, 0), (178, 85,  0, 2), (178,  0, 22, 0),
    (181,  0,  1, 0), (181, 86, 65, 2), (181, 11,  0, 0), (181, 64,  0, 0),
    (255, 85,  0, 0), (255, 86, 65, 0), (255, 85,  0, 2), (255, 10,  1, 2),
    (256, 85,  0, 0), (256, 86, 65, 0), (256, 86, 65, 2), (256,  0, 21, 0),
    (257, 85,  0, 0), (257, 86, 65, 0), (257, 85,  0, 2), (257, 65, 64, 2),
)
RUN_LENGTHS = (13, 14, 15, 16, 17, 18, 19, 63, 64, 65, 130)


@functools.lru_cache(maxsize=None)
def _cond_dense(n, kind): return float(np.linalg.cond(np.asarray(dense_case(n, kind)[1], dtype=float)))
@functools.lru_cache(maxsize=None)
def _cond_arrow(case): return float(np.linalg.cond(arrow_case(*case)[1]))


def cap(Nstate, cond):
    return 32.*Nstate*EPS*max(1., np.sqrt(cond))


def backward_error(x, N, b):
    """the normwise backward error of every row of x as a solution of x N = b (N symmetric), in long double"""
    Nl, xl, bl = np.asarray(N, dtype=LD), np.asarray(x, dtype=LD), np.asarray(b, dtype=LD)
    res  = np.abs(xl @ Nl - bl).max(axis=-1)
    Ninf = np.abs(Nl).sum(axis=1).max()
    return np.asarray(res/(Ninf*np.abs(xl).max(axis=-1) + np.abs(bl).max(axis=-1)), dtype=float)


# ---------------------------------------------------------------- the generators' own check: no GPU
def test_generated_cases_are_well_conditioned_and_exact():
    """every case of the tests below: cond(N) <= 50 (dense family), <= 2000 (arrowheads), and the integer kinds exact in
    doubles with room to spare (|N| < 2^40: N x_true and the reference's own sums stay far below 2^53)"""
    worst = 0.
    for n in sorted(set(n for g in DENSE_GROUPS.values() for n in g) | set(ENTRY_SIZES)):
        N = dense_case(n, "integer")[1]
        assert N.dtype == np.float64 and np.array_equal(N, np.round(N)) and np.abs(N).max() < 2.**40, n
        assert _cond_dense(n, "integer") <= 50., (n, _cond_dense(n, "integer"))
        worst = max(worst, _cond_dense(n, "integer"))
    for n in ENTRY_SIZES:
        assert dense_case(n, "real")[1].dtype == LD
        assert _cond_dense(n, "real") <= 50., (n, _cond_dense(n, "real"))
        worst = max(worst, _cond_dense(n, "real"))
    print(f"dense family: cond <= {worst:.1f}")
    assert len(set(ARROW_CASES)) == len(ARROW_CASES) == 40
    for case in ARROW_CASES:
        J, N, x_true, b = arrow_case(*case)
        assert J.shape[1] <= 3200
        assert np.array_equal(N, np.round(N)) and np.abs(N).max() < 2.**40, case
        assert np.array_equal(b, np.round(b)) and np.abs(b).max() < 2.**50, case
        assert _cond_arrow(case) <= 2000., (case, _cond_arrow(case))
        print(f"arrow {case}: Nstate {J.shape[1]}, cond {_cond_arrow(case):.0f}")
    # the cases the issue's selection rule asks for: every value of each axis twice, the wide camera blocks with both big E parts
    for axis in (0, slice(1, 3), 3):
        vals = [c[axis] for c in ARROW_CASES]
        assert all(vals.count(v) >= 2 for v in vals), axis
    for Nc in (255, 256, 257):
        assert {(85, 0), (86, 65)} <= {c[1:3] for c in ARROW_CASES if c[0] == Nc}
    # the runs lie across wave boundaries, and each half of a wave gets 6 to 9 rows of the short ones
    for R in RUN_LENGTHS:
        assert _runs_across_wave_boundaries(R) >= 1, R
        J, N = runs_case(R)
        assert np.linalg.cond(np.asarray(N, dtype=float)) <= 2000.
    assert runs_case(16, tail_to_64k_plus_1=True)[0].shape[0] % 64 == 1
    Je = runs_case(16, empty_row=True)[0]
    assert Je.shape[0] == runs_case(16)[0].shape[0] + 1 and (np.diff(Je.indptr) == 0).sum() == 1


# ---------------------------------------------------------------- GPU
def _path(n):
    return "LDS" if n <= 178 else ("179-180" if n <= 180 else "large")


def _check_solve(tag, F, N, x_true, b, cond):
    """the A solve of 3 right-hand sides with a known answer: backward and forward error under the cap. -> x"""
    n = N.shape[0]
    x = F.solve_xt_JtJ_bt(b)
    eta = backward_error(x, N, b).max()
    fwd = np.abs(x - x_true).max()/np.abs(x_true).max()
    print(f"{tag}: eta/(n eps) {eta/(n*EPS):.4f}  forward/(n eps cond) {fwd/(n*EPS*cond):.4f}  cap/(n eps) {cap(n, cond)/(n*EPS):.1f}")
    assert np.all(np.isfinite(x)), tag
    assert eta <= cap(n, cond), (tag, eta, cap(n, cond))
    assert fwd <= cap(n, cond)*cond, (tag, fwd, cap(n, cond)*cond)
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("group", DENSE_GROUPS)
def test_dense_every_size(amd, group):
    """the whole matrix as the camera block, every n: the LDS Cholesky with every length of its last panel, 179 and 180
    (factored in LDS, solved by the blocked kernel), the launch-per-panel Cholesky around every multiple of its 64"""
    for n in DENSE_GROUPS[group]:
        J, N, x_true, b = dense_case(n, "integer")
        cond = _cond_dense(n, "integer")
        F = amd.CHOLMOD_factorization(J)
        x = _check_solve(f"dense n={n} path={_path(n)}", F, N, x_true, b, cond)
        dL = np.diag(np.linalg.cholesky(N))
        expected = (dL.min()/dL.max())**2
        assert abs(F.rcond() - expected) <= 1e-10*expected, (n, F.rcond(), expected)
        F2 = amd.CHOLMOD_factorization(J)
        assert np.array_equal(F2.solve_xt_JtJ_bt(b), x) and F2.rcond() == F.rcond(), n


def _check_factor(tag, F, N):
    """L lower triangular, P a permutation, L L^T = P N P^T entry by entry (in long double). -> L, P"""
    from test_factorization_project import _factor_dense
    n = N.shape[0]
    cond = float(np.linalg.cond(np.asarray(N, dtype=float)))
    L, Pm = _factor_dense(F, n)
    assert np.abs(np.triu(L, 1)).max() <= cap(n, cond)*np.abs(L).max(), tag
    assert np.isin(Pm, (0., 1.)).all() and np.all(Pm.sum(axis=0) == 1) and np.all(Pm.sum(axis=1) == 1), tag
    Ll  = np.tril(L).astype(LD)
    order = (Pm @ np.arange(n)).round().astype(int)
    PNP = np.asarray(N, dtype=LD)[np.ix_(order, order)]
    err = float(np.abs(Ll @ Ll.T - PNP).max()/np.abs(PNP).max())
    print(f"{tag}: |L Lt - P N Pt|/|N| /(n eps) {err/(n*EPS):.4f}  cap/(n eps) {cap(n, cond)/(n*EPS):.1f}")
    assert err <= cap(n, cond), (tag, err, cap(n, cond))
    return L, Pm


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("integer", "real"))
@pytest.mark.parametrize("n", ENTRY_SIZES)
def test_dense_factor_entry_by_entry(amd, n, kind):
    """the factor itself and all nine systems, at the panel edges of either Cholesky and on both sides of the LDS
    kernel's last size: 179 and 180 are factored in LDS and solved against by fsolve_dense_blocked_kernel"""
    J, N, _, _ = dense_case(n, kind)
    cond = _cond_dense(n, kind)
    F = amd.CHOLMOD_factorization(J)
    L, Pm = _check_factor(f"factor n={n} {kind} path={_path(n)}", F, N)
    rng = np.random.default_rng([n, 3])
    B = rng.normal(size=(3, n))
    bound = cap(n, cond)
    Nd = np.asarray(N, dtype=float)
    ops = {"A": Nd, "L": L, "LD": L, "Lt": L.T, "DLt": L.T, "LDLt": L @ L.T, "D": np.eye(n), "P": Pm.T, "Pt": Pm}
    for sys, M in ops.items():
        got = F.solve_xt_JtJ_bt(B, sys=sys)
        res = np.abs(np.asarray((M.astype(LD) @ got.T.astype(LD)).T - B, dtype=float)).max()
        lim = bound*np.abs(M).max()*np.abs(got).max()/max(1.0, np.abs(B).max()) + bound
        print(f"n={n} {kind} sys={sys}: residual {res:.3g}  limit {lim:.3g}")
        assert np.all(np.isfinite(got)) and res <= lim, (n, kind, sys, res, lim)
    # a row alone has the bits it has in a batch of n rows
    Bn = rng.normal(size=(n, n))
    for sys in ("A", "L", "Lt", "LDLt", "P"):
        big = F.solve_xt_JtJ_bt(Bn, sys=sys)
        for i in sorted({0, n//2, n - 1}):
            assert np.array_equal(F.solve_xt_JtJ_bt(Bn[i], sys=sys), big[i]), (n, kind, sys, i)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ARROW_CASES, ids=["-".join(str(v) for v in c) for c in ARROW_CASES])
def test_arrowhead_edges(amd, case):
    """frame and point blocks eliminated onto a camera block: the elimination, the SYRK's slices and tiles, the Cholesky
    of the Schur complement and the solves' reductions at the sizes where their grids and kernels change"""
    Nc, Nfb, Npb, Nwarp = case
    J, N, x_true, b = arrow_case(*case)
    n, cond = N.shape[0], _cond_arrow(case)
    F = amd.CHOLMOD_factorization(J, _partition=case)
    x = _check_solve(f"arrow {case} Nstate={n}", F, N, x_true, b, cond)
    if n <= 700:
        _, Pm = _check_factor(f"arrow factor {case}", F, N)
        # the factor's order: the eliminated blocks first, then the camera block with the warp behind it
        order = (Pm @ np.arange(n)).round().astype(int)
        assert np.array_equal(order, np.concatenate((np.arange(Nc, n - Nwarp), np.arange(Nc), np.arange(n - Nwarp, n)))), case
    F2 = amd.CHOLMOD_factorization(J, _partition=case)
    assert np.array_equal(F2.solve_xt_JtJ_bt(b), x) and F2.rcond() == F.rcond(), case


def _check_runs(amd, tag, J, N):
    part = (RUNS_NC, RUNS_NFB, 0, 0)
    Fs = [amd.CHOLMOD_factorization(J, _partition=part) for _ in range(3)]
    _check_factor(tag, Fs[0], N)
    bt = np.random.default_rng(5).normal(size=(3, J.shape[1]))
    xs = [F.solve_xt_JtJ_bt(bt) for F in Fs]
    Ls = [F.solve_xt_JtJ_bt(bt, sys="L") for F in Fs]
    for k in (1, 2):
        assert np.array_equal(xs[k], xs[0]) and np.array_equal(Ls[k], Ls[0]) and Fs[k].rcond() == Fs[0].rcond(), tag


@pytest.mark.gpu
@pytest.mark.parametrize("R", RUN_LENGTHS)
def test_row_runs(amd, R):
    """the row assembly's sums across a half-wave: runs that leave 6 to 9 rows to a half (R = 13 ... 19: the halves hold
    the even and the odd rows), whole waves and more, all of them across 64-row boundaries, with real entries"""
    J, N = runs_case(R)
    _check_runs(amd, f"runs R={R}", J, N)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ("64k+1 rows", "empty row"))
def test_row_runs_last_wave_and_empty_row(amd, variant):
    """a last wave that holds one row; a row without entries in the middle of a run"""
    J, N = runs_case(16, tail_to_64k_plus_1=(variant == "64k+1 rows"), empty_row=(variant == "empty row"))
    _check_runs(amd, f"runs {variant}", J, N)


@pytest.mark.gpu
@pytest.mark.parametrize("R", (7, 8))
def test_short_groups_go_row_by_row(amd, R):
    """Fewer than 8 rows of a wave with the same columns are not a run: they go one lane a row, through sums in which no
    addition rounds - so the factor does not depend on the ORDER of such rows. (A run's sum across the half-wave is
    rounded: with 8 rows it may depend on it, and nothing is asserted about that but the accuracy.) Waves of 64 rows,
    each holding R rows of one column list at the even and odd places alike, and rows of their own"""
    rng = np.random.default_rng([R, 13])
    Nc, Nfb = RUNS_NC, 4
    Nstate = Nc + 6*Nfb
    rows = []
    for f in range(Nfb):
        cols = sorted(rng.choice(Nc, size=4, replace=False)) + [Nc + 6*f + k for k in range(6)]
        wave = [(cols, rng.normal(size=len(cols))) for _ in range(R)]
        for _ in range(64 - R):
            c = sorted(rng.choice(Nc, size=3, replace=False)) + [Nc + 6*f + k for k in sorted(rng.choice(6, size=4, replace=False))]
            wave.append((c, rng.normal(size=len(c))))
        rows.append(wave)
    def build(order):
        indptr, indices, data = [0], [], []
        for f, wave in enumerate(rows):
            for i in order[f]:
                indices.extend(wave[i][0]); data.extend(wave[i][1]); indptr.append(len(indices))
        for c in range(Nstate):
            indices.append(c); data.append(4.); indptr.append(len(indices))
        return _csr(indptr, indices, data, Nstate)
    J0 = build([np.arange(64)]*Nfb)                                  # the R rows first: R//2 (+1) to each half
    J1 = build([rng.permutation(64) for _ in range(Nfb)])            # the same rows of every wave in another order
    Jl = _dense(J0).astype(LD)
    N  = Jl.T @ Jl
    F0 = amd.CHOLMOD_factorization(J0, _partition=(Nc, Nfb, 0, 0))
    F1 = amd.CHOLMOD_factorization(J1, _partition=(Nc, Nfb, 0, 0))
    _check_factor(f"short groups R={R}", F0, N)
    _check_factor(f"short groups R={R} shuffled", F1, N)
    if R < 8:
        I = np.eye(Nstate)
        assert np.array_equal(F0.solve_xt_JtJ_bt(I, sys="L"), F1.solve_xt_JtJ_bt(I, sys="L"))
        assert F0.rcond() == F1.rcond()


@pytest.mark.gpu
def test_no_camera_block_is_refused(amd):
    """Nc = Nwarp = 0 - nothing but eliminated blocks - is not served: the Schur complement's reduction and the solve's
    would be launched on grids of no workgroups. Refused with a message before anything is queued"""
    rng = np.random.default_rng(1)
    Nfb = 3
    A = np.zeros((10*Nfb, 6*Nfb))
    for f in range(Nfb): A[10*f:10*f + 10, 6*f:6*f + 6] = rng.normal(size=(10, 6))
    with pytest.raises(RuntimeError, match="no variable outside the eliminated blocks"):
        amd.CHOLMOD_factorization(csr_matrix(A), _partition=(0, Nfb, 0, 0))
    with pytest.raises(RuntimeError, match="no variable outside the eliminated blocks"):
        amd.CHOLMOD_factorization(csr_matrix((0, 0)))
    # one camera variable beside the same blocks is served
    A1 = np.column_stack((rng.normal(size=10*Nfb), A))
    F = amd.CHOLMOD_factorization(csr_matrix(A1), _partition=(1, Nfb, 0, 0))
    N = A1.T @ A1
    b = rng.normal(size=(2, 1 + 6*Nfb))
    cond = np.linalg.cond(N)
    assert backward_error(F.solve_xt_JtJ_bt(b), N, b).max() <= cap(N.shape[0], cond)
