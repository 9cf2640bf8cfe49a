"""The board kernel's tile with one row a lane (csrc/problem.hpp, board_lane_corner(), board_tile_row(); csrc/kernels.hip):
with everything optimized, a lane no longer computes the corner of its own number. Inside each half of 32 corners
in-half lane j takes corner j/2 + 16 (j%2), writes tile row `lane`, and the Gram and the copy-out find the rows where
that puts them. Nothing a caller sees may move: which corner a residual and a Jacobian row belong to, what is summed
into the normal equations and in which order.

  boards     6x4 (24 corners: a partial first half, its live lanes all over the half), 11x4 (44: a full half and a
             second one of 12 corners), 7x7 (49: a second half of 17)
  problems   2 cameras x 3 frames, seed 3, tests/test_board_tile_handoff.py's three variants: OPENCV8 with everything
             optimized (the new layout), OPENCV8 with the distortions locked (the general kernel, the rows in order),
             OPENCV4 (six column blocks)
  outliers   observation 2, one corner in each of the in-half ranges 8..15 and 16..23, in the last half of the board
             that has such a corner

  - x and J of optimizer_callback() against the compiled reference: the structure bit for bit, the values to that
    file's REL_TOL; the outliers' rows are zeros
  - normal_equations() against JtJ and Jtx formed in numpy from the problem's own J() and x(): 1e-10 of the largest entry
  - the same bits with and without the Jacobian stream, at the seed and after two solver steps
  - A, Bt, D, g, norm2_x, x at the seed and after two steps, and b_packed after them, bit for bit against
    tests/golden/lane_permutation/<case>.npz. The fixtures were recorded on an MI355X by
    tools/record_lane_permutation_goldens.py from the library of commit 285e373 ("Board Gram in 7 MFMAs a k-step for
    OPENCV8; Gram stride by lookup"), the last one in which every board kernel had lane = corner and the rows in order.
"""
import os
import numpy as np
import pytest

from conftest import relative_error
from mrcal_amd.synthetic import make_calibration_problem, copy_inputs
from test_board_tile_handoff import VARIANTS, REL_TOL, blocks_to_dense, dense_normal
from test_gram_packing_gpu import state

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lane_permutation")

BOARDS = ((6, 4), (11, 4), (7, 7))


def outlier_corners(W, H):
    """one corner in each of the in-half ranges 8..15 and 16..23, in the last half of the board that has one"""
    n = W*H
    out = []
    for lo in (8, 16):
        first = ((n - 1 - lo)//32)*32               # the first corner of the last half that reaches into the range
        assert first >= 0
        out.append(min(first + lo + 2, n - 1))
    return out


def problem(api, W, H, variant):
    lensmodel, flags = VARIANTS[variant]
    oi, _ = make_calibration_problem(api, Ncameras=2, Nframes=3, lensmodel=lensmodel,
                                     object_width_n=W, object_height_n=H, seed=3)
    oi.update(flags)
    for pt in outlier_corners(W, H):
        oi["observations_board"][2, pt // W, pt % W, 2] = -1.
    return oi


def case_name(W, H, variant):
    return f"{variant}-{W}x{H}"


def evaluate_case(api, W, H, variant, stream=True, check=None):
    """what a fixture holds: the normal equations and x at the seed and after two solver steps, b_packed after them.
    check(p), if given, is called at the seed"""
    from mrcal_amd.resident import Problem
    with Problem(**copy_inputs(problem(api, W, H, variant))) as p:
        p.set_jacobian_stream(stream)
        out = state(p, "seed", False)
        if check is not None: check(p)
        n, _ = p.run_steps(2)
        assert n == 2
        out.update(state(p, "step2", True))
    return out


def test_outlier_corners():
    assert outlier_corners(6, 4) == [10, 18] and outlier_corners(11, 4) == [42, 18] and outlier_corners(7, 7) == [42, 48]


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("W,H", BOARDS)
def test_callback_against_reference(amd, ref_api, W, H, variant):
    oi = problem(amd._api, W, H, variant)
    _, x_a, J_a, _ = amd.optimizer_callback(no_factorization=True, **copy_inputs(oi))
    _, x_r, J_r, _ = ref_api.optimizer_callback(no_factorization=True, **copy_inputs(oi))
    assert J_a.shape == J_r.shape
    assert np.array_equal(J_a.indptr,  J_r.indptr)
    assert np.array_equal(J_a.indices, J_r.indices)
    ex, eJ = relative_error(x_a, x_r), relative_error(J_a.data, J_r.data)
    print(f"{W}x{H} {variant}: max rel err x {ex.max():.3g}, J {eJ.max():.3g}")
    assert ex.max() < REL_TOL
    assert eJ.max() < REL_TOL, f"J at nnz {eJ.argmax()}: ours {J_a.data[eJ.argmax()]} reference {J_r.data[eJ.argmax()]}"
    for pt in outlier_corners(W, H):
        i = 2*(2*W*H + pt)
        assert not J_a.data[J_a.indptr[i]:J_a.indptr[i+2]].any() and not x_a[i:i+2].any()
    # ... and theirs alone: every other row of that observation has values
    zero_rows = [r for r in range(2*2*W*H, 2*3*W*H) if not J_a.data[J_a.indptr[r]:J_a.indptr[r+1]].any()]
    assert zero_rows == sorted(2*(2*W*H + pt) + xy for pt in outlier_corners(W, H) for xy in (0, 1))


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("W,H", BOARDS)
def test_normal_equations_stream_and_recorded_bits(amd, W, H, variant):
    def against_numpy(p):
        ne, x = p.normal_equations(), p.x()
        N, g = dense_normal(p.J(), x)
        eN = np.abs(blocks_to_dense(ne, p.Nstate) - N).max() / np.abs(N).max()
        eg = np.abs(ne["g"] - g).max() / np.abs(g).max()
        print(f"{W}x{H} {variant}: JtJ off by {eN:.3g}, Jtx by {eg:.3g} of the largest entry")
        assert eN < 1e-10
        assert eg < 1e-10
        assert abs(ne["norm2_x"] - x @ x) < 1e-10*(x @ x)

    got     = evaluate_case(amd._api, W, H, variant, stream=True, check=against_numpy)
    without = evaluate_case(amd._api, W, H, variant, stream=False)
    assert sorted(got) == sorted(without)
    assert not [k for k in got if not np.array_equal(got[k], without[k])]

    golden = np.load(os.path.join(GOLDEN, case_name(W, H, variant) + ".npz"))
    assert sorted(golden.files) == sorted(got)
    different = [k for k in sorted(got) if not np.array_equal(got[k], golden[k])]
    for k in different:
        d = np.abs(got[k] - golden[k])
        print(f"{W}x{H} {variant}: {k} differs in {np.count_nonzero(d)} of {d.size} values, by {d.max():.3g} at most")
    assert not different
