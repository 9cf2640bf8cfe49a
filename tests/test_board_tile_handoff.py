"""The board kernel's tile hand-off: every combination of pass and half that its loops can take.

A pass is 64 corners; its two halves (32 corners = 64 rows each) go through the LDS tile one after the other, each
from its own set of row registers, and the Gram's accumulators live across all of them (csrc/kernels.hip,
board_observation()). The board sizes below make every shape of that loop occur: a partial first half alone, a
full first half with a partial second, both full, a second pass that stops after a partial first half, and second
passes with a short and with a long second half. Camera 0 has no extrinsics (rows of 18 nonzeros with OPENCV8),
camera 1 has them (24): both copy-out fast paths run. One corner of one observation is an outlier: its rows are
zeros.

  - x and J of optimizer_callback() against the compiled reference: the structure bit for bit, the values to 1e-6
    relative (tests/test_callback_parity.py's bar)
  - a resident Problem's normal equations against JtJ and Jtx formed in numpy from its own J() and x(): 1e-10 of
    the largest entry (tests/test_moving_camera.py::test_callback_and_normal_equations' bar)
  - the same problem told to leave the Jacobian stream out: the same bits in the normal equations and x - at the
    seed, and after two solver steps, whose evaluations are the ones that go without the stream
"""
import numpy as np
import pytest

from conftest import relative_error
from mrcal_amd.synthetic import make_calibration_problem, copy_inputs

pytestmark = pytest.mark.gpu

REL_TOL = 1e-6

BOARDS = ((5, 5),       # 25 corners: first half partial, no second half
          (8, 5),       # 40: first half full, second half 16 rows
          (8, 8),       # 64: both halves full, one pass exactly
          (9, 8),       # 72: second pass with a partial first half only
          (10, 10),     # 100: second pass, second half of 8 rows
          (12, 10))     # 120: second pass, second half of 48 rows

VARIANTS = {"opencv8-all":            ("LENSMODEL_OPENCV8", {}),                                                # everything optimized
            "opencv8-no-distortions": ("LENSMODEL_OPENCV8", dict(do_optimize_intrinsics_distortions=False)),   # the general kernel
            "opencv4-all":            ("LENSMODEL_OPENCV4", {})}                                                # six column blocks


def dense_normal(J, x):
    Jd = J.toarray()
    return Jd.T @ Jd, Jd.T @ x


def blocks_to_dense(ne, Nstate):
    """the solver's block form as the dense (Nstate,Nstate) JtJ: S index s is state s below S_split and
    s + S_shift from there on, E index e is state E_state0 + e (Problem.partition())"""
    Nc, NE, Nfb = ne["Nc"], ne["NE"], ne["Nfb"]
    s = np.arange(Nc)
    sidx = np.where(s < ne["S_split"], s, s + ne["S_shift"]).astype(int)
    E0 = ne["E_state0"]
    N = np.zeros((Nstate, Nstate))
    N[np.ix_(sidx, sidx)] = ne["A"]
    for e in range(NE):
        N[E0+e, sidx] = ne["Bt"][e]
        N[sidx, E0+e] = ne["Bt"][e]
    for b in range(ne["NEb"]):
        if b < Nfb: e0, de = 6*b, 6
        else:       e0, de = 6*Nfb + 3*(b-Nfb), 3
        N[E0+e0:E0+e0+de, E0+e0:E0+e0+de] = ne["D"][b,:de,:de]
    return N


def problem(api, W, H, variant):
    lensmodel, flags = VARIANTS[variant]
    oi, _ = make_calibration_problem(api, Ncameras=2, Nframes=3, lensmodel=lensmodel,
                                     object_width_n=W, object_height_n=H, seed=3)
    oi.update(flags)
    # an outlier in the last half that the board has: observation 2's last corner but one
    oi["observations_board"][2, H-1, W-2, 2] = -1.
    return oi


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
    # the outlier's two rows are stored zeros
    i = 2*(2*W*H + (H-1)*W + (W-2))
    assert not J_a.data[J_a.indptr[i]:J_a.indptr[i+2]].any() and not x_a[i:i+2].any()


def _state(p):
    ne = p.normal_equations()
    return ne, p.x()


def _same_bits(a, b):
    (ne_a, x_a), (ne_b, x_b) = a, b
    for k in ("A", "Bt", "D", "g"):
        assert np.array_equal(ne_a[k], ne_b[k]), k
    assert ne_a["norm2_x"] == ne_b["norm2_x"]
    assert np.array_equal(x_a, x_b)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("W,H", BOARDS)
def test_normal_equations_with_and_without_the_stream(amd, W, H, variant):
    from mrcal_amd.resident import Problem
    oi = problem(amd._api, W, H, variant)
    res = []
    for stream in (True, False):
        with Problem(**copy_inputs(oi)) as p:
            p.set_jacobian_stream(stream)
            ne, x = seed = _state(p)
            if stream:
                J = p.J()
                N, g = dense_normal(J, x)
                eN = np.abs(blocks_to_dense(ne, p.Nstate) - N).max() / np.abs(N).max()
                eg = np.abs(ne["g"] - g).max() / np.abs(g).max()
                print(f"{W}x{H} {variant}: JtJ off by {eN:.3g}, Jtx by {eg:.3g} of the largest entry")
                assert eN < 1e-10
                assert eg < 1e-10
                assert abs(ne["norm2_x"] - x @ x) < 1e-10*(x @ x)
            # the solver's own evaluations are the ones that leave the stream out
            n, _ = p.run_steps(2)
            assert n == 2
            res.append((seed, _state(p), p.b_packed()))
    _same_bits(res[0][0], res[1][0])
    _same_bits(res[0][1], res[1][1])
    assert np.array_equal(res[0][2], res[1][2])
