"""What the board kernel makes of the Gram packings (csrc/problem.hpp, gram_packing(); csrc/kernels.hip): every number
of column blocks a board tile can have, every shape of the kernel's loop over a board.

  lens models   no distortions (5 column blocks), OPENCV4 (6), OPENCV8 (7: everything optimized, and with the
                distortions locked for the general kernel), OPENCV12 (8)
  boards        5x5 (a partial first half), 8x5 (a full half + 16 rows), 9x8 (a second pass with a partial first half),
                10x10 (the metric's shape)
  problems      2 cameras x 3 frames, seed 3, one outlier corner: tests/test_board_tile_handoff.py::problem()

  - normal_equations() against JtJ and Jtx formed in numpy from the problem's own J() and x(): 1e-10 of the largest
    entry (tests/test_board_tile_handoff.py's bar)
  - A, Bt, D, g, norm2_x and x at the seed, and the same with b_packed after run_steps(2), bit for bit against
    tests/golden/gram_packing/<case>.npz, recorded on the GPU from the library as it was before the packings were
    repacked (tools/record_gram_goldens.py). A packing decides WHERE a product is formed and stored, never what is
    multiplied or in which order it is summed: the same operand values go through v_mfma_f64_4x4x4 in the same k order,
    and where a block pair is stored the other way round, a*b = b*a exactly.
"""
import os
import numpy as np
import pytest

from mrcal_amd.synthetic import make_calibration_problem, copy_inputs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gram_packing")

BOARDS = ((5, 5), (8, 5), (9, 8), (10, 10))

VARIANTS = {"pinhole":                ("LENSMODEL_PINHOLE",  {}),                                               # 5 column blocks
            "opencv4":                ("LENSMODEL_OPENCV4",  {}),                                               # 6
            "opencv8":                ("LENSMODEL_OPENCV8",  {}),                                               # 7
            "opencv8-no-distortions": ("LENSMODEL_OPENCV8",  dict(do_optimize_intrinsics_distortions=False)),   # 7, the general kernel
            "opencv12":               ("LENSMODEL_OPENCV12", {})}                                               # 8

NORMAL = ("A", "Bt", "D", "g")


def problem(api, W, H, variant):
    lensmodel, flags = VARIANTS[variant]
    oi, _ = make_calibration_problem(api, Ncameras=2, Nframes=3, lensmodel=lensmodel,
                                     object_width_n=W, object_height_n=H, seed=3)
    oi.update(flags)
    # an outlier in the last half that the board has: observation 2's last corner but one
    oi["observations_board"][2, H-1, W-2, 2] = -1.
    return oi


def case_name(W, H, variant):
    return f"{variant}-{W}x{H}"


def state(p, prefix, with_b):
    ne = p.normal_equations()
    out = {f"{prefix}_{k}": np.array(ne[k]) for k in NORMAL}
    out[f"{prefix}_norm2_x"] = np.array(ne["norm2_x"], dtype=np.float64)
    out[f"{prefix}_x"] = np.array(p.x())
    if with_b: out[f"{prefix}_b_packed"] = np.array(p.b_packed())
    return out


def evaluate_case(api, W, H, variant, check=None):
    """what a fixture holds: the normal equations and x at the seed and after two solver steps, b_packed after them.
    check(p), if given, is called at the seed"""
    from mrcal_amd.resident import Problem
    with Problem(**copy_inputs(problem(api, W, H, variant))) as p:
        out = state(p, "seed", False)
        if check is not None: check(p)
        n, _ = p.run_steps(2)
        assert n == 2
        out.update(state(p, "step2", True))
    return out


def dense_normal_equations(ne, Nstate):
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


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("W,H", BOARDS)
def test_normal_equations_and_recorded_bits(amd, W, H, variant):
    def against_numpy(p):
        ne, x = p.normal_equations(), p.x()
        Jd = p.J().toarray()
        N, g = Jd.T @ Jd, Jd.T @ x
        eN = np.abs(dense_normal_equations(ne, p.Nstate) - N).max() / np.abs(N).max()
        eg = np.abs(ne["g"] - g).max() / np.abs(g).max()
        print(f"{W}x{H} {variant}: JtJ off by {eN:.3g}, Jtx by {eg:.3g} of the largest entry")
        assert eN < 1e-10
        assert eg < 1e-10
        assert abs(ne["norm2_x"] - x @ x) < 1e-10*(x @ x)

    got = evaluate_case(amd._api, W, H, variant, check=against_numpy)
    golden = np.load(os.path.join(GOLDEN, case_name(W, H, variant) + ".npz"))
    assert sorted(golden.files) == sorted(got)
    different = [k for k in sorted(got) if not np.array_equal(got[k], golden[k])]
    for k in different:
        d = np.abs(got[k] - golden[k])
        print(f"{W}x{H} {variant}: {k} differs in {np.count_nonzero(d)} of {d.size} values, by {d.max():.3g} at most")
    assert not different
