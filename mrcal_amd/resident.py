"""Resident tier: a calibration problem held in HBM across evaluations and
solver steps (include/mrcal_amd.h, mrcal_amd_problem_*). This is what the
benchmark and the multi-GPU driver use; optimize()/optimizer_callback() are the
one-shot forms of the same thing.
"""
import ctypes as C
import numpy as np

from . import _handle
from ._cabi import _ptr
from ._handle import Handle, _failed


class Problem(Handle):
    """One optimization problem (or one frame-shard of it) resident on the
    current HIP device.

        p = Problem(**optimization_inputs)
        p.evaluate()                 # x, J at the resident packed state
        x = p.x()                    # host copies on demand
    """

    _destroy = "mrcal_amd_problem_destroy"
    _error = RuntimeError

    def __init__(self, _shard=(0,-1), _leader=True, _shard_points=(0,-1), _shard_tripoints=(0,-1), _ingested=None,
                 **optimization_inputs):
        lib, _api = _handle._libs()
        self._api = _api
        self._lib = lib.lib
        # (_ingested: the marshalled arguments of an optimizer_callback() call, which holds them already)
        p = _ingested if _ingested is not None else _api._ingest(optimization_inputs, callback=False)
        self._inputs = p   # keeps the numpy arrays alive
        a = _api._common_args(p)
        # common args: ..., lensmodel, imagersizes, sel, problem_constants, spacing, W, H, verbose
        self._create("mrcal_amd_problem_create()", "mrcal_amd_problem_create_sharded",
                     *a[:18], a[18], a[19], a[20], a[22], a[23], a[24],
                     int(_shard[0]), int(_shard[1]), int(_shard_points[0]), int(_shard_points[1]),
                     int(_shard_tripoints[0]), int(_shard_tripoints[1]), bool(_leader))
        self.Nstate = self._lib.mrcal_amd_problem_Nstate(self.handle)
        self.Nmeas  = self._lib.mrcal_amd_problem_Nmeasurements(self.handle)
        self.Nnz    = self._lib.mrcal_amd_problem_Nnz(self.handle)
        self.Nstate_global, self.Nmeas_global, self.Nnz_global = self.Nstate, self.Nmeas, self.Nnz

    def evaluate(self, with_jacobian=True, sync=True):
        self._call("evaluate", "mrcal_amd_problem_evaluate", with_jacobian, sync)

    def jacobian_kernel_ms(self):
        return self._lib.mrcal_amd_problem_last_jacobian_kernel_ms(self.handle)

    def synchronize(self):
        self._call("synchronize", "mrcal_amd_problem_synchronize")

    def jacobian_algorithmic_bytes(self):
        return int(self._lib.mrcal_amd_problem_jacobian_algorithmic_bytes(self.handle))

    def jacobian_timing_begin(self, capacity, stride=1):
        self._call("jacobian_timing_begin", "mrcal_amd_problem_jacobian_timing_begin_strided", int(capacity), int(stride))

    def jacobian_timing_end(self):
        """(Nlaunches, total_ms, min_ms, max_ms) of the Jacobian kernel since _begin()"""
        n = C.c_int(0); t = C.c_double(0); mn = C.c_double(0); mx = C.c_double(0)
        self._call("jacobian_timing_end", "mrcal_amd_problem_jacobian_timing_end", C.byref(n), C.byref(t), C.byref(mn), C.byref(mx))
        return n.value, t.value, mn.value, mx.value

    def dissection(self):
        """the nested-dissection order of a splined problem's camera block: dict(rounds, ns_max, active, nA, nB, nS) -
        rounds == 0: not in use (include/mrcal_amd.h)"""
        out = (C.c_int*9)()
        self._call("dissection", "mrcal_amd_problem_dissection", out)
        return dict(zip(("rounds", "ns_max", "active", "nA", "nB", "nS", "ideal_A", "ideal_B", "ideal_S"), [int(v) for v in out]))

    def set_jacobian_stream(self, stream):
        """stream=False: solve() / run_steps() do not write the CSR values of J to HBM in every step (nothing in the
        solve reads them; J() evaluates them on demand afterwards). The same bits in every result. Returns the previous
        setting (include/mrcal_amd.h)"""
        return bool(self._lib.mrcal_amd_problem_set_jacobian_stream(self.handle, 1 if stream else 0))

    def jacobian_stream_is_optional(self):
        return bool(self._lib.mrcal_amd_problem_jacobian_stream_is_optional(self.handle))

    def set_b_packed(self, b):
        b = np.ascontiguousarray(b, dtype=np.float64)
        assert b.shape == (self.Nstate,)
        self._call("set_b_packed", "mrcal_amd_problem_set_b_packed", _ptr(b))

    def b_packed(self):
        b = np.empty((self.Nstate,), dtype=np.float64)
        self._call("get_b_packed", "mrcal_amd_problem_get_b_packed", _ptr(b))
        return b

    def x(self):
        x = np.empty((self.Nmeas,), dtype=np.float64)
        self._call("get_x", "mrcal_amd_problem_get_x", _ptr(x))
        return x

    def J(self):
        import scipy.sparse
        P = np.empty((self.Nmeas+1,), dtype=np.int32)
        I = np.empty((self.Nnz,),     dtype=np.int32)
        X = np.empty((self.Nnz,),     dtype=np.float64)
        self._call("get_J", "mrcal_amd_problem_get_J", _ptr(P), _ptr(I), _ptr(X))
        return scipy.sparse.csr_matrix((X, I, P), shape=(self.Nmeas, self.Nstate))

    def stream(self):
        return self._lib.mrcal_amd_problem_stream(self.handle)

    # ---------------------------------------------------------------- solver
    def solve(self, max_iterations=0):
        """the whole solve (dog leg + outlier rejection); returns a stats dict.
        The solution stays resident: b_packed(), x()"""
        nout = C.c_int(0)
        rms = self._lib.mrcal_amd_problem_solve(self.handle, int(max_iterations), C.byref(nout))
        if rms < 0:
            raise _failed("mrcal_amd_problem_solve()", RuntimeError)
        st = self.solver_stats()
        st.update(rms_reproj_error__pixels=rms, Noutliers_board=nout.value)
        return st

    def run_steps(self, Nsteps, trustregion=None):
        """exactly Nsteps dog-leg steps; returns (steps done, trust region)"""
        tr = C.c_double(-1.0 if trustregion is None else float(trustregion))
        n = self._lib.mrcal_amd_problem_run_steps(self.handle, int(Nsteps), C.byref(tr))
        if n < 0:
            raise _failed("mrcal_amd_problem_run_steps()", RuntimeError)
        return n, tr.value

    def solver_stats(self):
        i = [C.c_int(0) for _ in range(4)]
        d = [C.c_double(0) for _ in range(3)]
        self._lib.mrcal_amd_problem_solver_stats(self.handle, *[C.byref(v) for v in i], *[C.byref(v) for v in d])
        return dict(Niterations=i[0].value, Nevaluations=i[1].value, Nfactorizations=i[2].value,
                    Noutlier_passes=i[3].value, norm2_x=d[0].value, lambda_=d[1].value, seconds=d[2].value)

    def factorization(self):
        """CHOLMOD_factorization of JtJ at the resident state (None if singular), from this problem's own normal
        equations: no atomics anywhere (include/mrcal_amd.h, mrcal_amd_factorization_create_from_problem)"""
        from ._factorization import CHOLMOD_factorization
        return CHOLMOD_factorization._from_problem(self)

    def normal_equations(self):
        """evaluates at the resident state; returns dict(A,Bt,D,g,norm2_x,+dims). Nie is S_split (== the partition()'s):
        the number of intrinsics + extrinsics variables when the frames are eliminated, of intrinsics variables alone
        when the extrinsics are (include/mrcal_amd.h)"""
        dims = (C.c_int*6)()
        self._call("get_normal_equations", "mrcal_amd_problem_get_normal_equations", None,None,None,None,None, dims)
        Nc, NE, NEb, Nfb, Nie, Nwarp = list(dims)
        A  = np.zeros((Nc,Nc)); Bt = np.zeros((NE,Nc)); D = np.zeros((NEb,6,6)); g = np.zeros((self.Nstate,))
        n2 = np.zeros((1,))
        self._call("get_normal_equations", "mrcal_amd_problem_get_normal_equations", _ptr(A), _ptr(Bt), _ptr(D), _ptr(g), _ptr(n2), dims)
        return dict(A=A, Bt=Bt, D=D, g=g, norm2_x=n2[0], Nc=Nc, NE=NE, NEb=NEb, Nfb=Nfb, Nie=Nie, Nwarp=Nwarp, **self.partition())

    def partition(self):
        """dict(S_split, S_shift, E_state0, eliminates): S index s is state s (s < S_split) or s + S_shift, E index
        e is state E_state0 + e; eliminates is 'frames' or 'extrinsics' (include/mrcal_amd.h)"""
        info = (C.c_int*4)()
        self._lib.mrcal_amd_problem_partition(self.handle, info)
        return dict(S_split=info[0], S_shift=info[1], E_state0=info[2], eliminates="extrinsics" if info[3] else "frames")

    def drt_cross_reprojection__dbpacked(self, icam_intrinsics=-1):
        """K (6,Nstate) of mrcal.drt_cross_reprojection__dbpacked() from the RESIDENT Jacobian at the current
        state: J never leaves the device"""
        K = np.zeros((6, self.Nstate))
        self._call("drt_cross_reprojection", "mrcal_amd_problem_drt_cross_reprojection",
                   -1 if icam_intrinsics is None else int(icam_intrinsics), _ptr(K))
        return K

    def gauss_newton_step(self):
        d = np.zeros((self.Nstate,))
        self._call("gauss_newton_step", "mrcal_amd_problem_gauss_newton_step", _ptr(d))
        return d

    def lchol_diag_ratio(self):
        """min / max of the diagonal of the big camera block's Cholesky factors over the last dog-leg pass; 1.0 where no
        such factorization ran (include/mrcal_amd.h)"""
        return float(self._lib.mrcal_amd_problem_lchol_diag_ratio(self.handle))

    def uses_sweep(self):
        """has this problem's big Cholesky gone over to the backward sweep (the automatic stable fallback, or the test hook)?"""
        return bool(self._lib.mrcal_amd_problem_uses_sweep(self.handle))
