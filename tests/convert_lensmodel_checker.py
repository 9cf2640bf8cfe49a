"""CHECKER for the lens-model fit and convert_lensmodel(): the reference's own sampled problem
(mrcal-convert-lensmodel:747-767) handed to the reference's compiled library (the ref_api fixture). No solver of its own:
x and J at any point are ref_api.optimizer_callback()'s, a solve from any start is ref_api.optimize()'s."""
import numpy as np


class CheckerInputs:
    """p (N,3), q (N,2), w (N,) or None, the target lens model, an intrinsics vector and a pose rt (6,) or None (no pose
    block at all), flags: optimize_core, apply_regularization. A point that takes no part (w <= 0, anything
    non-finite) is an outlier of the reference's: weight -1, with finite stand-ins for what is not finite"""

    def __init__(self, ref, p, q, w, lensmodel, intrinsics, rt, *, imagersize, optimize_core=True, apply_regularization=True):
        self.ref = ref
        p = np.array(p, dtype=float).reshape(-1, 3)
        q = np.array(q, dtype=float).reshape(-1, 2)
        N = len(p)
        w = np.ones(N) if w is None else np.array(w, dtype=float).reshape(N)
        bad = ~(np.isfinite(w) & (w > 0) & np.isfinite(p).all(axis=-1) & np.isfinite(q).all(axis=-1))
        p[bad] = (0., 0., 1.); q[bad] = 0.; w[bad] = -1.
        self.N, self.bad = N, bad
        idx = np.zeros((N, 3), dtype=np.int32)
        idx[:, 0] = np.arange(N)
        idx[:, 2] = -1 if rt is None else 0
        self.oi = dict(intrinsics=np.array(intrinsics, dtype=float).reshape(1, -1),
                       rt_cam_ref=None if rt is None else np.array(rt, dtype=float).reshape(1, 6),
                       rt_ref_frame=None, points=np.ascontiguousarray(p),
                       observations_board=None, indices_frame_camintrinsics_camextrinsics=None,
                       observations_point=np.ascontiguousarray(np.column_stack((q, w))),
                       indices_point_camintrinsics_camextrinsics=idx,
                       lensmodel=lensmodel, imagersizes=np.array(imagersize, dtype=np.int32).reshape(1, 2),
                       do_optimize_intrinsics_core=bool(optimize_core), do_optimize_intrinsics_distortions=True,
                       do_optimize_extrinsics=rt is not None, do_optimize_frames=False,
                       do_apply_regularization=bool(apply_regularization),
                       do_apply_outlier_rejection=False, verbose=False)

    def inputs(self, intrinsics=None, rt=None):
        oi = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in self.oi.items()}
        if intrinsics is not None: oi["intrinsics"] = np.array(intrinsics, dtype=float).reshape(1, -1)
        if rt is not None and oi["rt_cam_ref"] is not None: oi["rt_cam_ref"] = np.array(rt, dtype=float).reshape(1, 6)
        return oi

    def callback(self, intrinsics=None, rt=None):
        """(x, J packed (scipy CSR)) of the reference at the state given (None: the one it was made with)"""
        _, x, J, _ = self.ref.optimizer_callback(no_factorization=True, **self.inputs(intrinsics, rt))
        return x, J

    def cost(self, intrinsics=None, rt=None):
        """(x.x, the reference's rms_reproj_error__pixels: sqrt(x.x/Nmeasurements))"""
        x, _ = self.callback(intrinsics, rt)
        return float(x @ x), float(np.sqrt(x @ x/len(x)))

    def stationarity(self, intrinsics=None, rt=None):
        """|J^T x|_inf / (|J|_F |x|) from the reference's packed J and x"""
        x, J = self.callback(intrinsics, rt)
        Jd = J.toarray()
        return float(np.abs(Jd.T @ x).max()/(np.linalg.norm(Jd)*np.linalg.norm(x)))

    def optimize(self, intrinsics=None, rt=None):
        """the reference's own solve from a start: (stats, intrinsics (Nintrinsics,), rt (6,) or None)"""
        oi = self.inputs(intrinsics, rt)
        stats = self.ref.optimize(**oi)
        return stats, oi["intrinsics"][0].copy(), (None if oi["rt_cam_ref"] is None else oi["rt_cam_ref"][0].copy())


def sample_grid(dims, gridn, where, radius):
    """mrcal-convert-lensmodel:636-681 restated: the grid, then the pixels within the radius of the focus"""
    dims = np.asarray(dims)
    W, H = float(dims[0]), float(dims[1])
    cx, cy = (W - 1)/2, (H - 1)/2
    if radius is None:
        radius = -min(int(dims[0]), int(dims[1]))//4
    q = np.array([(x, y) for y in np.linspace(0, H - 1, gridn[1]) for x in np.linspace(0, W - 1, gridn[0])])
    if radius == 0:
        return q
    fx, fy = (cx, cy) if where is None else where
    r = radius if radius > 0 else np.hypot(W, H)/2 + radius
    return q[(q[:, 0] - fx)**2 + (q[:, 1] - fy)**2 < r*r]
