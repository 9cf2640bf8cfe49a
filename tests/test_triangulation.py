"""triangulate_*(): the six triangulation methods (mrcal_amd/csrc/triangulation_math.hpp, triangulation.hip,
mrcal_amd/triangulation.py) against the reference's own compiled mrcal_triangulate_*() (oracle/_ref).

Inputs, for every test: seeded true points 2-50 m in front of both cameras, baselines of 0.2-2 m with up to 15 degrees
of rotation between the cameras, pixels from the reference's mrcal_project() with up to 0.5 px of seeded noise, the
rays from the reference's mrcal_unproject(). Every 8th pair is DIVERGENT: its v0 and v1 are swapped (a near point,
so that the swapped rays open by more than 1 degree), and it shares a wavefront with convergent pairs. Nothing is left
out of a comparison: the reference's point must be nonzero for every convergent pair and exactly zero for every
divergent one (the inputs themselves are checked), and then all of them are compared.

Tolerance: 1e-6 of the largest magnitude in the array compared, the bar the project holds x and J to against the
compiled reference.

Without a GPU: the header built for the host (tests/hostcheck/triangulation_check.cpp). On the GPU: the kernels,
which must also give the host build's p to the bit."""
import ctypes as C
import os
import numpy as np
import pytest

import hostbuild

METHODS = dict(geometric=0, lindstrom=1, leecivera_l1=2, leecivera_linf=3, leecivera_mid2=4, leecivera_wmid2=5)
SIZES   = (1, 63, 64, 65, 257)
TOL     = 1e-6
LENSMODEL  = "LENSMODEL_OPENCV8"
INTRINSICS = np.array((1000., 1010., 1020., 760., -0.05, 0.02, 1e-4, -2e-4, 0.003, 0.01, -0.002, 0.001))


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _R_from_r(r):
    th = np.linalg.norm(r)
    if th < 1e-12: return np.eye(3)
    k = r/th
    K = np.array(((0., -k[2], k[1]), (k[2], 0., -k[0]), (-k[1], k[0], 0.)))
    return np.eye(3) + np.sin(th)*K + (1. - np.cos(th))*K @ K


def make_pairs(ref_api, N, seed):
    """N pairs, each with a geometry of its own. v0, v1: camera-0 coordinates; v1_local: camera 1's; Rt01 (N,4,3);
    divergent (N,) bool: every 8th pair (the 4th of each 8, so that N = 1 is convergent)"""
    rng = np.random.default_rng(seed)
    divergent = (np.arange(N) % 8) == 3
    Rt01 = np.zeros((N,4,3))
    p0   = np.zeros((N,3))
    for i in range(N):
        axis = rng.normal(size=3); axis /= np.linalg.norm(axis)
        Rt01[i,:3,:] = _R_from_r(axis*np.radians(rng.uniform(0., 15.)))
        # a mostly-lateral baseline: the parallax of a point at 50 m is then at least ~0.2/50 rad, about 4 px: the 0.5 px
        # of noise on each pixel cannot make a convergent pair diverge
        d = np.array((rng.choice((-1., 1.)), rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3)))
        Rt01[i,3,:] = d/np.linalg.norm(d)*(rng.uniform(0.5, 2.0) if divergent[i] else rng.uniform(0.2, 2.0))
        while True:
            rng_m = rng.uniform(2., 5.) if divergent[i] else rng.uniform(2., 50.)
            a, b  = np.radians(rng.uniform(-20., 20., size=2))
            p     = rng_m*np.array((np.tan(a), np.tan(b), 1.))/np.linalg.norm((np.tan(a), np.tan(b), 1.))
            p1    = Rt01[i,:3,:].T @ (p - Rt01[i,3,:])
            if p1[2] > 1.0 and np.all(np.abs(p1[:2]/p1[2]) < np.tan(np.radians(35.))): break
        p0[i] = p
    p1 = np.einsum("nji,nj->ni", Rt01[:,:3,:], p0 - Rt01[:,3,:])
    q0 = ref_api.project(p0, LENSMODEL, INTRINSICS) + rng.uniform(-0.5, 0.5, size=(N,2))
    q1 = ref_api.project(p1, LENSMODEL, INTRINSICS) + rng.uniform(-0.5, 0.5, size=(N,2))
    v0       = ref_api.unproject(q0, LENSMODEL, INTRINSICS)
    v1_local = ref_api.unproject(q1, LENSMODEL, INTRINSICS)
    assert np.all(np.isfinite(v0)) and np.all(np.isfinite(v1_local))
    v1 = np.einsum("nij,nj->ni", Rt01[:,:3,:], v1_local)
    # the divergent ones: the two rays trade places
    v0d, v1d = np.where(divergent[:,None], v1, v0), np.where(divergent[:,None], v0, v1)
    cos = np.einsum("ni,ni->n", v0d, v1d)/np.linalg.norm(v0d, axis=1)/np.linalg.norm(v1d, axis=1)
    assert np.all(np.degrees(np.arccos(cos[divergent])) > 1.0), "the divergent pairs must open by more than 1 degree"
    return dict(N=N, divergent=divergent, Rt01=Rt01, t01=np.ascontiguousarray(Rt01[:,3,:]), p_true=p0,
                v0=np.ascontiguousarray(v0d), v1=np.ascontiguousarray(v1d),
                v1_local=np.ascontiguousarray(np.einsum("nji,nj->ni", Rt01[:,:3,:], v1d)))


class Point3(C.Structure):
    _fields_ = [("x", C.c_double), ("y", C.c_double), ("z", C.c_double)]


def ref_triangulate_arrays(ref_api, method, a, b, c):
    """the reference's compiled mrcal_triangulate_<method>(), a pair at a time: p, dp_dv0, dp_dv1, dp_dt01 | dp_dRt01.
    a, b (N,3): v0, v1 (lindstrom: both local); c: t01 (N,3), or lindstrom's Rt01 (N,4,3)"""
    f = getattr(ref_api.clib, "mrcal_triangulate_" + method)
    f.restype, f.argtypes = Point3, [C.c_void_p]*6   # (the point comes back by value)
    a, b, c = (np.ascontiguousarray(x, dtype=float) for x in (a, b, c))
    N = a.shape[0]
    p, g0, g1, gp = np.zeros((N,3)), np.zeros((N,3,3)), np.zeros((N,3,3)), np.zeros((N,3) + c.shape[1:])
    for i in range(N):
        r = f(_ptr(g0[i]), _ptr(g1[i]), _ptr(gp[i]), _ptr(a[i]), _ptr(b[i]), _ptr(c[i]))
        p[i] = (r.x, r.y, r.z)
    # where the reference returns (0,0,0) it leaves the gradients alone: they stayed zero
    return p, g0, g1, gp


def ref_triangulate(ref_api, method, pairs):
    return ref_triangulate_arrays(ref_api, method, *method_inputs(method, pairs))


@pytest.fixture(scope="module")
def hostlib():
    L = C.CDLL(hostbuild.build_library("triangulation_check"))
    L.tricheck_eval.restype,          L.tricheck_eval.argtypes          = C.c_int, [C.c_int]*3 + [C.c_void_p]*7
    L.tricheck_eval_double.restype,   L.tricheck_eval_double.argtypes   = C.c_int, [C.c_int]*2 + [C.c_void_p]*4
    L.tricheck_is_convergent.restype, L.tricheck_is_convergent.argtypes = None, [C.c_int] + [C.c_void_p]*4
    return L


def host_triangulate(L, method, v0, v1, pose, with_grad=True):
    """the host build of triangulation_math.hpp. pose: t01 (N,3), or for lindstrom Rt01 (N,4,3)"""
    v0, v1, pose = (np.ascontiguousarray(a, dtype=float) for a in (v0, v1, pose))
    N = v0.shape[0]
    p, g0, g1, gp = np.zeros((N,3)), np.zeros((N,3,3)), np.zeros((N,3,3)), np.zeros((N,3) + pose.shape[1:])
    assert L.tricheck_eval(METHODS[method], int(with_grad), N, _ptr(v0), _ptr(v1), _ptr(pose),
                           _ptr(p), _ptr(g0), _ptr(g1), _ptr(gp)) == 0
    return (p, g0, g1, gp) if with_grad else p


def method_inputs(method, pairs):
    if method == "lindstrom": return pairs["v0"], pairs["v1_local"], pairs["Rt01"]
    return pairs["v0"], pairs["v1"], pairs["t01"]


@pytest.fixture(scope="module")
def cases(ref_api):
    """size -> (pairs, {method: the reference's p and gradients}): made once, read by every test"""
    out = {}
    for N in SIZES:
        pairs = make_pairs(ref_api, N, seed=1000 + N)
        refs  = {m: ref_triangulate(ref_api, m, pairs) for m in METHODS}
        for a in pairs.values():
            if isinstance(a, np.ndarray): a.setflags(write=False)
        for r in refs.values():
            for a in r: a.setflags(write=False)
        out[N] = (pairs, refs)
    return out


def assert_inputs_are_what_they_claim(pairs, p_ref):
    """the reference triangulates every convergent pair and refuses every divergent one"""
    nonzero = np.any(p_ref != 0., axis=1)
    assert np.all(nonzero[~pairs["divergent"]]), "the reference returned (0,0,0) for a convergent pair"
    assert not np.any(nonzero[pairs["divergent"]]), "the reference triangulated a divergent pair"


def worst(a, ref):
    """largest difference, relative to the largest magnitude in the reference array"""
    return np.abs(a - ref).max()/np.abs(ref).max()


@pytest.mark.parametrize("method", METHODS)
def test_the_committed_seeds_do_what_the_tests_say(cases, method):
    for N in SIZES:
        pairs, refs = cases[N]
        assert pairs["divergent"].sum() == (N + 4)//8
        assert_inputs_are_what_they_claim(pairs, refs[method][0])
        # and the convergent ones are where the points were put, to the noise: up to 1 px on a disparity of 3.7 or more
        ok = ~pairs["divergent"]
        err = np.linalg.norm(refs[method][0][ok] - pairs["p_true"][ok], axis=1)/np.linalg.norm(pairs["p_true"][ok], axis=1)
        assert err.max() < 0.5


@pytest.mark.parametrize("method", METHODS)
def test_host_methods_against_the_reference(hostlib, cases, method):
    for N in SIZES:
        pairs, refs = cases[N]
        assert_inputs_are_what_they_claim(pairs, refs[method][0])
        got = host_triangulate(hostlib, method, *method_inputs(method, pairs))
        for name, a, r in zip(("p", "dp_dv0", "dp_dv1", "dp_dpose"), got, refs[method]):
            e = worst(a, r)
            print(f"host {method} N={N} {name}: {e:.3g}")
            assert e < TOL, (method, N, name)
        # a refused pair: the point and every gradient exactly zero
        for a in got: assert not np.any(a[pairs["divergent"]])
        # the point is the same with and without the gradients, to the bit
        assert np.array_equal(host_triangulate(hostlib, method, *method_inputs(method, pairs), with_grad=False), got[0])


@pytest.mark.parametrize("method", METHODS)
def test_host_methods_on_plain_doubles(hostlib, cases, method):
    """the header's other scalar"""
    pairs, refs = cases[65]
    v0, v1, pose = (np.ascontiguousarray(a) for a in method_inputs(method, pairs))
    p = np.zeros((65,3))
    assert hostlib.tricheck_eval_double(METHODS[method], 65, _ptr(v0), _ptr(v1), _ptr(pose), _ptr(p)) == 0
    assert worst(p, refs[method][0]) < TOL
    assert not np.any(p[pairs["divergent"]])


def test_host_is_convergent_against_the_reference(hostlib, ref_api, cases):
    pairs, refs = cases[257]
    f = ref_api.clib._mrcal_triangulate_leecivera_mid2_is_convergent
    f.restype, f.argtypes = C.c_bool, [C.c_void_p]*3
    ref = np.array([f(_ptr(pairs["v0"][i]), _ptr(pairs["v1"][i]), _ptr(pairs["t01"][i])) for i in range(257)])
    got = np.zeros(257, dtype=np.int32)
    hostlib.tricheck_is_convergent(257, _ptr(pairs["v0"]), _ptr(pairs["v1"]), _ptr(pairs["t01"]), _ptr(got))
    assert np.array_equal(ref, ~pairs["divergent"])
    assert np.array_equal(got.astype(bool), ref)


@pytest.mark.parametrize("method", METHODS)
def test_host_gradients_against_central_differences(hostlib, cases, method):
    """Step h = 1e-6 on inputs of order 1. The point is ~ b/th with the parallax th >= 4e-3 rad, its gradient ~ p/th.
    Relative to that gradient a central difference is off by (h/th)^2 = 6e-8 of truncation, and by the rounding of p
    over 2h: p carries a few 1e-16/th^2 in the worst method (geometric: its denominator cancels to th^2), which is a
    few times 1e-16/(th h) = 3e-8. 1e-6 of the largest entry of a pair's gradient leaves about a tenfold margin"""
    pairs, _ = cases[65]
    v0, v1, pose = (np.array(a) for a in method_inputs(method, pairs))
    got = host_triangulate(hostlib, method, v0, v1, pose)
    h = 1e-6
    for iarg, g in ((0, got[1]), (1, got[2]), (2, got[3])):
        g  = g.reshape(65, 3, -1)
        fd = np.zeros_like(g)
        for k in range(g.shape[2]):
            args_p, args_m = [v0.copy(), v1.copy(), pose.copy()], [v0.copy(), v1.copy(), pose.copy()]
            args_p[iarg].reshape(65,-1)[:,k] += h
            args_m[iarg].reshape(65,-1)[:,k] -= h
            fd[:,:,k] = (host_triangulate(hostlib, method, *args_p, with_grad=False) -
                         host_triangulate(hostlib, method, *args_m, with_grad=False))/(2.*h)
        scale = np.abs(g).reshape(65,-1).max(axis=1)
        ok = ~pairs["divergent"]
        assert np.all(scale[ok] > 0.)
        e = (np.abs(fd - g).reshape(65,-1).max(axis=1)[ok]/scale[ok]).max()
        print(f"host {method} gradient {iarg} against differences: {e:.3g}")
        assert e < TOL
        assert not np.any(fd[~ok])


def test_parse_args_exceptions(amd):
    v, t, Rt = np.array((0., 0., 1.)), np.array((1., 0., 0.)), np.vstack((np.eye(3), (1., 0., 0.)))
    for f in (amd.triangulate_geometric, amd.triangulate_leecivera_l1, amd.triangulate_leecivera_linf,
              amd.triangulate_leecivera_mid2, amd.triangulate_leecivera_wmid2):
        with pytest.raises(Exception, match="Exactly one of Rt01 and t01 must be None. Both were non-None"):
            f(v, v, t, Rt01=Rt)
        with pytest.raises(Exception, match="Exactly one of Rt01 and t01 must be None. Both were None"):
            f(v, v)
        with pytest.raises(Exception, match="get_gradients is True, so v_are_local MUST be the default: False"):
            f(v, v, Rt01=Rt, v_are_local=True, get_gradients=True)
        with pytest.raises(Exception, match="v_are_local is True, so Rt01 MUST have been given"):
            f(v, v, t, v_are_local=True)
        with pytest.raises(Exception, match="get_gradients is True, so t01 MUST have been given"):
            f(v, v, Rt01=Rt, get_gradients=True)
    with pytest.raises(Exception, match="get_gradients is True, so v_are_local MUST be True"):
        amd.triangulate_lindstrom(v, v, Rt, v_are_local=False, get_gradients=True)


# ---------------------------------------------------------------------------------------------------------------------
# on the GPU

def device_function(amd, method):
    return getattr(amd, "triangulate_" + method)


def device_triangulate(amd, method, pairs, get_gradients):
    return device_function(amd, method)(*method_inputs(method, pairs), get_gradients=get_gradients)


@pytest.mark.gpu
@pytest.mark.parametrize("method", METHODS)
def test_device_methods_against_the_reference(amd, hostlib, cases, method):
    for N in SIZES:
        pairs, refs = cases[N]
        assert_inputs_are_what_they_claim(pairs, refs[method][0])
        got = device_triangulate(amd, method, pairs, True)
        assert got[3].shape == ((N,3,4,3) if method == "lindstrom" else (N,3,3))
        for name, a, r in zip(("p", "dp_dv0", "dp_dv1", "dp_dpose"), got, refs[method]):
            e = worst(a, r)
            print(f"device {method} N={N} {name}: {e:.3g}")
            assert e < TOL, (method, N, name)
        for a in got: assert not np.any(a[pairs["divergent"]])
        # without gradients: the same point, to the bit; and the same bits on a second call
        p = device_triangulate(amd, method, pairs, False)
        assert p.shape == (N,3) and np.array_equal(p, got[0])
        again = device_triangulate(amd, method, pairs, True)
        for a, b in zip(got, again): assert np.array_equal(a, b)
        # the host build of the same header: p to the bit
        assert np.array_equal(host_triangulate(hostlib, method, *method_inputs(method, pairs), with_grad=False), p)


@pytest.mark.gpu
@pytest.mark.parametrize("method", METHODS)
def test_device_local_vectors_and_Rt01_against_the_t01_form(amd, cases, method):
    pairs, refs = cases[65]
    f = device_function(amd, method)
    if method == "lindstrom":
        p_local = f(pairs["v0"], pairs["v1_local"], pairs["Rt01"])
        p_cam0  = f(pairs["v0"], pairs["v1"], pairs["Rt01"], v_are_local=False)
    else:
        p_cam0  = f(pairs["v0"], pairs["v1"], pairs["t01"])
        p_local = f(pairs["v0"], pairs["v1_local"], Rt01=pairs["Rt01"], v_are_local=True)
        assert np.array_equal(f(pairs["v0"], pairs["v1"], Rt01=pairs["Rt01"]), p_cam0)
    # (v1 goes through one more rotation in one of the two: the reference's point bounds both)
    assert worst(p_local, refs[method][0]) < TOL and worst(p_cam0, refs[method][0]) < TOL
    assert not np.any(p_local[pairs["divergent"]]) and not np.any(p_cam0[pairs["divergent"]])


@pytest.mark.gpu
@pytest.mark.parametrize("method", METHODS)
def test_device_broadcasting_and_out(amd, cases, method):
    pairs, _ = cases[65]
    f = device_function(amd, method)
    lind = method == "lindstrom"
    v0 = pairs["v0"][:5].reshape(5,1,3)
    v1 = (pairs["v1_local"] if lind else pairs["v1"])[8:12]                 # (4,3)
    pose = pairs["Rt01"][0] if lind else pairs["t01"][0]
    p, g0, g1, gp = f(v0, v1, pose, get_gradients=True)
    assert p.shape == (5,4,3) and g0.shape == (5,4,3,3) and g1.shape == (5,4,3,3)
    assert gp.shape == ((5,4,3,4,3) if lind else (5,4,3,3))
    for i in range(5):
        for j in range(4):
            one = f(v0[i,0], v1[j], pose, get_gradients=True)
            assert one[0].shape == (3,)
            for a, b in zip((p, g0, g1, gp), one): assert np.array_equal(a[i,j], b)
    # out=: filled and returned; a view that is not contiguous
    big = np.full((5,4,6), -1.)
    r = f(v0, v1, pose, out=big[...,::2])
    assert np.array_equal(big[...,::2], p) and np.all(big[...,1::2] == -1.) and r.base is big
    outs = tuple(np.zeros_like(a) for a in (p, g0, g1, gp))
    r = f(v0, v1, pose, get_gradients=True, out=outs)
    assert all(a is b for a, b in zip(r, outs))
    for a, b in zip(outs, (p, g0, g1, gp)): assert np.array_equal(a, b)


@pytest.mark.gpu
def test_device_buffers_are_given_back(amd, cases):
    pairs, _ = cases[65]
    before = amd.device_buffers_live()
    for method in METHODS: device_triangulate(amd, method, pairs, True)
    assert amd.device_buffers_live() == before


# =====================================================================================================================
# triangulate(): pixel pairs through camera models, with the noise propagated
#
# The checker is the reference's flow restated in numpy on the reference's compiled code: mrcal_unproject() and
# mrcal_project() (the gradients of an unprojection are those of the projection at the solution, as the reference's
# unproject(get_gradients = True) derives them), mrcal_triangulate_*(), J from optimizer_callback(); the pose
# arithmetic is mrcal_amd.poseutils (numpy) with the gradients by the closed forms below, which are checked against
# differences first.

from mrcal_amd.synthetic import make_calibration_problem, copy_inputs, intrinsics_for, IMAGERSIZE

from conftest import GOLDEN_DIR
COV_TOL    = 1e-6       # of the matrix's largest entry


def skew(r):
    return np.array(((0., -r[2], r[1]), (r[2], 0., -r[0]), (-r[1], r[0], 0.)))


def R_and_dR(r):
    """Rodrigues: R (3,3) and dR[i,j,k] = dR_ij/dr_k, from R = I + a K + b K^2, K = skew(r), a = sin(th)/th,
    b = (1 - cos(th))/th^2"""
    r = np.asarray(r, dtype=float)
    K, th2 = skew(r), r @ r
    G = np.stack([skew(e) for e in np.eye(3)], axis=-1)              # G[:,:,k] = dK/dr_k
    GK = np.einsum('ijk,jl->ilk', G, K) + np.einsum('ij,jlk->ilk', K, G)
    if th2 < 1e-16:
        return np.eye(3) + K + K @ K/2., G + GK/2.
    th = np.sqrt(th2)
    s, c = np.sin(th), np.cos(th)
    a, b = s/th, (1. - c)/th2
    da, db = (th*c - s)/th2, (th*s - 2.*(1. - c))/(th2*th)          # da/dth, db/dth; dth/dr_k = r_k/th
    R  = np.eye(3) + a*K + b*K @ K
    dR = a*G + b*GK + np.einsum('ij,k->ijk', da*K + db*K @ K, r/th)
    return R, dR


def rt01_and_gradients(amd, rt0, rt1):
    """rt01 = compose_rt(rt_0ref, invert_rt(rt_1ref)) (the repo's poseutils), and drt01/drt_0ref, drt01/drt_1ref (6,6)
    in closed form: R01 = R0 R1^T, t01 = t0 - R01 t1, and dr01 from dR01 through the pseudo-inverse of dR/dr at r01
    (R(r) is an immersion: a tangent dR01 is in the column space of dR/dr exactly)"""
    rt01 = amd.compose_rt(rt0, amd.invert_rt(rt1))
    (R0, dR0), (R1, dR1) = R_and_dR(rt0[:3]), R_and_dR(rt1[:3])
    R01 = R0 @ R1.T
    P = np.linalg.pinv(R_and_dR(rt01[:3])[1].reshape(9,3))
    dR01_dr0 = np.einsum('ijk,lj->ilk', dR0, R1)
    dR01_dr1 = np.einsum('ij,ljk->ilk', R0, dR1)
    d0, d1 = np.zeros((6,6)), np.zeros((6,6))
    d0[:3,:3] = P @ dR01_dr0.reshape(9,3)
    d1[:3,:3] = P @ dR01_dr1.reshape(9,3)
    d0[3:,:3] = -np.einsum('ilk,l->ik', dR01_dr0, rt1[3:])
    d1[3:,:3] = -np.einsum('ilk,l->ik', dR01_dr1, rt1[3:])
    d0[3:,3:] = np.eye(3)
    d1[3:,3:] = -R01
    return rt01, d0, d1


def ref_unproject_with_gradients(ref_api, q, lensmodel, intrinsics):
    """v (N,3), dv/dq (N,3,2), dv/dintrinsics (N,3,Ni) as the reference's unproject(get_gradients = True) derives
    them: v re-expressed as the stereographic representative (u, 1 - |u|^2/4) of its direction, and with the
    gradients of mrcal_project() there dv/dq = dv/du inv(dq/du), dv/dintrinsics = -dv/dq dq/dintrinsics.
    (A triangulated point does not depend on the length of v, so any representative gives the same dp/dq, dp/db)"""
    v = ref_api.unproject(np.ascontiguousarray(q), lensmodel, intrinsics)
    u = v[:,:2]*(2./(np.linalg.norm(v, axis=1) + v[:,2]))[:,None]
    v = np.column_stack((u, 1. - np.sum(u*u, axis=1)/4.))
    _, dq_dv, dq_di = ref_api.project(v, lensmodel, intrinsics, get_gradients=True)
    dv_du = np.zeros((len(v),3,2))
    dv_du[:,0,0] = dv_du[:,1,1] = 1.
    dv_du[:,2,:] = -u/2.
    dv_dq = dv_du @ np.linalg.inv(dq_dv @ dv_du)
    return v, dv_dq, -dv_dq @ dq_di


def test_closed_form_pose_gradients_against_differences(amd):
    """the checker's own closed forms: 1e-7 of the largest entry (central differences of step 1e-6 on smooth functions
    of order 1: truncation 1e-12, rounding 1e-10)"""
    rng = np.random.default_rng(5)
    h = 1e-6
    def differences(f, x):
        cols = []
        for k in range(len(x)):
            d = np.zeros(len(x)); d[k] = h
            cols.append((f(x + d) - f(x - d))/(2.*h))
        return np.stack(cols, axis=-1)
    for r in (rng.uniform(-0.3, 0.3, 3), rng.uniform(-1.5, 1.5, 3), np.zeros(3), np.array((1e-9, 0., 0.))):
        R, dR = R_and_dR(r)
        assert np.abs(R - amd.R_from_r(r)).max() < 1e-14
        assert np.abs(dR - differences(lambda x: R_and_dR(x)[0], r)).max() < 1e-7
    for rt0, rt1 in ((rng.uniform(-0.3, 0.3, 6), rng.uniform(-0.3, 0.3, 6)), (np.zeros(6), rng.uniform(-0.1, 0.1, 6)),
                     (rng.uniform(-1., 1., 6), rng.uniform(-1., 1., 6))):
        rt01, d0, d1 = rt01_and_gradients(amd, rt0, rt1)
        assert np.abs(d0 - differences(lambda x: amd.compose_rt(x, amd.invert_rt(rt1)), rt0)).max() < 1e-7*np.abs(d0).max()
        assert np.abs(d1 - differences(lambda x: amd.compose_rt(rt0, amd.invert_rt(x)), rt1)).max() < 1e-7*np.abs(d1).max()
        assert np.abs(amd.R_from_r(rt01[:3]) - amd.R_from_r(rt0[:3]) @ amd.R_from_r(rt1[:3]).T).max() < 1e-14


def test_ref_unproject_gradients_against_differences(ref_api):
    """... and the restated unprojection gradients, through a quantity that does not depend on the representative:
    the unit vector"""
    rng = np.random.default_rng(6)
    q = np.array((2000., 1100.)) + rng.uniform(-600., 600., size=(5,2))
    intr = INTRINSICS*np.array((1.7,1.7,1.95,1.45) + (1.,)*8)
    unit = lambda v: v/np.linalg.norm(v, axis=-1, keepdims=True)
    v, dv_dq, dv_di = ref_unproject_with_gradients(ref_api, q, LENSMODEL, intr)
    Pn = (np.eye(3) - unit(v)[:,:,None]*unit(v)[:,None,:])/np.linalg.norm(v, axis=1)[:,None,None]
    for k in range(2):
        d = np.zeros(2); d[k] = 1e-3
        fd = (unit(ref_api.unproject(q + d, LENSMODEL, intr)) - unit(ref_api.unproject(q - d, LENSMODEL, intr)))/2e-3
        assert np.abs((Pn @ dv_dq)[:,:,k] - fd).max() < 1e-6*np.abs(fd).max()
    for k in (0, 3, 5, 11):
        d = np.zeros(12); d[k] = 1e-4*max(1., abs(intr[k]))
        fd = (unit(ref_api.unproject(q, LENSMODEL, intr + d)) - unit(ref_api.unproject(q, LENSMODEL, intr - d)))/(2.*d[k])
        assert np.abs((Pn @ dv_di)[:,:,k] - fd).max() < 1e-5*np.abs(fd).max()


@pytest.mark.parametrize("correlation", (0., 0.3, 1.))
def test_Var_q_triangulation(amd, correlation):
    from mrcal_amd.triangulation import _compute_Var_q_triangulation
    s = 0.7
    V = _compute_Var_q_triangulation(s, correlation)
    # q0x, q0y, q1x, q1y: independent in x and y; the same coordinate of the two cameras correlated
    c = (s*correlation)**2
    assert np.array_equal(V, np.array(((s*s, 0., c, 0.), (0., s*s, 0., c), (c, 0., s*s, 0.), (0., c, 0., s*s))))


def test_triangulate_refusals_before_any_device_work(amd, ref_api, monkeypatch):
    import mrcal_amd.resident as resident
    def no_device(*a, **k): raise AssertionError("device work before the refusal")
    monkeypatch.setattr(resident.Problem, "__init__", no_device)
    monkeypatch.setattr(amd.Triangulation, "__init__", no_device)
    oi, _  = make_calibration_problem(ref_api, Ncameras=2, Nframes=6, seed=3)
    oi2, _ = make_calibration_problem(ref_api, Ncameras=2, Nframes=6, seed=4)
    m = [amd.cameramodel(optimization_inputs=oi, icam_intrinsics=i) for i in range(2)]
    q = np.array(((2000., 1100.), (1900., 1100.)))
    with pytest.raises(Exception, match="q_observation_stdev MUST be None or >= 0"):
        amd.triangulate(q, m, q_observation_stdev=-1.)
    bare = amd.cameramodel(m[0]); bare.optimization_inputs_reset()
    with pytest.raises(Exception, match="optimization_inputs are not available, so I cannot propagate calibration-time noise"):
        amd.triangulate(q, (bare, m[1]), q_calibration_stdev=1.)
    other = amd.cameramodel(optimization_inputs=oi2, icam_intrinsics=1)
    with pytest.raises(Exception, match="The optimization_inputs for all of the given models must be identical"):
        amd.triangulate(q, (m[0], other), q_calibration_stdev=1.)
    moved = amd.cameramodel(m[1]); rt = moved.rt_cam_ref().copy(); rt[3] += 0.01; moved.rt_cam_ref(rt)
    with pytest.raises(Exception, match="The given models must have been fixed inside the initial calibration. Model 1 has been moved"):
        amd.triangulate(q, (m[0], moved), q_calibration_stdev=-1.)
    for kw in (dict(q_calibration_stdev=1.), dict(q_observation_stdev=1.), dict(q_calibration_stdev=-1., q_observation_stdev=0.)):
        with pytest.raises(Exception, match="Triangulation gradients not supported .yet.. with method=triangulate_lindstrom"):
            amd.triangulate(q, m, method=amd.triangulate_lindstrom, **kw)
    with pytest.raises(Exception, match="method must be one of"):
        amd.triangulate(q, m, method=np.sum)
    with pytest.raises(Exception, match="models must have shape"):
        amd.triangulate(q, (m[0], m[1], m[0]))


# ---------------------------------------------------------------------------------------------------------------------
def make_pixel_pairs(amd, ref_api, cameras, pair_cameras, seed):
    """Pixel pairs for triangulate(). cameras: [(lensmodel, intrinsics, rt_cam_ref)]; pair_cameras (N,2): which two
    see each pair. True points 2-50 m in front of both, up to 0.5 px of noise; every 8th pair (the 4th of 8)
    divergent: a near point whose two rays trade places. -> q (N,2,2), divergent (N,)"""
    rng = np.random.default_rng(seed)
    N = len(pair_cameras)
    divergent = (np.arange(N) % 8) == 3
    q = np.zeros((N,2,2))
    for i, (c0, c1) in enumerate(pair_cameras):
        (lm0, in0, rt0), (lm1, in1, rt1) = cameras[c0], cameras[c1]
        rt01 = amd.compose_rt(rt0, amd.invert_rt(rt1))
        R01, t01 = amd.R_from_r(rt01[:3]), rt01[3:]
        while True:
            rng_m = rng.uniform(2., 5.) if divergent[i] else rng.uniform(2., 50.)
            a, b  = np.radians(rng.uniform(-15., 15., size=2))
            p0 = np.array((np.tan(a), np.tan(b), 1.)); p0 *= rng_m/np.linalg.norm(p0)
            p1 = R01.T @ (p0 - t01)
            if p1[2] > 1.0 and np.all(np.abs(p1[:2]/p1[2]) < np.tan(np.radians(30.))): break
        if divergent[i]:
            # camera 0 looks along camera 1's ray, camera 1 along camera 0's
            p0, p1 = R01 @ p1, R01.T @ p0
        q[i,0] = ref_api.project(p0, lm0, in0)
        q[i,1] = ref_api.project(p1, lm1, in1)
    return q + rng.uniform(-0.5, 0.5, size=q.shape), divergent


def unprojected_pairs(amd, ref_api, cameras, pair_cameras, q, with_intrinsics_gradients=False):
    """What of the composed flow does not depend on the method, made once: every pixel unprojected by the reference's
    compiled mrcal_unproject() (each camera's in one call), the gradients from its mrcal_project(), and the numpy
    pose arithmetic of each pair"""
    N = len(q)
    pc = np.asarray(pair_cameras).reshape(N,2)
    v_plain, v, dv_dq, dv_di = np.zeros((N,2,3)), np.zeros((N,2,3)), np.zeros((N,2,3,2)), [[None, None] for _ in range(N)]
    for c, (lm, intr, _) in enumerate(cameras):
        sel = np.nonzero(pc == c)
        if len(sel[0]) == 0: continue
        v_plain[sel] = ref_api.unproject(np.ascontiguousarray(q[sel]), lm, intr)
        vv, gq, gi = ref_unproject_with_gradients(ref_api, q[sel], lm, intr)
        v[sel], dv_dq[sel] = vv, gq
        if with_intrinsics_gradients:
            for k, (i, slot) in enumerate(zip(*sel)): dv_di[i][slot] = gi[k]
    pairs = []
    for i, (c0, c1) in enumerate(pc):
        rt01, drt01_drt0, drt01_drt1 = rt01_and_gradients(amd, cameras[c0][2], cameras[c1][2])
        R01, dR01 = R_and_dR(rt01[:3])
        pairs.append(dict(rt01=rt01, R01=R01, dR01=dR01, drt01_drt0=drt01_drt0, drt01_drt1=drt01_drt1,
                          v_plain=v_plain[i], v=v[i], dv_dq=dv_dq[i], dv_di=dv_di[i]))
    return pairs


def composed_flow(ref_api, pairs, method, q_observation_stdev=None, correlation=0.):
    """triangulate() without calibration-time noise, restated on unprojected_pairs(): the reference's compiled
    mrcal_triangulate_<method>() on its unprojections.
    -> p (N,3), Var_p_observation (N,3,3) or None, and the pieces the calibration checker goes on from"""
    from mrcal_amd.triangulation import _compute_Var_q_triangulation
    N = len(pairs)
    if q_observation_stdev is None:
        v0, vl1 = np.array([g["v_plain"][0] for g in pairs]), np.array([g["v_plain"][1] for g in pairs])
        if method == "lindstrom":
            return ref_triangulate_arrays(ref_api, method, v0, vl1, np.array([np.vstack((g["R01"], g["rt01"][3:])) for g in pairs]))[0], None, None
        v1 = np.array([g["R01"] @ g["v_plain"][1] for g in pairs])
        return ref_triangulate_arrays(ref_api, method, v0, v1, np.array([g["rt01"][3:] for g in pairs]))[0], None, None
    v0, vl1 = np.array([g["v"][0] for g in pairs]), np.array([g["v"][1] for g in pairs])
    v1 = np.array([g["R01"] @ g["v"][1] for g in pairs])
    p, dp_dv0, dp_dv1, dp_dt01 = ref_triangulate_arrays(ref_api, method, v0, v1, np.array([g["rt01"][3:] for g in pairs]))
    Var_q = _compute_Var_q_triangulation(q_observation_stdev, correlation)
    Var, pieces = np.zeros((N,3,3)), []
    for i, g in enumerate(pairs):
        dp_dq = np.hstack((dp_dv0[i] @ g["dv_dq"][0], dp_dv1[i] @ g["R01"] @ g["dv_dq"][1]))
        Var[i] = dp_dq @ Var_q @ dp_dq.T
        pieces.append(dict(p=p[i], dp_dv0=dp_dv0[i], dp_dv1=dp_dv1[i], dp_dt01=dp_dt01[i], R01=g["R01"],
                           dv0_di=g["dv_di"][0], dvl1_di=g["dv_di"][1], dv1_dr01=np.einsum('ijk,j->ik', g["dR01"], vl1[i]),
                           drt01_drt0=g["drt01_drt0"], drt01_drt1=g["drt01_drt1"]))
    return p, Var, pieces


def check_points(p_ref, divergent):
    nonzero = np.any(p_ref != 0., axis=-1)
    assert np.all(nonzero[~divergent]), "the reference returned (0,0,0) for a convergent pair"
    assert not np.any(nonzero[divergent]), "the reference triangulated a divergent pair"


def lens_cameras(amd):
    """four cameras of four lens models, 0.2-2 m and up to 15 degrees apart"""
    rng = np.random.default_rng(77)
    spl = amd.cameramodel(os.path.join(GOLDEN_DIR, "real_splined-0.cameramodel"))
    models = [("LENSMODEL_OPENCV8", intrinsics_for("LENSMODEL_OPENCV8", 1)[0]), spl.intrinsics(),
              ("LENSMODEL_CAHVORE_linearity=0.37", np.concatenate((intrinsics_for("LENSMODEL_CAHVORE_linearity=0.37", 1)[0][:9], np.zeros(3)))),
              ("LENSMODEL_STEREOGRAPHIC", intrinsics_for("LENSMODEL_STEREOGRAPHIC", 1)[0])]
    cameras, x = [], 0.
    for lm, intr in models:
        axis = rng.normal(size=3); axis /= np.linalg.norm(axis)
        r = axis*np.radians(rng.uniform(0., 7.))          # any two are then at most 14 degrees apart
        t_ref_cam = np.array((x, rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05)))
        cameras.append((lm, np.array(intr, dtype=float), np.concatenate((r, -amd.R_from_r(r) @ t_ref_cam))))
        x += rng.uniform(0.25, 0.6)
    return cameras


def as_models(amd, cameras):
    return [amd.cameramodel(intrinsics=(lm, intr), imagersize=IMAGERSIZE, rt_cam_ref=rt) for lm, intr, rt in cameras]


@pytest.mark.gpu
@pytest.mark.parametrize("N", SIZES)
def test_triangulate_without_noise_and_with_observation_noise(amd, ref_api, N):
    cameras = lens_cameras(amd)
    models  = as_models(amd, cameras)
    # mixed models in one call: every ordered pair of different cameras in turn
    kinds = [(a, b) for a in range(4) for b in range(4) if a != b]
    pair_cameras = [kinds[i % len(kinds)] for i in range(N)]
    q, divergent = make_pixel_pairs(amd, ref_api, cameras, pair_cameras, seed=2000 + N)
    pair_models  = np.array([[models[a], models[b]] for a, b in pair_cameras], dtype=object)
    pairs = unprojected_pairs(amd, ref_api, cameras, pair_cameras, q)
    with amd.Triangulation(pair_models) as t:
        for method in METHODS:
            f = device_function(amd, method)
            p_ref, _, _ = composed_flow(ref_api, pairs, method)
            check_points(p_ref, divergent)
            p = t.triangulate(q, method=f)
            assert p.shape == (N,3)
            e = worst(p, p_ref)
            print(f"triangulate() {method} N={N} p: {e:.3g}")
            assert e < TOL and not np.any(p[divergent])
            assert np.array_equal(p, amd.triangulate(q, pair_models, method=f))          # one-shot == reused, to the bit
            if method == "lindstrom": continue
            for corr in (0., 0.7):
                p_ref, Var_ref, _ = composed_flow(ref_api, pairs, method, 0.4, corr)
                check_points(p_ref, divergent)
                p, Var = t.triangulate(q, method=f, q_observation_stdev=0.4, q_observation_stdev_correlation=corr)
                assert Var.shape == (N,3,3)
                ep = worst(p, p_ref)
                ev = max(np.abs(Var[i] - Var_ref[i]).max()/np.abs(Var_ref[i]).max() for i in np.nonzero(~divergent)[0])
                print(f"triangulate() {method} N={N} correlation {corr}: p {ep:.3g}, Var_p_observation {ev:.3g}")
                assert ep < TOL and ev < COV_TOL
                assert not np.any(p[divergent]) and not np.any(Var[divergent]) and not np.any(Var_ref[divergent])
                assert np.array_equal(Var, np.swapaxes(Var, -1, -2))
                assert np.linalg.eigvalsh(Var).min() >= -1e-12*np.abs(Var).max()
                again = t.triangulate(q, method=f, q_observation_stdev=0.4, q_observation_stdev_correlation=corr)
                assert np.array_equal(again[0], p) and np.array_equal(again[1], Var)


@pytest.mark.gpu
def test_triangulate_broadcasting_and_return_shapes(amd, ref_api):
    oi, _ = make_calibration_problem(amd._api, Ncameras=2, Nframes=6, seed=3)
    amd.optimize(**oi)
    m = [amd.cameramodel(optimization_inputs=oi, icam_intrinsics=i) for i in range(2)]
    cameras = [(oi["lensmodel"], oi["intrinsics"][i], m[i].rt_cam_ref()) for i in range(2)]
    q, _ = make_pixel_pairs(amd, ref_api, cameras, [(0, 1)]*6, seed=9)
    # one pair: no leading dimensions
    assert amd.triangulate(q[0], m).shape == (3,)
    r = amd.triangulate(q[0], m, q_calibration_stdev=0.3, q_observation_stdev=0.2)
    assert [x.shape for x in r] == [(3,), (3,3), (3,3), (3,3)]
    # (2,3, 2,2) x (2,): p (2,3,3)
    q23 = q.reshape(2,3,2,2)
    p = amd.triangulate(q23, m)
    assert p.shape == (2,3,3)
    r = amd.triangulate(q23, m, q_calibration_stdev=0.3)
    assert len(r) == 2 and r[1].shape == (2,3,3, 2,3,3) and np.array_equal(r[0], amd.triangulate(q23, m, q_observation_stdev=0.1)[0])
    r = amd.triangulate(q23, m, q_observation_stdev=0.1)
    assert len(r) == 2 and r[1].shape == (2,3,3,3)
    r = amd.triangulate(q23, m, q_calibration_stdev=0.3, q_observation_stdev=0.1)
    assert [x.shape for x in r] == [(2,3,3), (2,3,3,2,3,3), (2,3,3,3), (2,3,3,2,3,3)]
    # models (3,2) against q (2,1, 2,2)
    mm = np.array([[m[0], m[1]], [m[1], m[0]], [m[0], m[1]]], dtype=object)
    assert amd.triangulate(q[:2].reshape(2,1,2,2), mm).shape == (2,3,3)
    # a standard deviation of zero: zeros, of the right shapes, and the same points
    r = amd.triangulate(q23, m, q_calibration_stdev=0., q_observation_stdev=0.)
    assert [x.shape for x in r] == [(2,3,3), (2,3,3,2,3,3), (2,3,3,3), (2,3,3,2,3,3)]
    assert np.array_equal(r[0], p) and not any(np.any(x) for x in r[1:])
    r = amd.triangulate(q23, m, q_calibration_stdev=0.)
    assert len(r) == 2 and r[1].shape == (2,3,3,2,3,3) and not np.any(r[1])
    r = amd.triangulate(q23, m, q_observation_stdev=0.)
    assert len(r) == 2 and r[1].shape == (2,3,3,3) and not np.any(r[1])
    # lindstrom is fine as long as no noise is propagated
    r = amd.triangulate(q23, m, method=amd.triangulate_lindstrom, q_observation_stdev=0.)
    assert r[0].shape == (2,3,3) and not np.any(r[1])
    # a context made without the calibration cannot propagate its noise
    with amd.Triangulation(m) as t:
        with pytest.raises(Exception, match="calibration = False"):
            t.triangulate(q, q_calibration_stdev=1.)


# ---------------------------------------------------------------------------------------------------------------------
# calibration-time noise

class CalibrationChecker:
    """_propagate_calibration_uncertainty() restated densely: A = F (J*^T J*)^-1, Var = sigma^2 A J*[obs]^T J*[obs] A^T,
    with J from the reference's compiled optimizer_callback() and F = dp/db as _triangulation_uncertainty_internal()
    assembles it"""

    def __init__(self, amd, ref, oi):
        self.amd, self.ref, self.oi = amd, ref, oi
        _, x, J, _ = ref.optimizer_callback(no_factorization=True, **oi)
        self.J, self.Nstate = J, J.shape[1]
        self.Nreg  = ref.num_measurements_regularization(**oi)
        self.scale = np.ones(self.Nstate); ref.unpack_state(self.scale, **oi)
        ob = oi["observations_board"]
        i0 = ref.measurement_index_boards(0, **oi)
        xb = x[i0:i0 + ref.num_measurements_boards(**oi)].reshape(ob.shape[:-1] + (2,))[ob[...,2] > 0]
        self.sigma_est = np.sqrt(np.sum(xb*xb)/xb.size)/np.sqrt(1. - self.Nstate/xb.size)
        Ncam = len(oi["intrinsics"])
        self.cameras = [(oi["lensmodel"], oi["intrinsics"][i], oi["rt_cam_ref"][i-1] if i > 0 else np.zeros(6)) for i in range(Ncam)]
        self.Nsi = ref.num_intrinsics_optimization_params(**oi)
        Ncore = 4
        i0 = 0 if oi.get("do_optimize_intrinsics_core", True) else Ncore
        i1 = None if oi.get("do_optimize_intrinsics_distortions", True) else Ncore
        self.optimized = slice(i0, i1)
        self.istate_i = [ref.state_index_intrinsics(i, **oi) for i in range(Ncam)]
        self.istate_e = [None] + [ref.state_index_extrinsics(i-1, **oi) for i in range(1, Ncam)]
        self.istate_f0 = ref.state_index_frames(0, **oi)

    def F_packed(self, pieces, pair_cameras, stabilize_coords):
        oi, F = self.oi, np.zeros((len(pieces), 3, self.Nstate))
        frames = oi["rt_ref_frame"] if (stabilize_coords and self.istate_f0 is not None) else None
        for i, (g, (c0, c1)) in enumerate(zip(pieces, pair_cameras)):
            A1 = g["dp_dv1"] @ g["R01"]
            if self.istate_i[c0] is not None: F[i,:,self.istate_i[c0]:self.istate_i[c0] + self.Nsi] = g["dp_dv0"] @ g["dv0_di"][:,self.optimized]
            if self.istate_i[c1] is not None: F[i,:,self.istate_i[c1]:self.istate_i[c1] + self.Nsi] = A1 @ g["dvl1_di"][:,self.optimized]
            B = g["dp_dv1"] @ g["dv1_dr01"]
            for c, d in ((c1, g["drt01_drt1"]), (c0, g["drt01_drt0"])):
                e = self.istate_e[c]
                if e is None: continue
                F[i,:,e:e+3]   = B @ d[:3,:3] + g["dp_dt01"] @ d[3:,:3]
                F[i,:,e+3:e+6] = g["dp_dt01"] @ d[3:,3:]
            if not stabilize_coords: continue
            # the point in the reference frame, and in every frame: the direct dependence on those transformations
            rt0 = self.cameras[c0][2]
            R0, dR0 = R_and_dR(rt0[:3])
            dp_ref_drt0 = np.hstack((np.einsum('jik,j->ik', dR0, g["p"] - rt0[3:]), -R0.T))
            if self.istate_e[c0] is not None:
                F[i,:,self.istate_e[c0]:self.istate_e[c0] + 6] += np.linalg.solve(R0.T, dp_ref_drt0)
            if frames is not None:
                p_ref = R0.T @ (g["p"] - rt0[3:])
                for f, rtf in enumerate(frames):
                    Rf, dRf = R_and_dR(rtf[:3])
                    dpf_drtf = np.hstack((np.einsum('jik,j->ik', dRf, p_ref - rtf[3:]), -Rf.T))
                    F[i,:,self.istate_f0 + 6*f:self.istate_f0 + 6*f + 6] = np.linalg.solve(Rf.T @ R0.T, dpf_drtf)/len(frames)
        return F*self.scale

    def Var(self, F, sigma):
        F = F.reshape(-1, self.Nstate)
        JtJ = (self.J.T @ self.J).toarray()
        A = np.linalg.solve(JtJ, F.T).T
        Jo = self.J[:self.J.shape[0] - self.Nreg] if self.Nreg > 0 else self.J
        AJ = np.asarray((Jo @ A.T).T)
        return AJ @ AJ.T*sigma*sigma


def calibration_problem(amd, lensmodel="LENSMODEL_OPENCV8", **flags):
    oi, _ = make_calibration_problem(amd._api, Ncameras=3, Nframes=6, lensmodel=lensmodel, seed=11)
    oi.update(flags)
    amd.optimize(**oi)
    return oi


PAIRS3 = ((0, 1), (1, 2), (0, 2))


def check_calibration_noise(amd, ref_api, oi, N, seed, *, stabilize=(True, False), sigmas=(None, 0.4), method="leecivera_mid2"):
    ch = CalibrationChecker(amd, ref_api, oi)
    models = [amd.cameramodel(optimization_inputs=oi, icam_intrinsics=i) for i in range(3)]
    pair_cameras = [PAIRS3[i % 3] for i in range(N)] if N > 1 else [PAIRS3[1]]
    q, divergent = make_pixel_pairs(amd, ref_api, ch.cameras, pair_cameras, seed)
    pair_models  = np.array([[models[a], models[b]] for a, b in pair_cameras], dtype=object)
    p_ref, Vobs_ref, pieces = composed_flow(ref_api, unprojected_pairs(amd, ref_api, ch.cameras, pair_cameras, q, True), method, 0.3, 0.)
    check_points(p_ref, divergent)
    f = device_function(amd, method)
    live = amd.device_buffers_live()
    out = {}
    with amd.Triangulation(pair_models, calibration=True) as t:
        assert abs(t.observed_pixel_uncertainty - ch.sigma_est) < 1e-9*ch.sigma_est
        for stab in stabilize:
            F = ch.F_packed(pieces, pair_cameras, stab)
            for sigma in sigmas:
                V_ref = ch.Var(F, ch.sigma_est if sigma is None else sigma)
                p, V = t.triangulate(q, q_calibration_stdev=(-1. if sigma is None else sigma), method=f, stabilize_coords=stab)
                assert V.shape == (N,3,N,3)
                e = np.abs(V.reshape(3*N,3*N) - V_ref).max()/np.abs(V_ref).max()
                print(f"Var_p_calibration N={N} stabilize {stab} sigma {sigma}: {e:.3g} (p {worst(p, p_ref):.3g})")
                assert worst(p, p_ref) < TOL and e < COV_TOL
                assert np.array_equal(V.reshape(3*N,3*N), V.reshape(3*N,3*N).T)
                out[stab, sigma] = (q, pair_models, p, V)
    assert amd.device_buffers_live() == live
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("N", (1, 65))
def test_calibration_noise_against_the_dense_propagation(amd, ref_api, N):
    """pairs (0,1), (1,2) and (0,2) in one call (camera 0 has no extrinsics), the coordinates stabilized and not,
    sigma given and estimated"""
    oi = calibration_problem(amd)
    check_calibration_noise(amd, ref_api, oi, N, seed=3000 + N)


@pytest.mark.gpu
@pytest.mark.parametrize("flags", (dict(do_optimize_frames=False), dict(do_optimize_intrinsics_core=False),
                                   dict(do_optimize_intrinsics_distortions=False), dict(do_apply_regularization=False)),
                         ids=lambda d: next(iter(d)))
def test_calibration_noise_with_parts_of_the_state_fixed(amd, ref_api, flags):
    # (without regularization, a model with fewer parameters: OPENCV8 on these few frames is nearly singular then)
    lensmodel = "LENSMODEL_OPENCV4" if "do_apply_regularization" in flags else "LENSMODEL_OPENCV8"
    oi = calibration_problem(amd, lensmodel, **flags)
    check_calibration_noise(amd, ref_api, oi, 65, seed=3100, sigmas=(0.4,))


@pytest.mark.gpu
def test_calibration_noise_splined(amd, ref_api):
    oi = calibration_problem(amd, "LENSMODEL_SPLINED_STEREOGRAPHIC_order=3_Nx=8_Ny=6_fov_x_deg=80", do_optimize_intrinsics_core=False)
    check_calibration_noise(amd, ref_api, oi, 3, seed=3200, stabilize=(True,), sigmas=(0.4,))


@pytest.mark.gpu
def test_calibration_noise_properties(amd, ref_api):
    oi = calibration_problem(amd)
    out = check_calibration_noise(amd, ref_api, oi, 65, seed=3300, stabilize=(True,), sigmas=(0.4,), method="leecivera_wmid2")
    q, pair_models, p, V = out[True, 0.4]
    f = amd.triangulate_leecivera_wmid2
    live = amd.device_buffers_live()
    # one-shot == the reused context, to the bit; and the same bits twice
    r1 = amd.triangulate(q, pair_models, q_calibration_stdev=0.4, q_observation_stdev=0.3, q_observation_stdev_correlation=0.7, method=f)
    r2 = amd.triangulate(q, pair_models, q_calibration_stdev=0.4, q_observation_stdev=0.3, q_observation_stdev_correlation=0.7, method=f)
    assert np.array_equal(r1[0], p) and np.array_equal(r1[1], V)
    for a, b in zip(r1, r2): assert np.array_equal(a, b)
    # the joint covariance: the observation-time blocks added on the diagonal, to the bit
    J = r1[1].copy().reshape(195,195)
    for i in range(65): J[3*i:3*i+3, 3*i:3*i+3] += r1[2][i]
    assert np.array_equal(J, r1[3].reshape(195,195))
    assert np.array_equal(r1[2], amd.triangulate(q, pair_models, q_observation_stdev=0.3, q_observation_stdev_correlation=0.7, method=f)[1])
    # scales as sigma^2 (one multiplication more or less: a few units in the last place)
    V3 = amd.triangulate(q, pair_models, q_calibration_stdev=1.2, method=f)[1]
    assert np.abs(V3 - 9.*V).max() < 1e-12*np.abs(V3).max()
    assert amd.device_buffers_live() == live
