// The six public triangulation methods: two observation rays -> the point they
// see, with its gradients. __host__ __device__: the kernels of triangulation.hip
// and the host build of the CPU tests compile this one source.
//
// Reference behaviour being reproduced (math and branch points):
//   triangulation.cc:16-101    triangulate_assume_intersect() (the better-
//                              conditioned of the xz / yz systems, |det| <= 1e-10,
//                              k0 <= 0, k1 < 0 -> no point)
//   triangulation.cc:107-209   geometric   (|denom| <= 1e-10, k0 <= 0, k1 <= 0)
//   triangulation.cc:214-431   lindstrom   (niter2 of "Triangulation Made Easy";
//                              LOCAL observation vectors, the whole Rt01)
//   triangulation.cc:436-510   leecivera_l1   (which ray moves: the one less
//                              perpendicular to t01)
//   triangulation.cc:515-573   leecivera_linf (which bisector: the longer normal)
//   triangulation.cc:576-636   chirality()
//   triangulation.cc:640-706   leecivera_mid2, ..._is_convergent
//   triangulation.cc:710-764   leecivera_wmid2
// Where the reference returns (0,0,0) a method here returns false, and its
// caller writes a zero point and zero gradients.
//
// The implementation is new. Every method is a template on its scalar: double,
// or Dual<N> of device_math.hpp with the inputs seeded as the independent
// variables (v0: 0..2, v1: 3..5, t01: 6..8; Lindstrom: Rt01 6..17). tri_eval()
// below seeds them NCHUNK at a time, so a lane never holds more than NCHUNK
// partials of anything, and takes the point from Dual<0>: a dual without
// partials runs the same operators in the same order as the passes that carry
// them, so p has the same bits with and without gradients (as plain doubles the
// front end would fuse a*b + c*d where the dual's operators cannot)
#pragma once
#include "device_math.hpp"

namespace mrcal_amd {

enum TriMethod { TRI_GEOMETRIC = 0, TRI_LINDSTROM = 1, TRI_LEECIVERA_L1 = 2, TRI_LEECIVERA_LINF = 3,
                 TRI_LEECIVERA_MID2 = 4, TRI_LEECIVERA_WMID2 = 5, TRI_NMETHODS = 6 };

// the third input: t01 (3 values), or Lindstrom's Rt01 (12)
MRCAL_AMD_HD constexpr int tri_pose_size(int method) { return method == TRI_LINDSTROM ? 12 : 3; }

MRCAL_AMD_HD double tri_value(double x) { return x; }
template<int N> MRCAL_AMD_HD double tri_value(const Dual<N>& x) { return x.x; }
MRCAL_AMD_HD double tri_sqrt(double x) { return sqrt(x); }
template<int N> MRCAL_AMD_HD Dual<N> tri_sqrt(const Dual<N>& x) { return dsqrt(x); }

template<class T> MRCAL_AMD_HD T tri_dot(const T* a, const T* b) { return a[0]*b[0] + a[1]*b[1] + a[2]*b[2]; }
template<class T> MRCAL_AMD_HD void tri_cross(T* c, const T* a, const T* b)
{
    c[0] = a[1]*b[2] - a[2]*b[1];
    c[1] = a[2]*b[0] - a[0]*b[2];
    c[2] = a[0]*b[1] - a[1]*b[0];
}
template<class T> MRCAL_AMD_HD T tri_cross_dot(const T* a, const T* b)
{
    T c[3];
    tri_cross(c, a, b);
    return tri_dot(c, c);
}
// v -= n (v.n)/(n.n): what is left of v in the plane with normal n
template<class T> MRCAL_AMD_HD void tri_project_out(T* v, const T* n)
{
    const T vn = tri_dot(v, n), nn = tri_dot(n, n);
    for(int i=0;i<3;i++) v[i] = v[i] - n[i]*vn/nn;
}
template<class T> MRCAL_AMD_HD void tri_normalize(T* v)
{
    const T mag = tri_sqrt(tri_dot(v, v));
    for(int i=0;i<3;i++) v[i] = v[i]/mag;
}

// Two rays known to intersect: k0 v0 = t01 + k1 v1, solved in the z axis and whichever of x, y gives the larger
// determinant. false: (nearly) parallel in both, or the intersection is behind either camera
template<class T> MRCAL_AMD_HD bool tri_assume_intersect(T* m, const T* v0, const T* v1, const T* t01)
{
    const double v0z = tri_value(v0[2]), v1z = tri_value(v1[2]), tz = tri_value(t01[2]);
    // (each product a statement of its own: nothing here for -ffp-contract=on to fuse, so a host without fused
    // multiply-adds takes the same branch as the device)
    const double xa = tri_value(v0[0])*v1z, xb = v0z*tri_value(v1[0]);
    const double ya = tri_value(v0[1])*v1z, yb = v0z*tri_value(v1[1]);
    const double det_xz = fabs(xb - xa);
    const double det_yz = fabs(yb - ya);
    const bool xz = det_xz > det_yz;
    if((xz ? det_xz : det_yz) <= 1e-10) return false;

    // (selected by value: an index that a lane computes would put the vectors in memory)
    const T v0a = xz ? v0[0] : v0[1], v1a = xz ? v1[0] : v1[1], ta = xz ? t01[0] : t01[1];
    const T det = v1a*v0[2] - v0a*v1[2];
    const T k0  = (t01[2]*v1a - ta*v1[2])/det;
    if(tri_value(k0) <= 0.0) return false;
    const bool k1_negative = (tz*tri_value(v0a) > tri_value(ta)*v0z) != (tri_value(det) > 0.0);
    if(k1_negative) return false;
    for(int i=0;i<3;i++) m[i] = v0[i]*k0;
    return true;
}

// The signs of l0, l1: would flipping either or both bring l0 v0 and t01 + l1 v1 closer together?
template<class T> MRCAL_AMD_HD bool tri_signs_are_right(const T& l0, const T* v0, const T& l1, const T* v1, const T* t01)
{
    T w0(0.0), w1(0.0), w01(0.0);
    for(int i=0;i<3;i++)
    {
        const T xn  = ( l1*v1[i] + t01[i]) - l0*v0[i];
        const T x0  = ( l1*v1[i] + t01[i]) + l0*v0[i];
        const T x1  = (-l1*v1[i] + t01[i]) - l0*v0[i];
        const T x01 = (-l1*v1[i] + t01[i]) + l0*v0[i];
        w0  = w0  + (x0 *x0  - xn*xn);
        w1  = w1  + (x1 *x1  - xn*xn);
        w01 = w01 + (x01*x01 - xn*xn);
    }
    return tri_value(w0) > 0.0 && tri_value(w1) > 0.0 && tri_value(w01) > 0.0;
}

// The midpoint of the two rays' closest approach
template<class T> MRCAL_AMD_HD bool tri_geometric(T* m, const T* v0, const T* v1, const T* t01)
{
    const T v0v0 = tri_dot(v0, v0), v1v1 = tri_dot(v1, v1), v0v1 = tri_dot(v0, v1);
    const T v0t  = tri_dot(v0, t01), v1t = tri_dot(v1, t01);
    const T denom = v0v0*v1v1 - v0v1*v0v1;
    if(-1e-10 <= tri_value(denom) && tri_value(denom) <= 1e-10) return false;
    const T denom_recip = T(1.0)/denom;
    const T k0 = denom_recip*(v1v1*v0t - v0v1*v1t);
    if(tri_value(k0) <= 0.0) return false;
    const T k1 = denom_recip*(v0v1*v0t - v0v0*v1t);
    if(tri_value(k1) <= 0.0) return false;
    for(int i=0;i<3;i++) m[i] = (v0[i]*k0 + v1[i]*k1 + t01[i])*0.5;
    return true;
}

// L1 angle error: the ray less perpendicular to the baseline moves into the other's epipolar plane
template<class T> MRCAL_AMD_HD bool tri_leecivera_l1(T* m, const T* v0_in, const T* v1_in, const T* t01)
{
    T v0[3] = { v0_in[0], v0_in[1], v0_in[2] }, v1[3] = { v1_in[0], v1_in[1], v1_in[2] };
    const double v0v0 = tri_value(tri_dot(v0, v0)), v1v1 = tri_value(tri_dot(v1, v1));
    const double v0t  = tri_value(tri_dot(v0, t01)), v1t = tri_value(tri_dot(v1, t01));
    T n[3];
    if(v0t*v0t*v1v1 > v1t*v1t*v0v0)
    {
        tri_cross(n, v1, t01);
        tri_project_out(v0, n);
    }
    else
    {
        tri_cross(n, v0, t01);
        tri_project_out(v1, n);
    }
    return tri_assume_intersect(m, v0, v1, t01);
}

// L-infinity angle error: both unit rays move into the plane of the baseline and one of their bisectors
template<class T> MRCAL_AMD_HD bool tri_leecivera_linf(T* m, const T* v0_in, const T* v1_in, const T* t01)
{
    T v0[3] = { v0_in[0], v0_in[1], v0_in[2] }, v1[3] = { v1_in[0], v1_in[1], v1_in[2] };
    tri_normalize(v0);
    tri_normalize(v1);
    T sum[3], dif[3], na[3], nb[3];
    for(int i=0;i<3;i++) { sum[i] = v0[i] + v1[i]; dif[i] = v0[i] - v1[i]; }
    tri_cross(na, sum, t01);
    tri_cross(nb, dif, t01);
    const bool use_na = tri_value(tri_dot(na, na)) > tri_value(tri_dot(nb, nb));
    T n[3];
    for(int i=0;i<3;i++) n[i] = use_na ? na[i] : nb[i];
    tri_project_out(v0, n);
    tri_project_out(v1, n);
    return tri_assume_intersect(m, v0, v1, t01);
}

// "Mid2" of "Triangulation: Why Optimize?"
template<class T> MRCAL_AMD_HD bool tri_leecivera_mid2(T* m, const T* v0, const T* v1, const T* t01)
{
    const T p_recip = T(1.0)/tri_cross_dot(v0, v1);
    const T l0 = tri_sqrt(tri_cross_dot(v1, t01)*p_recip);
    const T l1 = tri_sqrt(tri_cross_dot(v0, t01)*p_recip);
    if(!tri_signs_are_right(l0, v0, l1, v1, t01)) return false;
    for(int i=0;i<3;i++) m[i] = (v0[i]*l0 + t01[i] + v1[i]*l1)/2.0;
    return true;
}
MRCAL_AMD_HD bool tri_leecivera_mid2_is_convergent(const double* v0, const double* v1, const double* t01)
{
    typedef Dual<0> K;
    const K a[3] = { K(v0[0]), K(v0[1]), K(v0[2]) }, b[3] = { K(v1[0]), K(v1[1]), K(v1[2]) }, t[3] = { K(t01[0]), K(t01[1]), K(t01[2]) };
    K m[3];
    if(!tri_leecivera_mid2(m, a, b, t)) return false;
    return !(m[0].x == 0.0 && m[1].x == 0.0 && m[2].x == 0.0);
}

// "wMid2": unit rays, the two estimates weighted by the inverse of their ranges
template<class T> MRCAL_AMD_HD bool tri_leecivera_wmid2(T* m, const T* v0_in, const T* v1_in, const T* t01)
{
    T v0[3] = { v0_in[0], v0_in[1], v0_in[2] }, v1[3] = { v1_in[0], v1_in[1], v1_in[2] };
    tri_normalize(v0);
    tri_normalize(v1);
    const T p_recip = T(1.0)/tri_sqrt(tri_cross_dot(v0, v1));
    const T l0 = tri_sqrt(tri_cross_dot(v1, t01))*p_recip;
    const T l1 = tri_sqrt(tri_cross_dot(v0, t01))*p_recip;
    if(!tri_signs_are_right(l0, v0, l1, v1, t01)) return false;
    const T lsum = l0 + l1;
    for(int i=0;i<3;i++) m[i] = (v0[i]*l0*l1 + t01[i]*l0 + v1[i]*l0*l1)/lsum;
    return true;
}

// L2 pinhole reprojection error, two iterations. v0, v1 are in their OWN cameras' coordinates; Rt01: R01 row-major,
// then t01
template<class T> MRCAL_AMD_HD bool tri_lindstrom(T* m, const T* v0_local, const T* v1_local, const T* Rt01)
{
    const T* R = Rt01;
    const T* t = Rt01 + 9;
    // E = cross(t01) R01
    const T E[9] = { R[6]*t[1] - R[3]*t[2], R[7]*t[1] - R[4]*t[2], R[8]*t[1] - R[5]*t[2],
                     R[0]*t[2] - R[6]*t[0], R[1]*t[2] - R[7]*t[0], R[2]*t[2] - R[8]*t[0],
                     R[3]*t[0] - R[0]*t[1], R[4]*t[0] - R[1]*t[1], R[5]*t[0] - R[2]*t[1] };
    // the rays where they meet z = 1
    const T x0[2] = { v0_local[0]/v0_local[2], v0_local[1]/v0_local[2] };
    const T x1[2] = { v1_local[0]/v1_local[2], v1_local[1]/v1_local[2] };

    T n[2]  = { E[0]*x1[0] + E[1]*x1[1] + E[2], E[3]*x1[0] + E[4]*x1[1] + E[5] };
    T nn[2] = { E[0]*x0[0] + E[3]*x0[1] + E[6], E[1]*x0[0] + E[4]*x0[1] + E[7] };
    const T a = n[0]*E[0]*nn[0] + n[0]*E[1]*nn[1] + n[1]*E[3]*nn[0] + n[1]*E[4]*nn[1];
    const T b = (n[0]*n[0] + n[1]*n[1] + nn[0]*nn[0] + nn[1]*nn[1])*0.5;
    const T n2 = E[6]*x1[0] + E[7]*x1[1] + E[8];
    const T c = n[0]*x0[0] + n[1]*x0[1] + n2;
    const T d = tri_sqrt(b*b - a*c);
    T l = c/(b + d);
    T dx[2]  = { l*n[0],  l*n[1]  };
    T dxx[2] = { l*nn[0], l*nn[1] };
    n[0]  = n[0]  - E[0]*dxx[0] - E[1]*dxx[1];
    n[1]  = n[1]  - E[3]*dxx[0] - E[4]*dxx[1];
    nn[0] = nn[0] - E[0]*dx[0]  - E[3]*dx[1];
    nn[1] = nn[1] - E[1]*dx[0]  - E[4]*dx[1];
    const T bb = (n[0]*n[0] + n[1]*n[1] + nn[0]*nn[0] + nn[1]*nn[1])*0.5;
    l = l/d*bb;
    dx[0]  = l*n[0];   dx[1]  = l*n[1];
    dxx[0] = l*nn[0];  dxx[1] = l*nn[1];

    const T v0[3] = { x0[0] - dx[0],  x0[1] - dx[1],  T(1.0) };
    const T v1[3] = { x1[0] - dxx[0], x1[1] - dxx[1], T(1.0) };
    // the corrected rays intersect exactly; both in camera 0
    const T Rv1[3] = { R[0]*v1[0] + R[1]*v1[1] + R[2]*v1[2],
                       R[3]*v1[0] + R[4]*v1[1] + R[5]*v1[2],
                       R[6]*v1[0] + R[7]*v1[1] + R[8]*v1[2] };
    return tri_assume_intersect(m, v0, Rv1, t);
}

template<int METHOD, class T> MRCAL_AMD_HD bool tri_method(T* m, const T* v0, const T* v1, const T* pose)
{
    static_assert(0 <= METHOD && METHOD < TRI_NMETHODS, "one of TriMethod");
    if constexpr(METHOD == TRI_GEOMETRIC)            return tri_geometric      (m, v0, v1, pose);
    else if constexpr(METHOD == TRI_LINDSTROM)       return tri_lindstrom      (m, v0, v1, pose);
    else if constexpr(METHOD == TRI_LEECIVERA_L1)    return tri_leecivera_l1   (m, v0, v1, pose);
    else if constexpr(METHOD == TRI_LEECIVERA_LINF)  return tri_leecivera_linf (m, v0, v1, pose);
    else if constexpr(METHOD == TRI_LEECIVERA_MID2)  return tri_leecivera_mid2 (m, v0, v1, pose);
    else                                             return tri_leecivera_wmid2(m, v0, v1, pose);
}

// One pass: the inputs as duals whose independent variables are [ivar0, ivar0 + N) of (v0, v1, pose)
template<int METHOD, int N> MRCAL_AMD_HD bool tri_pass(Dual<N>* m, int ivar0, const double* v0, const double* v1, const double* pose)
{
    constexpr int NP = tri_pose_size(METHOD);
    Dual<N> a[3], b[3], c[NP];
    for(int i=0;i<3;i++)  { a[i] = Dual<N>::variable(v0[i], i - ivar0); b[i] = Dual<N>::variable(v1[i], 3 + i - ivar0); }
    for(int i=0;i<NP;i++) c[i] = Dual<N>::variable(pose[i], 6 + i - ivar0);
    return tri_method<METHOD>(m, a, b, c);
}

// One pair. p[3]; with WITH_GRAD dp_dv0[3][3], dp_dv1[3][3] and dp_dpose[3][NP] (dp_dt01, or Lindstrom's dp_dRt01),
// row-major, NCHUNK partials a pass (NCHUNK divides 3). No point: everything zero
template<int METHOD, bool WITH_GRAD, int NCHUNK> MRCAL_AMD_HD
void tri_eval(double* p, double* dp_dv0, double* dp_dv1, double* dp_dpose, const double* v0, const double* v1, const double* pose)
{
    constexpr int NP = tri_pose_size(METHOD);
    static_assert(3 % NCHUNK == 0, "a pass does not straddle two of the inputs");
    Dual<0> m0[3];
    const bool ok = tri_pass<METHOD, 0>(m0, 0, v0, v1, pose);
    for(int i=0;i<3;i++) p[i] = ok ? m0[i].x : 0.0;
    if constexpr(WITH_GRAD)
    {
        if(!ok)
        {
            for(int i=0;i<9;i++)    { dp_dv0[i] = 0.0; dp_dv1[i] = 0.0; }
            for(int i=0;i<3*NP;i++) dp_dpose[i] = 0.0;
            return;
        }
#pragma unroll
        for(int ivar0 = 0; ivar0 < 6 + NP; ivar0 += NCHUNK)
        {
            Dual<NCHUNK> m[3];
            tri_pass<METHOD, NCHUNK>(m, ivar0, v0, v1, pose);
            double* g    = ivar0 < 3 ? dp_dv0 : (ivar0 < 6 ? dp_dv1 : dp_dpose);
            const int nc = ivar0 < 6 ? 3 : NP;
            const int c0 = ivar0 < 3 ? ivar0 : (ivar0 < 6 ? ivar0 - 3 : ivar0 - 6);
            for(int i=0;i<3;i++)
                for(int k=0;k<NCHUNK;k++) g[nc*i + c0 + k] = m[i].d[k];
        }
    }
}

} // namespace mrcal_amd
