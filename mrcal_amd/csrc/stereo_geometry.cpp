// The geometry of a rectified stereo pair. HOST code: stereo_geometry.hpp
//
// Reference: stereo.c:19-780 (mrcal_rectified_resolution(), compute_pinhole_cxy(), mrcal_rectified_system2(),
// mrcal_rectified_system()): the math, the order of the refusals and their messages. The reference finds the
// quartic's roots with LAPACK's dgeev; the library has no LAPACK: roots_real_polynomial() below.
#include <math.h>
#include <float.h>
#include <string.h>
#include "host_state.hpp"
#include "lens_models.hpp"
#include "lens_dispatch.hpp"
#include "stereo_geometry.hpp"

namespace mrcal_amd {

namespace {

// monic: x^n + c[n-1] x^(n-1) + ... + c[0]
double poly  (int n, const double* c, double x) { double v = 1.0;       for(int i=n-1;i>=0;i--) v = v*x + c[i];             return v; }
double poly_d(int n, const double* c, double x) { double v = (double)n; for(int i=n-1;i>=1;i--) v = v*x + (double)i*c[i];   return v; }
double poly_dd(int n, const double* c, double x)
{
    double v = (double)(n*(n-1));
    for(int i=n-1;i>=2;i--) v = v*x + (double)(i*(i-1))*c[i];
    return v;
}

void mul33(double* out, const double* A, const double* B)
{
    for(int i=0;i<3;i++) for(int j=0;j<3;j++)
        out[3*i+j] = A[3*i]*B[j] + A[3*i+1]*B[3+j] + A[3*i+2]*B[6+j];
}
void mul33_v(double* out, const double* A, const double* x)
{
    for(int i=0;i<3;i++) out[i] = A[3*i]*x[0] + A[3*i+1]*x[1] + A[3*i+2]*x[2];
}
void transpose33(double* out, const double* A)
{
    for(int i=0;i<3;i++) for(int j=0;j<3;j++) out[3*i+j] = A[3*j+i];
}

} // namespace

int roots_real_polynomial(double* roots, int n, const double* c)
{
    if(n < 1 || n > 4) return -1;
    if(n == 1) { roots[0] = -c[0]; return 1; }

    // the stationary points: the real roots of p'/n, which is monic of order n-1
    double d[4], crit[4];
    for(int i=0;i<n-1;i++) d[i] = (double)(i+1)*c[i+1]/(double)n;
    const int Ncrit = roots_real_polynomial(crit, n-1, d);
    if(Ncrit < 0) return -1;

    // every root lies inside Cauchy's bound
    double B = 0.0;
    for(int i=0;i<n;i++) if(fabs(c[i]) > B) B = fabs(c[i]);
    B += 1.0;

    double pts[6]; bool isroot[6];
    int Npts = 0;
    pts[Npts] = -B; isroot[Npts++] = false;
    for(int i=0;i<Ncrit;i++)
    {
        const double p = poly(n, c, crit[i]);
        pts[Npts]      = crit[i];
        isroot[Npts++] = p == 0.0 || fabs(p) <= 0.5*fabs(poly_dd(n, c, crit[i]))*1e-14;
    }
    pts[Npts] = B; isroot[Npts++] = false;

    int Nroots = 0;
    for(int i=0;i+1<Npts;i++)
    {
        if(isroot[i]) roots[Nroots++] = pts[i];
        if(isroot[i] || isroot[i+1]) continue;
        double a = pts[i], b = pts[i+1];
        double fa = poly(n, c, a);
        const double fb = poly(n, c, b);
        if(!((fa < 0.0) != (fb < 0.0))) continue;
        // p is monotonic between two neighbouring stationary points: one root
        for(int it=0; it<200; it++)
        {
            const double m = 0.5*(a + b);
            if(!(m > a && m < b)) break;
            const double fm = poly(n, c, m);
            if(fm == 0.0) { a = b = m; break; }
            if((fm < 0.0) == (fa < 0.0)) { a = m; fa = fm; } else b = m;
        }
        double x = 0.5*(a + b);
        for(int it=0; it<3; it++)
        {
            const double g = poly_d(n, c, x);
            if(g == 0.0) break;
            const double x1 = x - poly(n, c, x)/g;
            if(!(x1 >= pts[i] && x1 <= pts[i+1]) || fabs(poly(n, c, x1)) > fabs(poly(n, c, x))) break;
            x = x1;
        }
        roots[Nroots++] = x;
    }
    return Nroots;
}

bool rectified_pinhole_cxy(double* cxy, double fxy, double tanazel0, double fov_deg)
{
    // The imager spans the pixels 0 .. N-1, N - 1 = 2 (tan(angle0) f + c), and its two edge rays, (-c/f, 1) and
    // (2 tan(angle0) + c/f, 1) in the plane of this axis, are to be fov apart. With u = c/f and k = 2 tan(angle0):
    //     cos(fov) |(-u,1)| |(k+u,1)| = (-u,1).(k+u,1) = 1 - k u - u^2
    // Squared, and divided by -sin^2(fov) to make it monic, this is a quartic in u:
    //     u^4 + 2k u^3 + (k^2 + 2 - 4/s) u^2 + 2k (1 - 2/s) u + 1 + k^2 (1 - 1/s) = 0,    s = sin^2(fov)
    const double c = cos(fov_deg*M_PI/180.);
    const double s = 1. - c*c;
    const double k = 2.*tanazel0;
    const double quartic[4] = { 1. + k*k*(1. - 1./s), 2.*k*(1. - 2./s), k*k + 2. - 4./s, 2.*k };
    for(double q : quartic) if(!isfinite(q)) return false;
    double u[4];
    const int Nu = roots_real_polynomial(u, 4, quartic);

    // Squaring lost the sign of cos(fov): a root counts only if the unsquared right-hand side has that sign (to 1e-9,
    // the reference's allowance), and only if the imager it implies has a positive size. One root should be left;
    // of several (rounding), the one that agrees in sign most clearly
    auto signed_side = [&](double ui) { return c*(1. - k*ui - ui*ui); };
    int best = -1;
    for(int i=0; i<Nu; i++)
    {
        if(signed_side(u[i]) < -1e-9)                continue;
        if(!(2.*fxy*(tanazel0 + u[i]) + 1. > 0.))    continue;
        if(best < 0 || signed_side(u[i]) > signed_side(u[best])) best = i;
    }
    if(best < 0) return false;
    *cxy = u[best]*fxy;
    return true;
}

bool project_with_gradient_host(double* q, double (*dq_dv)[3], const double* v,
                                const mrcal_lensmodel_t* lensmodel, const double* intrinsics)
{
    const LensConfig cfg = lens_config_of(*lensmodel);
    if(for_parametric_lens(lensmodel->type, [&](auto k)
       {
           using K = decltype(k);
           double gk[2][K::NDIST > 0 ? K::NDIST : 1];
           project_lens<K::PROJ,K::NDIST,true>(q, dq_dv, gk, v, intrinsics, cfg);
       }))
        return true;
    if(lensmodel->type != MRCAL_LENSMODEL_SPLINED_STEREOGRAPHIC) return false;
    double dfxy[2], cx[4], cy[4]; int ivar0;
    project_splined<true>(q, dq_dv, dfxy, &ivar0, cx, cy, v, intrinsics, cfg);
    return true;
}

void R_from_r_host(double* R, const double* r)
{
    const double th2 = r[0]*r[0] + r[1]*r[1] + r[2]*r[2];
    const double th  = sqrt(th2);
    double a, b;     // sin(th)/th, (1 - cos(th))/th^2
    if(th2 < 1e-12) { a = 1.0 - th2/6.0; b = 0.5 - th2/24.0; }
    else            { a = sin(th)/th;    b = (1.0 - cos(th))/th2; }
    const double K[9] = { 0., -r[2], r[1],   r[2], 0., -r[0],   -r[1], r[0], 0. };
    double KK[9];
    mul33(KK, K, K);
    for(int i=0;i<9;i++) R[i] = a*K[i] + b*KK[i];
    R[0] += 1.0; R[4] += 1.0; R[8] += 1.0;
}

void r_from_R_host(double* r, const double* R)
{
    const double v[3] = { R[7] - R[5], R[2] - R[6], R[3] - R[1] };   // 2 sin(th) axis
    const double s  = 0.5*sqrt(v[0]*v[0] + v[1]*v[1] + v[2]*v[2]);
    const double c  = 0.5*(R[0] + R[4] + R[8] - 1.0);
    const double th = atan2(s, c);
    if(c > 0 && s <= 1e-6) { for(int i=0;i<3;i++) r[i] = 0.5*v[i]; return; }
    if(c > 0 || s > 0.1)   { for(int i=0;i<3;i++) r[i] = v[i]*(th/(2.0*s)); return; }
    // near pi: the axis from the symmetric part, sym(R) - cos(th) I = (1 - cos(th)) a a^T
    double Bm[9];
    for(int i=0;i<3;i++) for(int j=0;j<3;j++) Bm[3*i+j] = 0.5*(R[3*i+j] + R[3*j+i]) - (i == j ? c : 0.0);
    int k = 0;
    if(Bm[4] > Bm[4*k]) k = 1;
    if(Bm[8] > Bm[4*k]) k = 2;
    double a[3] = { Bm[3*k], Bm[3*k+1], Bm[3*k+2] };
    const double mag = sqrt(a[0]*a[0] + a[1]*a[1] + a[2]*a[2]);
    const double sgn = (a[0]*v[0] + a[1]*v[1] + a[2]*v[2] < 0) ? -1.0 : 1.0;
    for(int i=0;i<3;i++) r[i] = sgn*a[i]/mag*th;
}

} // namespace mrcal_amd

using namespace mrcal_amd;

namespace {

double dot3(const double* a, const double* b) { return a[0]*b[0] + a[1]*b[1] + a[2]*b[2]; }
void cross3(double* out, const double* a, const double* b)
{
    out[0] = a[1]*b[2] - a[2]*b[1];
    out[1] = a[2]*b[0] - a[0]*b[2];
    out[2] = a[0]*b[1] - a[1]*b[0];
}
void scale3(double* a, double s) { for(int i=0;i<3;i++) a[i] *= s; }
const double DEG = M_PI/180.;

// the unit (LATLON, LONLAT) or z = 1 (PINHOLE) vector of a rectified model at (az, el), and its derivatives by the two
// angles. false: another model
bool rectified_vector(double* v, double* dv_daz, double* dv_del, mrcal_lensmodel_type_t model, double az, double el)
{
    const double sa = sin(az), ca = cos(az), se = sin(el), ce = cos(el);
    switch(model)
    {
    case MRCAL_LENSMODEL_LATLON:        // az is the latitude about the baseline, el the longitude
        v[0] = sa;       v[1] = ca*se;       v[2] = ca*ce;
        dv_daz[0] = ca;  dv_daz[1] = -sa*se; dv_daz[2] = -sa*ce;
        dv_del[0] = 0.;  dv_del[1] = ca*ce;  dv_del[2] = -ca*se;
        return true;
    case MRCAL_LENSMODEL_LONLAT:
        v[0] = ce*sa;        v[1] = se;       v[2] = ce*ca;
        dv_daz[0] = ce*ca;   dv_daz[1] = 0.;  dv_daz[2] = -ce*sa;
        dv_del[0] = -se*sa;  dv_del[1] = ce;  dv_del[2] = -se*ca;
        return true;
    case MRCAL_LENSMODEL_PINHOLE:       // v = (tan az, tan el, 1): d tan(th)/dth = 1/cos^2(th)
        v[0] = sa/ca;              v[1] = se/ce;             v[2] = 1.;
        dv_daz[0] = 1./(ca*ca);    dv_daz[1] = 0.;           dv_daz[2] = 0.;
        dv_del[0] = 0.;            dv_del[1] = 1./(ce*ce);   dv_del[2] = 0.;
        return true;
    default:
        return false;
    }
}

} // namespace

extern "C" {

bool mrcal_rectified_resolution(double* pixels_per_deg_az, double* pixels_per_deg_el,
                                const mrcal_lensmodel_t* lensmodel, const double* intrinsics,
                                const mrcal_point2_t* azel_fov_deg, const mrcal_point2_t* azel0_deg,
                                const double* R_cam0_rect0, const mrcal_lensmodel_type_t rectification_model_type)
{
    last_error_string().clear();
    double* pixels_per_deg[2] = { pixels_per_deg_az, pixels_per_deg_el };
    if(*pixels_per_deg[0] < 0 || *pixels_per_deg[1] < 0)
    {
        // A negative value scales the resolution camera 0 has at the centre of the rectified view: the length of
        // dq/d(angle) there, q = project(R_cam0_rect0 v(az, el))
        double v[3], dv[2][3];
        if(!rectified_vector(v, dv[0], dv[1], rectification_model_type, azel0_deg->x*DEG, azel0_deg->y*DEG))
        {
            set_error("Unsupported rectification model");
            return false;
        }
        double v_cam0[3], q[2], dq_dv[2][3];
        mul33_v(v_cam0, R_cam0_rect0, v);
        if(!project_with_gradient_host(q, dq_dv, v_cam0, lensmodel, intrinsics))
        {
            set_error("mrcal_rectified_resolution(): lens model %d is not supported", (int)lensmodel->type);
            return false;
        }
        for(int k=0;k<2;k++)
        {
            if(!(*pixels_per_deg[k] < 0)) continue;
            double dv_cam0[3];
            mul33_v(dv_cam0, R_cam0_rect0, dv[k]);
            const double pixels_per_rad = hypot(dot3(dq_dv[0], dv_cam0), dot3(dq_dv[1], dv_cam0));
            *pixels_per_deg[k] *= -pixels_per_rad*DEG;
        }
    }
    // An equiangular model has the same resolution everywhere, so the field of view can be made a whole number of
    // pixels. A PINHOLE model's resolution is the one at the centre and stays as asked
    if(rectification_model_type == MRCAL_LENSMODEL_LATLON || rectification_model_type == MRCAL_LENSMODEL_LONLAT)
        for(int k=0;k<2;k++)
        {
            const double fov = azel_fov_deg->xy[k];
            *pixels_per_deg[k] = round(fov * (*pixels_per_deg[k]))/fov;
        }
    return true;
}

bool mrcal_rectified_system2(unsigned int* imagersize_rectified, double* fxycxy_rectified, double* rt_rect0_ref,
                             double* baseline,
                             double* pixels_per_deg_az, double* pixels_per_deg_el,
                             mrcal_point2_t* azel_fov_deg, mrcal_point2_t* azel0_deg,
                             const double az_edge_margin_deg,
                             const mrcal_lensmodel_t* lensmodel0, const double* intrinsics0,
                             const double* rt_cam0_ref, const double* rt_cam1_ref,
                             const mrcal_lensmodel_type_t rectification_model_type,
                             bool az0_deg_autodetect, bool el0_deg_autodetect,
                             bool az_fov_deg_autodetect, bool el_fov_deg_autodetect)
{
    last_error_string().clear();
    // the refusals, in the reference's order and with its messages
    const struct { bool asked; const char* what; } not_yet[3] = { { el0_deg_autodetect,    "el0_deg_autodetect" },
                                                                  { az_fov_deg_autodetect, "az_fov_deg_autodetect" },
                                                                  { el_fov_deg_autodetect, "el_fov_deg_autodetect" } };
    for(const auto& n : not_yet)
        if(n.asked) { set_error("%s is not yet supported", n.what); return false; }
    const bool latlon = rectification_model_type == MRCAL_LENSMODEL_LATLON;
    if(!latlon && rectification_model_type != MRCAL_LENSMODEL_PINHOLE)
    {
        set_error("Unsupported rectification model %d. Only LENSMODEL_LATLON and LENSMODEL_PINHOLE are supported",
                  (int)rectification_model_type);
        return false;
    }
    if(!lens_supported(lensmodel0->type))
    {
        set_error("mrcal_rectified_system2(): lens model %d is not supported", (int)lensmodel0->type);
        return false;
    }
    // (CAHVORE is the one noncentral model, and it is central when its last three parameters, E, are zero)
    if(lensmodel0->type == MRCAL_LENSMODEL_CAHVORE)
    {
        const double* E = intrinsics0 + lensmodel_num_params(*lensmodel0) - 3;
        if(E[0] != 0 || E[1] != 0 || E[2] != 0)
        {
            set_error("Stereo rectification is only possible with a central projection. Please centralize your models. This is CAHVORE, so set E=0 to centralize. This will ignore all noncentral effects near the lens");
            return false;
        }
    }
    double* pixels_per_deg[2] = { pixels_per_deg_az, pixels_per_deg_el };
    for(int k=0;k<2;k++)
        if(*pixels_per_deg[k] == 0)
        {
            set_error("pixels_per_deg_%s == 0 is illegal. Must be >0 if we're trying to specify a value, or <0 to autodetect", k == 0 ? "az" : "el");
            return false;
        }
    if(!(azel_fov_deg->x > 0. && azel_fov_deg->y > 0.))
    {
        set_error("az_fov_deg, el_fov_deg must be > 0. No auto-detection implemented yet");
        return false;
    }

    // Camera 1 seen from camera 0: R01 = R0 R1^T, t01 = t0 - R01 t1
    double R0[9], R1[9], R1t[9], R01[9], t01[3];
    R_from_r_host(R0, rt_cam0_ref);
    R_from_r_host(R1, rt_cam1_ref);
    transpose33(R1t, R1);
    mul33(R01, R0, R1t);
    mul33_v(t01, R01, rt_cam1_ref + 3);
    for(int i=0;i<3;i++) t01[i] = rt_cam0_ref[3+i] - t01[i];

    // The rectified frame is camera 0 turned: x along the baseline; z the sum of the two optical axes (camera 1's is
    // the last column of R01) with its part along x taken off; y = z cross x. They are the rows of R_rect0_cam0
    *baseline = sqrt(dot3(t01, t01));
    if(*baseline < 1e-6)
    {
        set_error("The stereo pair has a unnaturally small baseline. Did you accidentally pass the same model for the two cameras?");
        return false;
    }
    double R_rect0_cam0[9];
    double *x = R_rect0_cam0, *y = R_rect0_cam0 + 3, *z = R_rect0_cam0 + 6;
    for(int i=0;i<3;i++) x[i] = t01[i]/(*baseline);
    const double axes[3]     = { R01[2], R01[5], R01[8] + 1. };
    const double axes_along  = dot3(axes, x);
    for(int i=0;i<3;i++) z[i] = axes[i] - axes_along*x[i];
    scale3(z, 1./sqrt(dot3(z, z)));
    cross3(y, z, x);

    // The centre of the view in azimuth. az = 0 is normal to the baseline; the cameras' mean axis need not be (one
    // camera may sit behind the other), so by default the view is centred on that axis - and moved if it then comes
    // within the margin of looking along the baseline. (The test is 1e-3 degrees looser than the move, so that a
    // moved centre passes it)
    const double half  = azel_fov_deg->x/2.;
    const double reach = 90. - az_edge_margin_deg;
    auto clear_of_baseline = [&](double az0) { return az0 - half > -(reach + 1e-3) && az0 + half < reach + 1e-3; };
    if(az0_deg_autodetect)
    {
        azel0_deg->x = asin(axes_along/sqrt(dot3(axes, axes)))/DEG;
        if(!clear_of_baseline(azel0_deg->x))
        {
            if(half > reach)
            {
                set_error("ERROR: rectified view cannot avoid looking along the baseline vector: az_fov_deg is too large. Have az_fov=%.1fdeg angle_margin=%.1fdeg",
                          azel_fov_deg->x, az_edge_margin_deg);
                return false;
            }
            azel0_deg->x = fmin(fmax(azel0_deg->x, half - reach), reach - half);
        }
    }
    else if(!clear_of_baseline(azel0_deg->x))
    {
        set_error("ERROR: rectified view looks along the baseline vector. Reduce az_fov_deg or move az0_deg closer to the center. Have az0=%.1fdeg az_fov=%.1fdeg angle_margin=%.1fdeg",
                  azel0_deg->x, azel_fov_deg->x, az_edge_margin_deg);
        return false;
    }

    double R_cam0_rect0[9];
    transpose33(R_cam0_rect0, R_rect0_cam0);
    if(!mrcal_rectified_resolution(pixels_per_deg_az, pixels_per_deg_el, lensmodel0, intrinsics0,
                                   azel_fov_deg, azel0_deg, R_cam0_rect0, rectification_model_type))
        return false;

    // The intrinsics and the imager, an axis at a time (k = 0: azimuth, x; 1: elevation, y)
    for(int k=0;k<2;k++)
    {
        const double angle0 = azel0_deg->xy[k]*DEG, fov_deg = azel_fov_deg->xy[k];
        double& f = fxycxy_rectified[k];
        double& c = fxycxy_rectified[2+k];
        int N;
        f = *pixels_per_deg[k]/DEG;                      // pixels per radian
        if(latlon)
        {
            // q = f angle + c. N pixels cover the field of view, and the middle of the imager looks at angle0
            N = (int)round(fov_deg * (*pixels_per_deg[k]));
            c = (N - 1)/2. - f*angle0;
        }
        else
        {
            // q = f tan(angle) + c: dq/dangle = f/cos^2(angle), and the resolution asked for is the one at angle0. The
            // view is not symmetric about angle0 in tan(angle): c is solved for, and N follows from it
            f *= cos(angle0)*cos(angle0);
            if(!rectified_pinhole_cxy(&c, f, tan(angle0), fov_deg))
            {
                set_error("Couldn't compute the rectified pinhole c%s. Something is wrong.", k == 0 ? "x" : "y");
                return false;
            }
            N = (int)round(2.*(f*tan(angle0) + c)) + 1;
        }
        imagersize_rectified[k] = (unsigned int)N;
    }
    if((int)imagersize_rectified[1] <= 0)
    {
        set_error("Resulting stereo geometry has Nel=%d. This is nonsensical. You should examine the geometry or adjust the elevation bounds or pixels-per-deg",
                  (int)imagersize_rectified[1]);
        return false;
    }

    // rect0 <- ref: camera 0's pose turned by R_rect0_cam0
    double R_rect0_ref[9];
    mul33(R_rect0_ref, R_rect0_cam0, R0);
    r_from_R_host(rt_rect0_ref, R_rect0_ref);
    mul33_v(rt_rect0_ref + 3, R_rect0_cam0, rt_cam0_ref + 3);
    return true;
}

// the form without az_edge_margin_deg: 10 degrees
bool mrcal_rectified_system(unsigned int* imagersize_rectified, double* fxycxy_rectified, double* rt_rect0_ref,
                            double* baseline,
                            double* pixels_per_deg_az, double* pixels_per_deg_el,
                            mrcal_point2_t* azel_fov_deg, mrcal_point2_t* azel0_deg,
                            const mrcal_lensmodel_t* lensmodel0, const double* intrinsics0,
                            const double* rt_cam0_ref, const double* rt_cam1_ref,
                            const mrcal_lensmodel_type_t rectification_model_type,
                            bool az0_deg_autodetect, bool el0_deg_autodetect,
                            bool az_fov_deg_autodetect, bool el_fov_deg_autodetect)
{
    return mrcal_rectified_system2(imagersize_rectified, fxycxy_rectified, rt_rect0_ref, baseline,
                                   pixels_per_deg_az, pixels_per_deg_el, azel_fov_deg, azel0_deg,
                                   10.0, lensmodel0, intrinsics0, rt_cam0_ref, rt_cam1_ref, rectification_model_type,
                                   az0_deg_autodetect, el0_deg_autodetect, az_fov_deg_autodetect, el_fov_deg_autodetect);
}

} // extern "C"
