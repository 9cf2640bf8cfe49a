// The geometry of a rectified stereo pair: mrcal_rectified_resolution(), mrcal_rectified_system2() (reference:
// stereo.c:19-780). HOST code, no HIP runtime types: the one projection gradient the resolution autodetect needs comes
// from the host build of lens_models.hpp, so the whole of rectified_system() runs without a GPU.
#pragma once
#include "../../include/mrcal_amd.h"

namespace mrcal_amd {

// the real roots of x^n + c[n-1] x^(n-1) + ... + c[0], n <= 4, ascending; a root of even multiplicity is reported
// once. Returns how many. The reference asks LAPACK for the eigenvalues of the companion matrix and keeps those with
// |imag| <= 1e-7; here the roots are bracketed between the real roots of the derivative (found the same way, down to
// the linear polynomial), bisected and polished by Newton. A stationary point where |p| <= |p''|/2 (1e-7)^2 is the
// double root the reference's threshold would keep
int roots_real_polynomial(double* roots, int n, const double* c);

// cx (or cy) of a PINHOLE rectified system: stereo.c:274-385. false: no valid root
bool rectified_pinhole_cxy(double* cxy, double fxy, double tanazel0, double fov_deg);

// q = project(v) and dq/dv (2x3) of one point on the host, any supported model. false: unsupported model
bool project_with_gradient_host(double* q, double (*dq_dv)[3], const double* v,
                                const mrcal_lensmodel_t* lensmodel, const double* intrinsics);

void R_from_r_host(double* R /*3x3*/, const double* r);
void r_from_R_host(double* r, const double* R /*3x3*/);

} // namespace mrcal_amd
