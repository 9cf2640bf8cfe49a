// Host build of mrcal_amd/csrc/stereo_geometry.cpp ALONE for tests/test_stereo.py: the geometry of the rectified system
// has no device code and links against nothing of the library. Built with -ffp-contract=on like the library
#include "../../mrcal_amd/csrc/stereo_geometry.cpp"

extern "C" {

int stereocheck_roots_real_polynomial(double* roots, int n, const double* c)
{
    return mrcal_amd::roots_real_polynomial(roots, n, c);
}

// 1: *cxy is the centre pixel; 0: no valid root
int stereocheck_rectified_pinhole_cxy(double* cxy, double fxy, double tanazel0, double fov_deg)
{
    return mrcal_amd::rectified_pinhole_cxy(cxy, fxy, tanazel0, fov_deg) ? 1 : 0;
}

}
