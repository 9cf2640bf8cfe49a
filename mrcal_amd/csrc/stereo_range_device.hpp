// The range and the observation vector of a pixel of the rectified camera 0: the ONE __device__ source of both, for
// the range kernels of rectification.hip and the point-cloud kernels of point_cloud.hip. DEVICE code.
// (stereo.c:1263-1417; the derivation: the docstring of mrcal.stereo_range())
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace mrcal_amd {

struct RangeArgs { double fx, fy, cx, cy, baseline; int latlon; };

// The range of the point seen at (qx, qy) in the rectified camera 0 and `disparity` pixels to the left of that in
// camera 1; 0 if that is not finite.
//   LATLON:  the two rays leave the ends of the baseline at the azimuths az0 and az1 = az0 - disparity/fx, measured from
//            its normal. In the triangle they make with the baseline the angle at the point is the parallax az0 - az1
//            and the angle at camera 1 is pi/2 + az1: by the law of sines range = baseline cos(az1)/sin(parallax)
//   PINHOLE: the depth along the rectified axis is z = baseline fx/disparity, and the point is z (tan az0, tan el, 1)
__device__ __forceinline__
double stereo_range_one(double disparity, double qx, double qy, const RangeArgs& a)
{
    const double ux = (qx - a.cx)/a.fx, parallax = disparity/a.fx;
    double range;
    if(a.latlon) range = a.baseline*cos(ux - parallax)/sin(parallax);
    else
    {
        const double uy = (qy - a.cy)/a.fy;
        range = a.baseline/parallax*sqrt(ux*ux + uy*uy + 1.);
    }
    return isfinite(range) ? range : 0.0;
}

// v: the unit observation vector of the pixel (qx, qy) of the rectified camera 0
__device__ __forceinline__
void stereo_unit_vector(double* v, double qx, double qy, const RangeArgs& a)
{
    const double ux = (qx - a.cx)/a.fx, uy = (qy - a.cy)/a.fy;
    if(a.latlon)
    {
        double sx, cx, sy, cy;
        sincos(ux, &sx, &cx);
        sincos(uy, &sy, &cy);
        v[0] = sx; v[1] = cx*sy; v[2] = cx*cy;
    }
    else
    {
        const double s = 1.0/sqrt(ux*ux + uy*uy + 1.0);
        v[0] = ux*s; v[1] = uy*s; v[2] = s;
    }
}

} // namespace mrcal_amd
