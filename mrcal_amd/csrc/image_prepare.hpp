// What is done to a raw image of the host before it is used on the device: the upload, then the equalization if one
// is asked for (equalize.hip), then the anti-aliasing filter if one is (smooth.hip). ONE place for the rectification's
// entry points and the feature matcher. The struct and ok() are host code with no HIP type or call:
// tests/hostcheck/image_prepare_check.cpp runs them under the host sanitizers. upload() is in rectification.hip.
#pragma once
#include <string>
#include "image_format.hpp"
#include "equalize_plan.hpp"
#include "smooth_plan.hpp"

namespace mrcal_amd {

class DeviceBuffers;

struct ImagePreparation
{
    EqualizeParams equalization;        // the method NONE: none
    SmoothParams   antialias;           // ... and after that; both sigmas 0: none

    bool off() const { return equalization.method == EQUALIZE_METHOD_NONE && smooth_is_off(antialias); }
    // the type of the prepared image: stretch makes uint8 of uint16
    int  dtype_out(int dtype) const { return equalize_dtype_out(equalization.method, dtype); }

    // An image that cannot be prepared: false, and why. The equalization speaks first, then the filter, of the type the
    // equalization leaves. (Of a pair, the second image's equalization cannot fail where the first one's filter does)
    bool ok(std::string* error, int width, int height, int channels, int dtype) const
    {
        const bool equalized = equalization.method != EQUALIZE_METHOD_NONE, filtered = !smooth_is_off(antialias);
        if((equalized || filtered) && channels != 1)
        {
            *error = std::string(equalized ? "equalize(): an image that is equalized" : "smooth(): an image that is filtered") +
                     " is grey, not of " + std::to_string(channels) + " channels";
            return false;
        }
        return (!equalized || equalize_params_ok(error, width, height, dtype, equalization)) &&
               (!filtered  || smooth_params_ok(error, width, height, dtype_out(dtype), antialias));
    }

    // The W x H image of C channels at host_image on the device, prepared: *d_image, of *dtype_image, a buffer of
    // `result`. Whatever else was made on the way (the raw image, the histograms and LUTs, the equalized image where it
    // is filtered afterwards) is `workspace`'s, which may go once the NULL stream has run dry. With everything off the
    // raw image IS the result, and nothing is queued. *d_unfiltered, if it is wanted: the image as it was before the
    // filter. The arguments have been checked (ok())
    bool upload(DeviceBuffers& result, DeviceBuffers& workspace, const void* host_image, int W, int H, int C, int dtype,
                const void** d_image, int* dtype_image, const void** d_unfiltered = NULL) const;
};

} // namespace mrcal_amd
