// The Gaussian pre-filter of smooth.hip for the translation unit that has an image on the device already
// (rectification.hip's ImagePreparation::upload(): a raw image between its upload, its equalization and whatever uses it).
// HOST declarations; the kernel stays where it is.
#pragma once
#include <stdint.h>
#include "../../include/mrcal_amd.h"
#include "device_memory.hpp"
#include "resident_common.hpp"
#include "smooth_plan.hpp"

namespace mrcal_amd {

// the C struct's fields as the plan takes them; NULL: both sigmas 0, which is "off"
SmoothParams smooth_params_of(const mrcal_amd_smooth_params_t* params);

// Filters the plan's W x H image at d_in into d_out (both on the device, dense, not the same memory), in the NULL
// stream: ONE launch. Queues it and returns: what reads d_out afterwards in that stream sees it filtered.
// events: NULL, or the events recorded before the launch and after it
typedef StageEvents<2> SmoothEvents;
bool smooth_device(const SmoothPlan& plan, const void* d_in, void* d_out, SmoothEvents* events = NULL);

// An image that lies on the device, filtered: *d_smoothed is a new buffer of `result`. Both sigmas 0:
// *d_smoothed = d_image, nothing runs and nothing is allocated
bool smooth_resident(DeviceBuffers& result, const SmoothParams& params, const void* d_image, int W, int H, int dtype,
                     const void** d_smoothed);

} // namespace mrcal_amd
