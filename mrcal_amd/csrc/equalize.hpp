// The equalization of equalize.hip for the other translation units that have an image on the device already
// (rectification.hip's ImagePreparation::upload(): a raw image after its upload, for rectification.hip's remaps and match_feature.hip's matcher).
// HOST declarations; the kernels stay where they are.
#pragma once
#include <stdint.h>
#include "../../include/mrcal_amd.h"
#include "device_memory.hpp"
#include "resident_common.hpp"
#include "equalize_plan.hpp"

namespace mrcal_amd {

// the C struct's fields as the plan takes them; NULL: no equalization
EqualizeParams equalize_params_of(const mrcal_amd_equalize_params_t* params);

// Equalizes the plan's W x H image at d_in into d_out (both on the device, dense, aligned to 16 bytes, not the same
// memory), in the NULL stream. pool: the device memory the plan's offsets hist, lut and minmax count from, whose
// contents are of no account before and after. Queues the launches and returns: what reads d_out afterwards in that
// stream sees it equalized. The method NONE is refused: there is nothing to run. stage_events: NULL, or the events
// recorded before the histograms (stretch: the extremes), the LUTs and the result, and after it
typedef StageEvents<4> EqualizeStageEvents;
bool equalize_device(const EqualizePlan& plan, const void* d_in, void* d_out, uint8_t* pool, EqualizeStageEvents* stage_events = NULL);

// An image that lies on the device, equalized: *d_equalized is a new buffer of `result` (of *dtype_equalized: stretch
// makes uint8 of uint16); the histograms and LUTs are buffers of `workspace`, which may go once the NULL stream has
// run dry. The method NONE: *d_equalized = d_image, nothing runs and nothing is allocated
bool equalize_resident(DeviceBuffers& result, DeviceBuffers& workspace, const EqualizeParams& params,
                       const void* d_image, int W, int H, int dtype, const void** d_equalized, int* dtype_equalized);

} // namespace mrcal_amd
