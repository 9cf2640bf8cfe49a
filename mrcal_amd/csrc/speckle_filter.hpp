// The speckle filter of speckle_filter.hip for the other translation unit that has a disparity image on the device
// already (stereo_sgm.hip: the matcher's filter stage). HOST declarations; the kernels stay where they are.
#pragma once
#include <stdint.h>
#include "speckle_plan.hpp"
#include "resident_common.hpp"

namespace mrcal_amd {

// Filters the W x H image at `image` (device, dense int16) in place, in the NULL stream. workspace: device memory of
// speckle_workspace_bytes(W H) bytes, aligned to 4, whose contents are of no account before and after. Queues the
// launches and returns: what reads the image afterwards in that stream sees it filtered. pass_events: NULL, or the
// events to record before the first pass and after each of the four
typedef StageEvents<5> SpecklePassEvents;
bool speckle_filter_device(const SpeckleGrids& grids, const SpeckleParams& params, int16_t* image, void* workspace,
                           SpecklePassEvents* pass_events = NULL);

} // namespace mrcal_amd
