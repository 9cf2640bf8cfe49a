// The matcher of stereo_sgm.hip for the other translation unit that has rectified images on the device already
// (rectification.hip: mrcal_amd_rectification_disparity()). HOST declarations; the kernels stay where they are.
#pragma once
#include <stdint.h>

struct mrcal_amd_stereo_sgm;

namespace mrcal_amd {

// where image i (0, 1) of the next match lies on the device: W H dense pixels, the start aligned to 256 bytes
void* sgm_device_image(mrcal_amd_stereo_sgm* m, int i);
// matches the two images that lie there; disparity (H,W) on the host
bool sgm_match_device(mrcal_amd_stereo_sgm* m, int16_t* disparity);

} // namespace mrcal_amd
