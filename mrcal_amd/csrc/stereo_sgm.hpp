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
// ... and leaves the disparities where they are: *d_disparity is the (H,W) int16 image on the device, aligned to 256
// bytes, complete once the work this queued in the NULL stream is. It is the matcher's: gone with it, and overwritten
// by its next match
bool sgm_match_device_resident(mrcal_amd_stereo_sgm* m, const int16_t** d_disparity);

} // namespace mrcal_amd
