// The point cloud of point_cloud.hip for the other translation unit that has disparities on the device already
// (rectification.hip: mrcal_amd_rectification_point_cloud_of_images()). HOST declarations; the kernels stay where they are.
#pragma once
#include <stdint.h>
#include "../../include/mrcal_amd.h"

namespace mrcal_amd {

// mrcal_amd_point_cloud_compute() of disparities that lie on the device: W H dense uint16 (or int16: the bits), the start
// aligned to 8 bytes, written by work queued in the NULL stream. They are read there and not changed.
// d_color_image: NULL, or the colour image the parameters describe where it lies on the DEVICE already, written by work
// queued in the NULL stream: params->image, which must still not be NULL, is then not read
bool point_cloud_compute_device(mrcal_amd_point_cloud_t* c, const uint16_t* d_disparity,
                                const mrcal_amd_point_cloud_params_t* params, int* N, const void* d_color_image = NULL);

} // namespace mrcal_amd
