// What every plan of the image path says about an image's format, once: the type codes, the bytes of a pixel, and the
// largest image any of them takes. Plain functions, no HIP type or call. The refusals and their words stay with each
// plan. tests/hostcheck/image_prepare_check.cpp runs it under the host sanitizers.
#pragma once
#include <stddef.h>

namespace mrcal_amd {

// (the values of MRCAL_AMD_IMAGE_*, which this file does not include: rectification.hip holds the two together)
#define IMAGE_DTYPE_UINT8   0
#define IMAGE_DTYPE_UINT16  1
#define IMAGE_DTYPE_FLOAT   2

#define IMAGE_MAX_PIXELS (1L << 28)         // a pixel index, a rank and a count of pixels are each an int32 with room to spare

inline size_t image_pixel_bytes(int dtype) { return dtype == IMAGE_DTYPE_UINT8 ? 1 : dtype == IMAGE_DTYPE_UINT16 ? 2 : 4; }
inline bool   image_dtype_is_integer(int dtype) { return dtype == IMAGE_DTYPE_UINT8 || dtype == IMAGE_DTYPE_UINT16; }
// not empty, and at most IMAGE_MAX_PIXELS
inline bool   image_size_ok(int W, int H) { return W > 0 && H > 0 && (long)W*(long)H <= IMAGE_MAX_PIXELS; }

} // namespace mrcal_amd
