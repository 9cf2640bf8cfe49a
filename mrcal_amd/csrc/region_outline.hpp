// The outline of the largest region of a mask (include/mrcal_amd.h, "valid-intrinsics region"). HOST code, nothing
// of HIP in it: tests/hostcheck/valid_region_check.cpp drives it under ASan + UBSan.
#pragma once
#include <stdint.h>
#include <vector>

namespace mrcal_amd {

struct OutlineVertex { int32_t x, y; };

// The 8 directions, clockwise on the screen (x to the right, y down) from east: the sense the border is followed in
constexpr int OUTLINE_DX[8] = { 1, 1, 0, -1, -1, -1,  0,  1 };
constexpr int OUTLINE_DY[8] = { 0, 1, 1,  1,  0, -1, -1, -1 };

// The vertices of the outer border of the component of set cells (mask != 0, [h][w]) with the largest shoelace area,
// the first of them in raster order among equals; not closed: the first vertex is not repeated. Empty for an empty
// mask. *area2: twice that area
std::vector<OutlineVertex> region_outline(const uint8_t* mask, int w, int h, int64_t* area2);

}

// the same for C: the number of vertices, of which the first min(count, capacity) are written; -1: bad arguments
extern "C" int mrcal_amd_region_outline(const uint8_t* mask, int gridn_width, int gridn_height, int32_t* vertices /* [capacity][2] */,
                                        int capacity, int64_t* area2);
