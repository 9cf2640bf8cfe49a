// The remap of rectification.hip for the other translation units that have an image and a map on the device already
// (match_feature.hip: the templates). HOST declarations; the kernel stays where it is.
#pragma once

namespace mrcal_amd {

// d_out[i] = d_src(d_map[i]) for the Nout entries of the map; all three on the device, dense, the arguments checked
// (remap_kernel: d_map and d_out each start an allocation). Queued on the null stream: returns without waiting
bool remap_device(const void* d_src, int W, int H, int C, int dtype, const float* d_map, void* d_out, int Nout,
                  int interp, int border_mode, const double* border_value);

} // namespace mrcal_amd
