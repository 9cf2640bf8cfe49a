// The sum of a double over the 64 lanes of a wavefront, for the feature kernels. DEVICE code only (a lane operation):
// kept out of device_math.hpp, which the host checks compile.
#pragma once
#include <hip/hip_runtime.h>

namespace mrcal_amd {

// the sum over the wavefront, every lane ends up with it; the order of the additions is fixed
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for(int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

} // namespace mrcal_amd
