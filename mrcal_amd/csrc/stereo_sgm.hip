// stereo_matching_sgm(): dense disparities of a rectified pair by semi-global matching on a census cost
// (include/mrcal_amd.h, "stereo_matching_sgm": the definition, to the bit). The reference's tool hands this step to
// cv2.StereoSGBM or libelas; nothing of either is imitated pixel for pixel.
//
//   sgm_census_kernel<T>   a lane a pixel (4 rows each), the 64 x 16 tile and its 4/3-pixel apron staged in LDS with
//                          clamped coordinates; one 64-bit word a pixel, 64 consecutive words a wavefront
//   sgm_path_kernel<NPL>   the hot path, ONE kernel for the 8 directions, a launch a direction. A path is carried by
//                          the 16 lanes of a DPP row, lane j holding the NPL = D/16 consecutive disparities
//                          j NPL .. j NPL + NPL - 1 of L_r in registers; a wavefront carries 4 paths and is a workgroup.
//                            horizontal: a path a row, a step a column
//                            vertical:   a path a column, a step a row: the 4 paths of a wavefront are 4 neighbouring
//                                        columns, so the census words and the entries of S a step touches are contiguous
//                            diagonal:   as vertical, the column moving by +-1 a step and WRAPPING around the image's
//                                        side, where the path begins anew (its predecessor is outside: L = C). Every
//                                        pixel of a row belongs to exactly one path, and a path never needs another's L
//                          The cost volume is not materialised: C is an XOR and a 64-bit popcount of two census words,
//                          recomputed per path. m = min_k L(p-r,k) is NPL - 1 minima in registers and 4 DPP steps
//                          (quad_perm, quad_perm, row_half_mirror, row_mirror); L(i-1), L(i+1) are register moves
//                          inside a lane and one row_shr:1 / row_shl:1 at its ends, whose `old` operand supplies
//                          "takes no part" for the lanes 0 and 15. No LDS. The loads (census words, entries of S)
//                          depend on the position alone and run SGM_AHEAD = 4 steps ahead of the recurrence
//                          S: each path adds its L into the 16-bit S, the launches in stream order (the first one
//                          stores); two disparities to a 32-bit word, added as words: no field exceeds 2040
//   sgm_select_kernel<NPL> 16 lanes a pixel, as above. The minimum over (S, index) packed into one integer, S above the
//                          index: the earlier index wins ties by construction. Uniqueness by a ballot over the row,
//                          the subpixel step with a floor division. The same tree, over the diagonal S(y, x1 + d, i),
//                          gives the right image's index i1
//   sgm_check_kernel       a lane a pixel, a launch AFTER the selection: every i1 is written before any is read
// No floating-point values, no atomics.
// On request only (mrcal_amd_stereo_sgm_set_speckle_filter()), the speckle filter of speckle_filter.hip runs on the
// disparity image after the check, its labels and counts in S, which nothing reads any more by then.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <string>
#include "../../include/mrcal_amd.h"
#include "host_state.hpp"
#include "device_memory.hpp"
#include "sgm_plan.hpp"
#include "stereo_sgm.hpp"
#include "speckle_filter.hpp"

namespace mrcal_amd {

namespace {

struct SgmArgs { int W, H, D, dmin, P1, P2; };

#define SGM_NO_PART (1 << 20)           // larger than any L + P2; what a neighbour that takes no part holds

////////////////////////////////////////////////////////////////////////////////
// census
////////////////////////////////////////////////////////////////////////////////
template<class T>
__global__ __launch_bounds__(256)
void sgm_census_kernel(int W, int H, const T* __restrict__ image, uint64_t* __restrict__ census)
{
    constexpr int ROWS = SGM_CENSUS_TILE_Y + 2*SGM_CENSUS_RY, COLS = SGM_CENSUS_TILE_X + 2*SGM_CENSUS_RX;
    __shared__ T tile[ROWS][COLS];
    const int x0 = blockIdx.x*SGM_CENSUS_TILE_X, y0 = blockIdx.y*SGM_CENSUS_TILE_Y;
    const int tid = threadIdx.y*SGM_CENSUS_TILE_X + threadIdx.x;
    for(int i = tid; i < ROWS*COLS; i += 256)
    {
        const int r = i / COLS, c = i - r*COLS;
        const int gy = min(max(y0 + r - SGM_CENSUS_RY, 0), H - 1), gx = min(max(x0 + c - SGM_CENSUS_RX, 0), W - 1);
        tile[r][c] = image[(size_t)gy*W + gx];
    }
    __syncthreads();
    const int tx = threadIdx.x, x = x0 + tx;
#pragma unroll
    for(int k = 0; k < 4; k++)
    {
        const int ty = threadIdx.y + 4*k, y = y0 + ty;
        const T centre = tile[ty + SGM_CENSUS_RY][tx + SGM_CENSUS_RX];
        uint64_t bits = 0;
#pragma unroll
        for(int dy = 0; dy <= 2*SGM_CENSUS_RY; dy++)
#pragma unroll
            for(int dx = 0; dx <= 2*SGM_CENSUS_RX; dx++)
                if(!(dy == SGM_CENSUS_RY && dx == SGM_CENSUS_RX))
                    bits = (bits << 1) | (uint64_t)(tile[ty + dy][tx + dx] < centre);
        if(x < W && y < H) census[(size_t)y*W + x] = bits;
    }
}

////////////////////////////////////////////////////////////////////////////////
// the 16 lanes of a DPP row
////////////////////////////////////////////////////////////////////////////////
template<int CTRL>
__device__ __forceinline__ int sgm_dpp(int old, int v) { return __builtin_amdgcn_update_dpp(old, v, CTRL, 0xf, 0xf, false); }

// the minimum over the row, in every lane of it
__device__ __forceinline__ int sgm_row_min(int v)
{
    v = min(v, sgm_dpp<0xB1>(v, v));        // quad_perm:[1,0,3,2]
    v = min(v, sgm_dpp<0x4E>(v, v));        // quad_perm:[2,3,0,1]
    v = min(v, sgm_dpp<0x141>(v, v));       // row_half_mirror
    v = min(v, sgm_dpp<0x140>(v, v));       // row_mirror
    return v;
}

// The NPL entries of S of this lane, s[0..NPL): aligned to 2 NPL bytes. Two to a 32-bit word, and as wide a load or
// store as NPL allows
template<int NPL> struct SgmWords
{
    static constexpr int NW = NPL/2;                                        // 32-bit words
    static constexpr int VW = NW % 4 == 0 ? 4 : NW % 2 == 0 ? 2 : 1;        // words a load
};
typedef uint32_t sgm_u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t sgm_u32x4 __attribute__((ext_vector_type(4)));

template<int NPL>
__device__ __forceinline__ void sgm_load_words(uint32_t (&w)[NPL/2], const uint16_t* s)
{
    constexpr int NW = SgmWords<NPL>::NW, VW = SgmWords<NPL>::VW;
#pragma unroll
    for(int v = 0; v < NW/VW; v++)
    {
        if constexpr (VW == 4) { const sgm_u32x4 q = ((const sgm_u32x4*)s)[v]; w[4*v] = q.x; w[4*v+1] = q.y; w[4*v+2] = q.z; w[4*v+3] = q.w; }
        else if constexpr (VW == 2) { const sgm_u32x2 q = ((const sgm_u32x2*)s)[v]; w[2*v] = q.x; w[2*v+1] = q.y; }
        else w[v] = ((const uint32_t*)s)[v];
    }
}
template<int NPL>
__device__ __forceinline__ void sgm_store_words(uint16_t* s, const uint32_t (&w)[NPL/2])
{
    constexpr int NW = SgmWords<NPL>::NW, VW = SgmWords<NPL>::VW;
#pragma unroll
    for(int v = 0; v < NW/VW; v++)
    {
        if constexpr (VW == 4) { sgm_u32x4 q; q.x = w[4*v]; q.y = w[4*v+1]; q.z = w[4*v+2]; q.w = w[4*v+3]; ((sgm_u32x4*)s)[v] = q; }
        else if constexpr (VW == 2) { sgm_u32x2 q; q.x = w[2*v]; q.y = w[2*v+1]; ((sgm_u32x2*)s)[v] = q; }
        else ((uint32_t*)s)[v] = w[v];
    }
}

template<int NPL>
__device__ __forceinline__ void sgm_load_S(int (&v)[NPL], const uint16_t* s)
{
    if constexpr (NPL % 2 == 0)
    {
        uint32_t w[NPL/2];
        sgm_load_words<NPL>(w, s);
#pragma unroll
        for(int j = 0; j < NPL/2; j++) { v[2*j] = (int)(w[j] & 0xFFFFu); v[2*j+1] = (int)(w[j] >> 16); }
    }
    else
    {
#pragma unroll
        for(int k = 0; k < NPL; k++) v[k] = (int)s[k];
    }
}

// The NPL entries of S of a lane on their way through the path kernel: loaded some steps ahead, L added, stored.
// An even NPL: as 32-bit words of two; an odd one: entry by entry
template<int NPL, bool WORDS = NPL % 2 == 0> struct SgmEntries;
template<int NPL> struct SgmEntries<NPL, true>
{
    uint32_t w[NPL/2];
    __device__ __forceinline__ void load(const uint16_t* s) { sgm_load_words<NPL>(w, s); }
    // S += L (first: S = L)
    __device__ __forceinline__ void add_and_store(uint16_t* s, const int (&L)[NPL], bool first)
    {
#pragma unroll
        for(int j = 0; j < NPL/2; j++)
        {
            const uint32_t add = (uint32_t)L[2*j] | ((uint32_t)L[2*j+1] << 16);
            w[j] = first ? add : w[j] + add;        // (no field exceeds 2040: nothing carries into its neighbour)
        }
        sgm_store_words<NPL>(s, w);
    }
};
template<int NPL> struct SgmEntries<NPL, false>
{
    uint16_t v[NPL];
    __device__ __forceinline__ void load(const uint16_t* s)
    {
#pragma unroll
        for(int k = 0; k < NPL; k++) v[k] = s[k];
    }
    __device__ __forceinline__ void add_and_store(uint16_t* s, const int (&L)[NPL], bool first)
    {
#pragma unroll
        for(int k = 0; k < NPL; k++) s[k] = (uint16_t)(first ? L[k] : (int)v[k] + L[k]);
    }
};

////////////////////////////////////////////////////////////////////////////////
// the paths
////////////////////////////////////////////////////////////////////////////////
// C(y,x,i0 + k), k = 0..NPL-1: the census words of image1 at x - d lie side by side, in descending order
template<int NPL>
__device__ __forceinline__
void sgm_cost(int (&C)[NPL], const SgmArgs& a, int x, int y, int i0,
              const uint64_t* __restrict__ census0, const uint64_t* __restrict__ census1)
{
    const size_t row = (size_t)y*a.W;
    const uint64_t c0 = census0[row + x];
    const int xr0 = x - (a.dmin + i0);
    // every load is made, from a clamped column, and all of them before the first is used: a load only where x - d is
    // inside becomes a branch a disparity, each with its own wait
    uint64_t c1[NPL];
#pragma unroll
    for(int k = 0; k < NPL; k++) c1[k] = census1[row + min(max(xr0 - k, 0), a.W - 1)];
#pragma unroll
    for(int k = 0; k < NPL; k++)
    {
        const int xr = xr0 - k;
        C[k] = (xr >= 0 && xr < a.W) ? __popcll(c0 ^ c1[k]) : 62;
    }
}

// where a path is: the pixel, and how many steps it has made
struct SgmCursor
{
    int x, y, t;
    __device__ __forceinline__ void advance(const SgmArgs& a, int dx, int dy, bool horizontal)
    {
        x += dx; y += dy; t++;
        if(!horizontal) { if(x < 0) x = a.W - 1; else if(x >= a.W) x = 0; }     // a diagonal comes around
    }
};

// How many steps ahead of the recurrence the loads run. A launch has one or two wavefronts a SIMD and a step is a
// serial chain, so nothing but the path's own later steps can cover a load's latency: the costs and the entries of S
// of step t + SGM_AHEAD are asked for before step t is worked out. They depend on the position alone
#define SGM_AHEAD 4

// (dx,dy): the direction r; dy == 0: horizontal. first: this launch stores S, the others add to it
template<int NPL>
__global__ __launch_bounds__(SGM_PATH_THREADS)
void sgm_path_kernel(SgmArgs a, int dx, int dy, int first,
                     const uint64_t* __restrict__ census0, const uint64_t* __restrict__ census1, uint16_t* __restrict__ S)
{
    const int  lane = threadIdx.x & (SGM_LANES - 1);
    const int  path = blockIdx.x*SGM_WAVE_PATHS + (threadIdx.x >> 4);
    const bool horizontal = dy == 0;
    const int  Npaths = horizontal ? a.H : a.W, Nsteps = horizontal ? a.W : a.H;
    if(path >= Npaths) return;          // (the whole DPP row)
    const int i0 = lane*NPL;
    // where a path enters the image sideways
    const int xenter = dx > 0 ? 0 : a.W - 1;
    SgmCursor at;                       // the recurrence
    at.x = horizontal ? xenter : path;
    at.y = horizontal ? path : (dy > 0 ? 0 : a.H - 1);
    at.t = 0;
    SgmCursor ahead = at;               // the loads

    int             C[SGM_AHEAD][NPL];
    SgmEntries<NPL> entries[SGM_AHEAD];
    auto ask = [&](int slot)
    {
        if(ahead.t >= Nsteps) return;
        sgm_cost<NPL>(C[slot], a, ahead.x, ahead.y, i0, census0, census1);
        if(!first) entries[slot].load(S + ((size_t)ahead.y*a.W + ahead.x)*(size_t)a.D + i0);
        ahead.advance(a, dx, dy, horizontal);
    };
#pragma unroll
    for(int slot = 0; slot < SGM_AHEAD; slot++) ask(slot);

    int L[NPL];
#pragma unroll
    for(int k = 0; k < NPL; k++) L[k] = 0;
    while(at.t < Nsteps)
    {
#pragma unroll
        for(int slot = 0; slot < SGM_AHEAD; slot++)
        {
            if(at.t >= Nsteps) break;
            // the predecessor p - r is outside the image: at the path's first step, and where a diagonal comes around
            // ... which is the recurrence from L = 0: m = 0, and the least of 0, P1, P2 is 0. (A select between C and
            // the recurrence's value becomes a branch a disparity)
            const bool begins = at.t == 0 || (!horizontal && dx != 0 && at.x == xenter);
#pragma unroll
            for(int k = 0; k < NPL; k++) L[k] = begins ? 0 : L[k];
            int m = L[0];
#pragma unroll
            for(int k = 1; k < NPL; k++) m = min(m, L[k]);
            m = sgm_row_min(m);
            const int below = sgm_dpp<0x111>(SGM_NO_PART, L[NPL-1]);        // row_shr:1: L(i0 - 1) from the lane before
            const int above = sgm_dpp<0x101>(SGM_NO_PART, L[0]);            // row_shl:1: L(i0 + NPL) from the lane after
            const int far = m + a.P2;
            int before = below;
#pragma unroll
            for(int k = 0; k < NPL; k++)
            {
                const int here  = L[k];
                const int after = k + 1 < NPL ? L[k+1] : above;
                const int best  = min(min(here, far), min(before, after) + a.P1);
                L[k]   = C[slot][k] + best - m;
                before = here;
            }
            entries[slot].add_and_store(S + ((size_t)at.y*a.W + at.x)*(size_t)a.D + i0, L, first != 0);
            at.advance(a, dx, dy, horizontal);
            ask(slot);                  // the slot is free: step at.t + SGM_AHEAD - 1
        }
    }
}

////////////////////////////////////////////////////////////////////////////////
// the selection
////////////////////////////////////////////////////////////////////////////////
// floor(n/d), d > 0
__device__ __forceinline__ int sgm_floor_div(int n, int d) { return n >= 0 ? n/d : -((-n + d - 1)/d); }

// scaled: the scaled index of step 4, or -1 for a pixel that is not unique
template<int NPL>
__global__ __launch_bounds__(SGM_SELECT_THREADS)
void sgm_select_kernel(SgmArgs a, int uniqueness_ratio, const uint16_t* __restrict__ S,
                       uint8_t* __restrict__ index_left, uint8_t* __restrict__ index_right, int16_t* __restrict__ scaled)
{
    const int    lane  = threadIdx.x & (SGM_LANES - 1);
    const size_t N     = (size_t)a.W*a.H;
    const size_t pixel = (size_t)blockIdx.x*SGM_SELECT_PIXELS + (threadIdx.x >> 4);
    if(pixel >= N) return;              // (the whole DPP row)
    const int y = (int)(pixel / a.W), x = (int)(pixel - (size_t)y*a.W);
    const int i0 = lane*NPL;
    const uint16_t* Sp = S + pixel*(size_t)a.D;

    // the left image: S above the index in one integer, so that the minimum is the first index of the least S
    int s[NPL];
    sgm_load_S<NPL>(s, Sp + i0);
    int key = (s[0] << 8) | i0;
#pragma unroll
    for(int k = 1; k < NPL; k++) key = min(key, (s[k] << 8) | (i0 + k));
    key = sgm_row_min(key);
    const int istar = key & 255, smin = key >> 8;
    bool rival = false;
#pragma unroll
    for(int k = 0; k < NPL; k++)
    {
        const int i = i0 + k;
        if((i < istar - 1 || i > istar + 1) && s[k]*(100 - uniqueness_ratio) < smin*100) rival = true;
    }
    const unsigned long long rivals = __ballot(rival);
    const bool unique = ((rivals >> (threadIdx.x & 48)) & 0xFFFFull) == 0;

    // the right image's pixel (y, x1 = x): S along the diagonal x1 + d
    int rkey = 0x7FFFFFFF;
#pragma unroll
    for(int k = 0; k < NPL; k++)
    {
        const int i = i0 + k, xl = x + a.dmin + i;
        if(xl >= 0 && xl < a.W)
            rkey = min(rkey, ((int)S[((size_t)y*a.W + xl)*(size_t)a.D + i] << 8) | i);
    }
    rkey = sgm_row_min(rkey);

    if(lane != 0) return;
    int v = SGM_DISPARITY_SCALE*istar;
    if(istar > 0 && istar < a.D - 1)
    {
        const int before = Sp[istar - 1], after = Sp[istar + 1];
        const int den = max(before + after - 2*smin, 1);
        v += sgm_floor_div((before - after)*SGM_DISPARITY_SCALE + den, 2*den);
    }
    scaled[pixel]      = (int16_t)(unique ? v : -1);
    index_left[pixel]  = (uint8_t)istar;
    index_right[pixel] = (uint8_t)(rkey & 255);         // (no i inside the image: never read)
}

// disparity: in, the scaled index or -1; out, the disparity of step 6
__global__ __launch_bounds__(SGM_CHECK_THREADS)
void sgm_check_kernel(SgmArgs a, int disp12_max_diff, const uint8_t* __restrict__ index_left,
                      const uint8_t* __restrict__ index_right, int16_t* __restrict__ disparity)
{
    const size_t N     = (size_t)a.W*a.H;
    const size_t pixel = (size_t)blockIdx.x*SGM_CHECK_THREADS + threadIdx.x;
    if(pixel >= N) return;
    const int v = disparity[pixel];
    bool valid = v >= 0;
    if(valid && disp12_max_diff >= 0)
    {
        const int y = (int)(pixel / a.W), x = (int)(pixel - (size_t)y*a.W);
        const int istar = index_left[pixel], x1 = x - (a.dmin + istar);
        valid = x1 >= 0 && x1 < a.W;
        if(valid)
        {
            const int i1 = index_right[(size_t)y*a.W + x1];
            valid = abs(i1 - istar) <= disp12_max_diff;
        }
    }
    disparity[pixel] = (int16_t)(valid ? SGM_DISPARITY_SCALE*a.dmin + v : SGM_DISPARITY_SCALE*(a.dmin - 1));
}

////////////////////////////////////////////////////////////////////////////////
// host
////////////////////////////////////////////////////////////////////////////////
template<int NPL>
void sgm_launch_path(const SgmPlan& plan, const SgmArgs& a, int dx, int dy, int first,
                     const uint64_t* census0, const uint64_t* census1, uint16_t* S)
{
    const unsigned grid = dy == 0 ? plan.path_grid_horizontal : plan.path_grid_vertical;
    hipLaunchKernelGGL(sgm_path_kernel<NPL>, dim3(grid), dim3(SGM_PATH_THREADS), 0, NULL, a, dx, dy, first, census0, census1, S);
}
template<int NPL>
void sgm_launch_select(const SgmPlan& plan, const SgmArgs& a, int uniqueness_ratio, const uint16_t* S,
                       uint8_t* index_left, uint8_t* index_right, int16_t* scaled)
{
    hipLaunchKernelGGL(sgm_select_kernel<NPL>, dim3(plan.select_grid), dim3(SGM_SELECT_THREADS), 0, NULL,
                       a, uniqueness_ratio, S, index_left, index_right, scaled);
}

// the one place that says which instantiation a D runs
#define SGM_PER_LANE(NPL, CALL)                                         \
    switch(NPL)                                                         \
    {                                                                   \
    case  1: CALL( 1); break; case  2: CALL( 2); break; case  3: CALL( 3); break; case  4: CALL( 4); break; \
    case  5: CALL( 5); break; case  6: CALL( 6); break; case  7: CALL( 7); break; case  8: CALL( 8); break; \
    case  9: CALL( 9); break; case 10: CALL(10); break; case 11: CALL(11); break; case 12: CALL(12); break; \
    case 13: CALL(13); break; case 14: CALL(14); break; case 15: CALL(15); break; case 16: CALL(16); break; \
    }

// (dx,dy), in the order they are launched; the first 4 are paths = 4
const int SGM_DIRECTIONS[8][2] = { { 1, 0 }, { -1, 0 }, { 0, 1 }, { 0, -1 }, { 1, 1 }, { -1, 1 }, { 1, -1 }, { -1, -1 } };

} // namespace

} // namespace mrcal_amd

using namespace mrcal_amd;

struct mrcal_amd_stereo_sgm
{
    DeviceBuffers mem;
    uint8_t*      pool = NULL;
    SgmPlan       plan;
    SgmParams     params;
    StageEvents<6> stage;           // before the census, and after each stage; the last: after the speckle filter
    // the speckle filter (speckle_filter.hip), on request only: its labels and counts lie in S, which is dead by then
    bool          speckle_on = false;
    SpeckleParams speckle = { 0, 0, 0 };
    SpeckleGrids  speckle_grids;
};

static bool sgm_given(const mrcal_amd_stereo_sgm* m)
{
    if(m != NULL) return true;
    set_error("the stereo matcher is NULL");
    return false;
}

namespace mrcal_amd {

void* sgm_device_image(mrcal_amd_stereo_sgm* m, int i) { return m->pool + m->plan.image[i]; }

// The launch sequence of a match, queued in the NULL stream: census, paths, selection, left-right check and, on
// request, the speckle filter; the disparity image stays on the device. events: the matcher's own, or NULL: nothing is
// recorded
static bool sgm_enqueue(mrcal_amd_stereo_sgm* m, StageEvents<6>* events, int16_t** d_disparity_out)
{
    const SgmPlan& plan = m->plan;
    SgmArgs a;
    a.W = plan.W; a.H = plan.H; a.D = plan.D; a.dmin = m->params.disparity_min; a.P1 = m->params.P1; a.P2 = m->params.P2;
    uint64_t* census[2] = { (uint64_t*)(m->pool + plan.census[0]), (uint64_t*)(m->pool + plan.census[1]) };
    uint16_t* S           = (uint16_t*)(m->pool + plan.S);
    uint8_t*  index_left  = m->pool + plan.index_left;
    uint8_t*  index_right = m->pool + plan.index_right;
    int16_t*  d_disparity = (int16_t*)(m->pool + plan.disparity);
    m->stage.timed = false;

    if(!record(events, 0)) return false;
    const dim3 census_grid(plan.census_grid[0], plan.census_grid[1]), census_block(SGM_CENSUS_TILE_X, 4);
    for(int i = 0; i < 2; i++)
    {
        if(plan.dtype == MRCAL_AMD_IMAGE_UINT8)
            hipLaunchKernelGGL(sgm_census_kernel<uint8_t>,  census_grid, census_block, 0, NULL, plan.W, plan.H, (const uint8_t*)(m->pool + plan.image[i]),  census[i]);
        else
            hipLaunchKernelGGL(sgm_census_kernel<uint16_t>, census_grid, census_block, 0, NULL, plan.W, plan.H, (const uint16_t*)(m->pool + plan.image[i]), census[i]);
    }
    HIP_TRY(hipGetLastError(), return false);
    if(!record(events, 1)) return false;
    for(int r = 0; r < m->params.paths; r++)
    {
#define SGM_CALL(NPL) sgm_launch_path<NPL>(plan, a, SGM_DIRECTIONS[r][0], SGM_DIRECTIONS[r][1], r == 0, census[0], census[1], S)
        SGM_PER_LANE(plan.per_lane, SGM_CALL)
#undef SGM_CALL
    }
    HIP_TRY(hipGetLastError(), return false);
    if(!record(events, 2)) return false;
#define SGM_CALL(NPL) sgm_launch_select<NPL>(plan, a, m->params.uniqueness_ratio, S, index_left, index_right, d_disparity)
    SGM_PER_LANE(plan.per_lane, SGM_CALL)
#undef SGM_CALL
    HIP_TRY(hipGetLastError(), return false);
    if(!record(events, 3)) return false;
    hipLaunchKernelGGL(sgm_check_kernel, dim3(plan.check_grid), dim3(SGM_CHECK_THREADS), 0, NULL,
                       a, m->params.disp12_max_diff, index_left, index_right, d_disparity);
    HIP_TRY(hipGetLastError(), return false);
    if(!record(events, 4)) return false;
    if(m->speckle_on)
    {
        // S is 2 D >= 32 bytes a pixel and nothing reads it after the selection: the filter's 8 bytes a pixel go there
        if(!speckle_filter_device(m->speckle_grids, m->speckle, d_disparity, S)) return false;
        if(!record(events, 5)) return false;
    }
    *d_disparity_out = d_disparity;
    return true;
}

bool sgm_match_device(mrcal_amd_stereo_sgm* m, int16_t* disparity)
{
    int16_t* d_disparity;
    if(!sgm_enqueue(m, &m->stage, &d_disparity)) return false;
    // (the copy waits for the launches)
    HIP_TRY(hipMemcpy(disparity, d_disparity, (size_t)m->plan.W*m->plan.H*sizeof(int16_t), hipMemcpyDeviceToHost), return false);
    m->stage.timed = true;
    return true;
}

// ... without the copy to the host, and without the events: the stages of this path are not reported
bool sgm_match_device_resident(mrcal_amd_stereo_sgm* m, const int16_t** d_disparity_out)
{
    int16_t* d_disparity;
    if(!sgm_enqueue(m, NULL, &d_disparity)) return false;
    *d_disparity_out = d_disparity;
    return true;
}

} // namespace mrcal_amd

extern "C" {

mrcal_amd_stereo_sgm_t*
mrcal_amd_stereo_sgm_create(int width, int height, int dtype, const mrcal_amd_stereo_sgm_params_t* params)
{
    last_error_string().clear();
    if(params == NULL) { set_error("stereo_matching_sgm(): the parameters are NULL"); return NULL; }
    SgmParams p;
    p.disparity_min = params->disparity_min; p.disparity_max = params->disparity_max;
    p.P1 = params->P1; p.P2 = params->P2; p.paths = params->paths;
    p.uniqueness_ratio = params->uniqueness_ratio; p.disp12_max_diff = params->disp12_max_diff;
    std::string why;
    if(!sgm_params_ok(&why, width, height, dtype, p)) { set_error("%s", why.c_str()); return NULL; }
    if(!have_device()) return NULL;
    size_t free_bytes = 0, total_bytes = 0;
    HIP_TRY(hipMemGetInfo(&free_bytes, &total_bytes), return NULL);
    SgmPlan plan;
    if(!sgm_plan(&plan, &why, width, height, dtype, p, free_bytes)) { set_error("%s", why.c_str()); return NULL; }

    mrcal_amd_stereo_sgm* m = new mrcal_amd_stereo_sgm;
    m->plan = plan; m->params = p;
    if(!m->mem.alloc(&m->pool, plan.bytes)) { delete m; return NULL; }
    if(!m->stage.create()) { delete m; return NULL; }
    return m;
}

bool mrcal_amd_stereo_sgm_match(mrcal_amd_stereo_sgm_t* m, const void* image0, const void* image1, int16_t* disparity)
{
    last_error_string().clear();
    if(!sgm_given(m) || !have_device()) return false;
    const size_t n = (size_t)m->plan.W*m->plan.H*image_pixel_bytes(m->plan.dtype);
    HIP_TRY(hipMemcpy(sgm_device_image(m, 0), image0, n, hipMemcpyHostToDevice), return false);
    HIP_TRY(hipMemcpy(sgm_device_image(m, 1), image1, n, hipMemcpyHostToDevice), return false);
    return sgm_match_device(m, disparity);
}

bool mrcal_amd_stereo_sgm_stage_milliseconds(mrcal_amd_stereo_sgm_t* m, float* milliseconds)
{
    last_error_string().clear();
    if(!sgm_given(m)) return false;
    if(!m->stage.timed) { set_error("stereo_matching_sgm(): no match has been made yet"); return false; }
    for(int i = 0; i < 4; i++)
        if(!m->stage.elapsed(&milliseconds[i], i, i+1)) return false;
    return true;
}

bool mrcal_amd_stereo_sgm_set_speckle_filter(mrcal_amd_stereo_sgm_t* m, int window_size, int range)
{
    last_error_string().clear();
    if(!sgm_given(m)) return false;
    SpeckleParams p;
    std::string why;
    if(!speckle_params_of_matcher(&p, &why, m->params.disparity_min, SGM_DISPARITY_SCALE, window_size, range))
    {
        set_error("%s", why.c_str());
        return false;
    }
    m->speckle = p;
    m->speckle_on = window_size > 0;
    if(m->speckle_on) m->speckle_grids = speckle_grids(m->plan.W, m->plan.H);
    m->stage.timed = false;
    return true;
}

bool mrcal_amd_stereo_sgm_speckle_milliseconds(mrcal_amd_stereo_sgm_t* m, float* milliseconds)
{
    last_error_string().clear();
    if(!sgm_given(m)) return false;
    if(!m->stage.timed) { set_error("stereo_matching_sgm(): no match has been made yet"); return false; }
    *milliseconds = 0.f;
    return !m->speckle_on || m->stage.elapsed(milliseconds, 4, 5);
}

void mrcal_amd_stereo_sgm_destroy(mrcal_amd_stereo_sgm_t* m) { delete m; }

} // extern "C"
