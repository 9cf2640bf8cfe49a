// find_chessboard_corners(): the calibration board detected in one grey image (include/mrcal_amd.h, "chessboard
// corners": the definition, to the bit for a..c). The lattice of part e is csrc/chessboard_grid.cpp, on the host.
//
//   cb_response_kernel<T>  a workgroup a tile of 64 x 16 pixels. It stages the tile and a halo of 6 pixels of I in LDS
//                          (every pixel is read from memory once a tile; outside the image: 0, which no R that is
//                          defined reads), writes the blur B of the tile and a halo of 5 into LDS, and takes the 16
//                          ring samples and the 5 of the centre from there: a wavefront is a row, its lanes read
//                          consecutive words. R is stored as int32, 0 on the border of 6 pixels; the workgroup's
//                          maximum goes into ONE atomicMax on an int, whose result does not depend on the order
//   cb_candidates_kernel   the same tiles of R with a halo of nms_radius. The threshold first: the few pixels that pass
//                          it look at their whole window, with the tie-break of the definition as it is written. A
//                          wavefront's verdicts are one __ballot: the mask word of 64 pixels of a row
//   cb_scan_kernel         ONE workgroup: the counts of the chunks of 16 words (popcounts: no count array is kept), an
//                          inclusive scan of the threads' sums in LDS, the exclusive bases and the total
//   cb_scatter_kernel      a workgroup a chunk, a wavefront a word at a time: the rank of a set bit is the chunk's base,
//                          the popcounts of the chunk's words before its own, the set bits below its lane. Words run
//                          along a row and rows follow each other, so the ranks are row-major. Ranks past max_candidates
//                          are not stored
//   cb_refine_kernel<T>    a wavefront a candidate; the 121 window points two to a lane (k and k + 64), the five sums
//                          added in that order in the lane and then across the lanes by a butterfly (xor 32 .. 1),
//                          which leaves every lane the same bits; all 20 iterations inside the launch. With DESCENT
//                          (p3 of the definition) a wavefront is a corner of the board that was found: the start is
//                          the float up(q) of the corner's position a level above, and the corner moves to this level
//                          when the refinement agrees with its start within CB_DESCENT_AGREEMENT
//   cb_decimate_kernel<T>  level l+1 of the pyramid from level l (p1). Where a row of level l is whole 16-byte words a
//                          lane loads one word of each of two rows (16 or 8 pixels a row) and stores 8 bytes of outputs:
//                          every pixel read once, every output written once, consecutive lanes consecutive words.
//                          Otherwise (a row length that leaves the words unaligned) a lane an output pixel
// Integer bookkeeping, the compaction of point_cloud.hip; no floating-point atomics, no scratch.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <chrono>
#include <string>
#include <vector>
#include "../../include/mrcal_amd.h"
#include "host_state.hpp"
#include "device_memory.hpp"
#include "resident_common.hpp"
#include "chessboard_plan.hpp"
#include "chessboard_grid.hpp"
#include "wave_sum.hpp"

namespace mrcal_amd {

namespace {

__device__ __forceinline__ int cb_absdiff(int a, int b) { return a > b ? a - b : b - a; }

template<class T>
__global__ __launch_bounds__(CB_THREADS)
void cb_response_kernel(int W, int H, unsigned tiles_x, const T* __restrict__ I, int32_t* __restrict__ R, int32_t* __restrict__ Rmax)
{
    constexpr int IW = CB_TX + 2*CB_HALO, IH = CB_TY + 2*CB_HALO;
    constexpr int BW = CB_TX + 2*CB_RING, BH = CB_TY + 2*CB_RING;
    __shared__ T        tile[IH*IW];
    __shared__ int32_t  blur[BH*BW];
    __shared__ int32_t  wave_max[CB_THREADS/64];
    const int x0 = (int)(blockIdx.x % tiles_x)*CB_TX, y0 = (int)(blockIdx.x / tiles_x)*CB_TY;
    for(int k=threadIdx.x; k<IH*IW; k+=CB_THREADS)
    {
        const int ly = k/IW, lx = k - ly*IW;
        const int x = x0 - CB_HALO + lx, y = y0 - CB_HALO + ly;
        tile[k] = (x >= 0 && x < W && y >= 0 && y < H) ? I[(size_t)y*W + x] : (T)0;
    }
    __syncthreads();
    for(int k=threadIdx.x; k<BH*BW; k+=CB_THREADS)
    {
        const int ly = k/BW, lx = k - ly*BW;
        const T* t = tile + (ly + 1)*IW + lx + 1;
        blur[k] =   (int)t[-IW-1] + 2*(int)t[-IW] +   (int)t[-IW+1]
                + 2*(int)t[-1]    + 4*(int)t[0]   + 2*(int)t[1]
                +   (int)t[IW-1]  + 2*(int)t[IW]  +   (int)t[IW+1];
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int x = x0 + lane;
    int best = 0;
    for(int r=wave; r<CB_TY; r+=CB_THREADS/64)
    {
        const int y = y0 + r;
        if(x >= W || y >= H) continue;
        int v = 0;
        if(x >= CB_HALO && x < W - CB_HALO && y >= CB_HALO && y < H - CB_HALO)
        {
            const int32_t* b = blur + (r + CB_RING)*BW + lane + CB_RING;
#define CB_S(dx, dy) b[(dy)*BW + (dx)]
            const int s0  = CB_S( 5, 0), s1  = CB_S( 5, 2), s2  = CB_S( 3, 3), s3  = CB_S( 2, 5),
                      s4  = CB_S( 0, 5), s5  = CB_S(-2, 5), s6  = CB_S(-3, 3), s7  = CB_S(-5, 2),
                      s8  = CB_S(-5, 0), s9  = CB_S(-5,-2), s10 = CB_S(-3,-3), s11 = CB_S(-2,-5),
                      s12 = CB_S( 0,-5), s13 = CB_S( 2,-5), s14 = CB_S( 3,-3), s15 = CB_S( 5,-2);
            const int S5 = CB_S(0,0) + CB_S(1,0) + CB_S(-1,0) + CB_S(0,1) + CB_S(0,-1);
#undef CB_S
            const int SR = cb_absdiff(s0 + s8,  s4 + s12) + cb_absdiff(s1 + s9,  s5 + s13) +
                           cb_absdiff(s2 + s10, s6 + s14) + cb_absdiff(s3 + s11, s7 + s15);
            const int DR = cb_absdiff(s0, s8)  + cb_absdiff(s1, s9)  + cb_absdiff(s2, s10) + cb_absdiff(s3, s11) +
                           cb_absdiff(s4, s12) + cb_absdiff(s5, s13) + cb_absdiff(s6, s14) + cb_absdiff(s7, s15);
            const int S16 = ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7)) + ((s8 + s9) + (s10 + s11)) + ((s12 + s13) + (s14 + s15));
            v = 5*SR - 5*DR - cb_absdiff(5*S16, 16*S5);
        }
        R[(size_t)y*W + x] = v;
        best = v > best ? v : best;
    }
    for(int off=32; off>0; off>>=1)
    {
        const int other = __shfl_xor(best, off);
        best = other > best ? other : best;
    }
    if(lane == 0) wave_max[wave] = best;
    __syncthreads();
    if(threadIdx.x == 0)
    {
        int m = 0;
#pragma unroll
        for(int w=0; w<CB_THREADS/64; w++) m = wave_max[w] > m ? wave_max[w] : m;
        if(m > 0) atomicMax(Rmax, m);
    }
}

__global__ __launch_bounds__(CB_THREADS)
void cb_candidates_kernel(int W, int H, unsigned tiles_x, int radius, int threshold_256, const int32_t* __restrict__ R,
                          const int32_t* __restrict__ Rmax, uint64_t* __restrict__ words)
{
    __shared__ int32_t tile[(CB_TY + 2*CB_NMS_RADIUS_MAX)*(CB_TX + 2*CB_NMS_RADIUS_MAX)];
    const int TW = CB_TX + 2*radius, TH = CB_TY + 2*radius;
    const unsigned tx = blockIdx.x % tiles_x;
    const int x0 = (int)tx*CB_TX, y0 = (int)(blockIdx.x / tiles_x)*CB_TY;
    for(int k=threadIdx.x; k<TH*TW; k+=CB_THREADS)
    {
        const int ly = k/TW, lx = k - ly*TW;
        const int x = x0 - radius + lx, y = y0 - radius + ly;
        tile[k] = (x >= 0 && x < W && y >= 0 && y < H) ? R[(size_t)y*W + x] : 0;
    }
    __syncthreads();
    const long long floor_256 = (long long)threshold_256*(long long)*Rmax;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int x = x0 + lane;
    for(int r=wave; r<CB_TY; r+=CB_THREADS/64)
    {
        const int y = y0 + r;                           // (the same for the whole wavefront)
        if(y >= H) break;
        bool candidate = false;
        if(x < W)
        {
            const int32_t* c = tile + (r + radius)*TW + lane + radius;
            const int v = *c;
            if(v > 0 && 256ll*v > floor_256)
            {
                candidate = true;
                for(int dy=-radius; dy<=radius; dy++)
                    for(int dx=-radius; dx<=radius; dx++)
                    {
                        if(dx == 0 && dy == 0) continue;
                        const int  other = c[dy*TW + dx];
                        const bool after = dy > 0 || (dy == 0 && dx > 0);
                        if(!(other < v || (other == v && after))) candidate = false;
                    }
            }
        }
        const uint64_t word = __ballot(candidate);
        if(lane == 0) words[(size_t)y*tiles_x + tx] = word;
    }
}

__device__ __forceinline__ uint32_t cb_chunk_count(const uint64_t* __restrict__ words, unsigned chunk)
{
    uint32_t n = 0;
#pragma unroll
    for(int q=0; q<CB_CHUNK_WORDS; q++) n += __popcll(words[(size_t)chunk*CB_CHUNK_WORDS + q]);
    return n;
}

// bases [chunks + 1]: the exclusive scan of the chunks' counts, and their total
__global__ __launch_bounds__(CB_SCAN_THREADS)
void cb_scan_kernel(unsigned chunks, unsigned per_thread, const uint64_t* __restrict__ words, uint32_t* __restrict__ bases)
{
    __shared__ uint32_t sum[CB_SCAN_THREADS];
    const unsigned t = threadIdx.x;
    const unsigned lo = t*per_thread < chunks ? t*per_thread : chunks;
    const unsigned hi = lo + per_thread < chunks ? lo + per_thread : chunks;
    uint32_t mine = 0;
    for(unsigned g=lo; g<hi; g++) mine += cb_chunk_count(words, g);
    sum[t] = mine;
    __syncthreads();
    for(unsigned step=1; step<CB_SCAN_THREADS; step*=2)
    {
        const uint32_t add = t >= step ? sum[t - step] : 0;
        __syncthreads();
        sum[t] += add;
        __syncthreads();
    }
    uint32_t at = sum[t] - mine;
    for(unsigned g=lo; g<hi; g++) { bases[g] = at; at += cb_chunk_count(words, g); }
    if(t == CB_SCAN_THREADS - 1) bases[chunks] = sum[t];
}

__global__ __launch_bounds__(CB_THREADS)
void cb_scatter_kernel(int W, unsigned words_per_row, unsigned max_candidates, const uint64_t* __restrict__ words,
                       const uint32_t* __restrict__ bases, const int32_t* __restrict__ R,
                       int32_t* __restrict__ xy, int32_t* __restrict__ response)
{
    __shared__ uint64_t word_of[CB_CHUNK_WORDS];
    __shared__ uint32_t before[CB_CHUNK_WORDS];
    const uint32_t base = bases[blockIdx.x];
    if(bases[blockIdx.x + 1] == base || base >= max_candidates) return;        // (the whole workgroup)
    if(threadIdx.x < CB_CHUNK_WORDS) word_of[threadIdx.x] = words[(size_t)blockIdx.x*CB_CHUNK_WORDS + threadIdx.x];
    __syncthreads();
    if(threadIdx.x == 0)
    {
        uint32_t n = base;
        for(int q=0; q<CB_CHUNK_WORDS; q++) { before[q] = n; n += __popcll(word_of[q]); }
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for(int q=wave; q<CB_CHUNK_WORDS; q+=CB_THREADS/64)
    {
        const uint64_t word = word_of[q];
        if(!((word >> lane) & 1)) continue;
        const uint32_t rank = before[q] + __popcll(word & ((1ull << lane) - 1));
        if(rank >= max_candidates) continue;
        const unsigned w = blockIdx.x*CB_CHUNK_WORDS + q;       // (a word of the image: the bit is set)
        const int y = (int)(w / words_per_row), x = (int)(w % words_per_row)*64 + lane;
        xy[2*rank] = x; xy[2*rank + 1] = y;
        response[rank] = R[(size_t)y*W + x];
    }
}

template<class T>
__device__ __forceinline__ double cb_sample(const T* __restrict__ I, int W, int H, double x, double y)
{
    x = fmin(fmax(x, 0.0), (double)(W - 1));
    y = fmin(fmax(y, 0.0), (double)(H - 1));
    const double fx0 = floor(x), fy0 = floor(y);
    const int ix0 = (int)fx0, iy0 = (int)fy0;
    const int ix1 = ix0 + 1 < W ? ix0 + 1 : W - 1, iy1 = iy0 + 1 < H ? iy0 + 1 : H - 1;
    const double fx = x - fx0, fy = y - fy0;
    const double v00 = (double)I[(size_t)iy0*W + ix0], v01 = (double)I[(size_t)iy0*W + ix1];
    const double v10 = (double)I[(size_t)iy1*W + ix0], v11 = (double)I[(size_t)iy1*W + ix1];
    const double top = v00*(1.0 - fx) + v01*fx, bottom = v10*(1.0 - fx) + v11*fx;
    return top*(1.0 - fy) + bottom*fy;
}

// DESCENT false: the candidates of part d, from their integer pixels xy; q and status are written.
// DESCENT true: the max_candidates corners of the board, from the float up(q) of those whose level is to_level + 1 (the
// others are left alone); q and level are updated where the corner moves to to_level (p3). total, xy, status: not read
template<class T, bool DESCENT>
__global__ __launch_bounds__(CB_THREADS)
void cb_refine_kernel(int W, int H, unsigned max_candidates, const T* __restrict__ I, const uint32_t* __restrict__ total,
                      const int32_t* __restrict__ xy, double* __restrict__ q, int32_t* __restrict__ status,
                      int32_t* __restrict__ level, int to_level)
{
    const unsigned c = blockIdx.x*(CB_THREADS/64) + (threadIdx.x >> 6);
    if(DESCENT)
    {
        if(c >= max_candidates || level[c] != to_level + 1) return;     // (the whole wavefront)
    }
    else
    {
        const unsigned n = *total < max_candidates ? *total : max_candidates;
        if(c >= n) return;                              // (the whole wavefront)
    }
    const int lane = threadIdx.x & 63;
    constexpr int SIDE = 2*CB_WINDOW + 1, POINTS = SIDE*SIDE;
    double wi[2], wj[2], ww[2];
#pragma unroll
    for(int h=0; h<2; h++)
    {
        const int k = lane + 64*h;
        const int j = k/SIDE - CB_WINDOW, i = k - (k/SIDE)*SIDE - CB_WINDOW;
        wi[h] = (double)i; wj[h] = (double)j;
        ww[h] = k < POINTS ? exp(-(wi[h]/CB_WINDOW)*(wi[h]/CB_WINDOW))*exp(-(wj[h]/CB_WINDOW)*(wj[h]/CB_WINDOW)) : 0.0;
    }
    const double startx = DESCENT ? 2.0*q[2*c]     + 0.5 : (double)xy[2*c];
    const double starty = DESCENT ? 2.0*q[2*c + 1] + 0.5 : (double)xy[2*c + 1];
    double qx = startx, qy = starty;
    int st = CB_STATUS_OK;
    for(int it=0; it<CB_REFINE_ITERATIONS; it++)
    {
        double a = 0.0, b = 0.0, cc = 0.0, bx = 0.0, by = 0.0;
#pragma unroll
        for(int h=0; h<2; h++)
        {
            if(lane + 64*h >= POINTS) continue;
            const double px = qx + wi[h], py = qy + wj[h];
            const double gx = (cb_sample(I, W, H, px + 1.0, py) - cb_sample(I, W, H, px - 1.0, py))/2.0;
            const double gy = (cb_sample(I, W, H, px, py + 1.0) - cb_sample(I, W, H, px, py - 1.0))/2.0;
            const double gxx = ww[h]*gx*gx, gxy = ww[h]*gx*gy, gyy = ww[h]*gy*gy;
            a += gxx; b += gxy; cc += gyy;
            bx += gxx*wi[h] + gxy*wj[h];
            by += gxy*wi[h] + gyy*wj[h];
        }
        a = wave_sum(a); b = wave_sum(b); cc = wave_sum(cc); bx = wave_sum(bx); by = wave_sum(by);
        const double det = a*cc - b*b, trace = a + cc;
        if(!(det > 1e-10*trace*trace)) { st = CB_STATUS_SINGULAR; break; }
        const double dx = (cc*bx - b*by)/det, dy = (a*by - b*bx)/det;
        qx += dx; qy += dy;
        if(!(fabs(qx - startx) <= 3.5 && fabs(qy - starty) <= 3.5)) { st = CB_STATUS_LEFT; break; }
        if(dx*dx + dy*dy < 1e-5*1e-5) break;
    }
    if(DESCENT)
    {
        // (every lane holds the same qx, qy and st)
        const bool moves = st == CB_STATUS_OK && fmax(fabs(qx - startx), fabs(qy - starty)) <= CB_DESCENT_AGREEMENT;
        if(lane == 0 && moves) { q[2*c] = qx; q[2*c + 1] = qy; level[c] = to_level; }
    }
    else if(lane == 0)
    {
        q[2*c]     = st == CB_STATUS_OK ? qx : (double)NAN;
        q[2*c + 1] = st == CB_STATUS_OK ? qy : (double)NAN;
        status[c]  = st;
    }
}

__device__ __forceinline__ uint32_t cb_quad(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return (a + b + c + d + 2u) >> 2; }

// two rows' words -> the word of outputs: 4 pixels of uint8 each, or 2 of uint16
template<class T>
__device__ __forceinline__ uint32_t cb_decimate_words(uint32_t t0, uint32_t t1, uint32_t b0, uint32_t b1);
template<>
__device__ __forceinline__ uint32_t cb_decimate_words<uint8_t>(uint32_t t0, uint32_t t1, uint32_t b0, uint32_t b1)
{
    return  cb_quad(t0 & 255u, (t0 >> 8) & 255u, b0 & 255u, (b0 >> 8) & 255u)
         | (cb_quad((t0 >> 16) & 255u, t0 >> 24, (b0 >> 16) & 255u, b0 >> 24) << 8)
         | (cb_quad(t1 & 255u, (t1 >> 8) & 255u, b1 & 255u, (b1 >> 8) & 255u) << 16)
         | (cb_quad((t1 >> 16) & 255u, t1 >> 24, (b1 >> 16) & 255u, b1 >> 24) << 24);
}
template<>
__device__ __forceinline__ uint32_t cb_decimate_words<uint16_t>(uint32_t t0, uint32_t t1, uint32_t b0, uint32_t b1)
{
    return cb_quad(t0 & 65535u, t0 >> 16, b0 & 65535u, b0 >> 16) | (cb_quad(t1 & 65535u, t1 >> 16, b1 & 65535u, b1 >> 16) << 16);
}

// in: (H_in, W_in) with W_in sizeof(T) a multiple of 16; out: (H_out, W_in/2). words_per_row = W_in sizeof(T)/16
template<class T>
__global__ __launch_bounds__(CB_THREADS)
void cb_decimate_wide_kernel(unsigned words_per_row, unsigned H_out, const uint4* __restrict__ in, uint2* __restrict__ out)
{
    const size_t k = (size_t)blockIdx.x*CB_THREADS + threadIdx.x;
    if(k >= (size_t)words_per_row*H_out) return;
    const size_t y = k/words_per_row, w = k - y*words_per_row;
    const uint4 t = in[(2*y)*words_per_row + w], b = in[(2*y + 1)*words_per_row + w];
    uint2 o;
    o.x = cb_decimate_words<T>(t.x, t.y, b.x, b.y);
    o.y = cb_decimate_words<T>(t.z, t.w, b.z, b.w);
    out[k] = o;
}

// any row length: a lane an output pixel
template<class T>
__global__ __launch_bounds__(CB_THREADS)
void cb_decimate_kernel(int W_in, int W_out, int H_out, const T* __restrict__ in, T* __restrict__ out)
{
    const size_t k = (size_t)blockIdx.x*CB_THREADS + threadIdx.x;
    if(k >= (size_t)W_out*H_out) return;
    const size_t y = k/W_out, x = k - y*W_out;
    const T* t = in + (2*y)*W_in + 2*x;
    out[k] = (T)cb_quad(t[0], t[1], t[W_in], t[W_in + 1]);
}

} // namespace

} // namespace mrcal_amd

using namespace mrcal_amd;

struct mrcal_amd_chessboard_detector
{
    DeviceBuffers  mem;
    uint8_t*       pool = NULL;
    ChessboardPyramidPlan pyramid;      // pyramid.level[0] is the plan of a detector without a pyramid
    // the last call
    int            N = -1;              // candidates kept
    bool           overflow = false;
    float          grid_ms = 0.f;
    int            level = 0;           // the level that was looked at last: what N, q, the response and the stages are of
    std::vector<double>  q;
    std::vector<int32_t> response, status;
    StageEvents<5> events;             // around the upload, after the response, the candidates, the refinement
    // ... with a pyramid. events 0 and 1 are around the start of the level looked at last then
    bool           pyramid_ran = false;
    float          level_ms[CB_MAX_LEVELS + 1] = {};               // the host's clock around each level tried: a..e and the read-back
    StageEvents<6> pyramid_events;     // around the upload, the decimation, the descent
    bool           descended = false;
};

static bool cb_given(const mrcal_amd_chessboard_detector* d)
{
    if(d != NULL) return true;
    set_error("find_chessboard_corners(): the detector is NULL");
    return false;
}

// parts a..d of a level, into the detector's own arrays. image: the host's, uploaded first (level 0, and what a
// detector without a pyramid does); NULL: the level's image is on the device already
static bool cb_run_level(mrcal_amd_chessboard_detector* d, int level, const void* image)
{
    d->N = -1;
    d->grid_ms = 0.f;
    d->level = level;
    const ChessboardPlan& p = d->pyramid.level[level];
    uint8_t*  d_image = d->pool + p.image;
    int32_t*  R       = (int32_t*)(d->pool + p.response);
    uint64_t* words   = (uint64_t*)(d->pool + p.words);
    uint32_t* bases   = (uint32_t*)(d->pool + p.bases);
    int32_t*  Rmax    = (int32_t*)(d->pool + p.response_max);
    int32_t*  xy      = (int32_t*)(d->pool + p.xy);
    int32_t*  cr      = (int32_t*)(d->pool + p.candidate_response);
    double*   q       = (double*)(d->pool + p.q);
    int32_t*  status  = (int32_t*)(d->pool + p.status);
    const dim3 tiles(p.tiles_x*p.tiles_y), block(CB_THREADS);

    if(!d->events.record(0)) return false;
    if(image != NULL)
        HIP_TRY(hipMemcpyAsync(d_image, image, (size_t)p.W*p.H*p.bytes_per_pixel, hipMemcpyHostToDevice, NULL), (void)hipDeviceSynchronize(); return false);
    if(!d->events.record(1)) { (void)hipDeviceSynchronize(); return false; }
    if(d->pyramid.levels > 0)
    {
        // the levels share the mask words, and the words of a chunk past a level's own are never written by it: what
        // another level left there would be counted
        const size_t used = (size_t)p.words_per_row*(size_t)p.H, all = (size_t)p.chunks*CB_CHUNK_WORDS;
        if(all > used)
            HIP_TRY(hipMemsetAsync(words + used, 0, (all - used)*sizeof(uint64_t), NULL), (void)hipDeviceSynchronize(); return false);
    }
    HIP_TRY(hipMemsetAsync(Rmax, 0, sizeof(int32_t), NULL), (void)hipDeviceSynchronize(); return false);
    if(p.bytes_per_pixel == 1) hipLaunchKernelGGL(cb_response_kernel<uint8_t>,  tiles, block, 0, NULL, p.W, p.H, p.tiles_x, (const uint8_t*)d_image,  R, Rmax);
    else                       hipLaunchKernelGGL(cb_response_kernel<uint16_t>, tiles, block, 0, NULL, p.W, p.H, p.tiles_x, (const uint16_t*)d_image, R, Rmax);
    HIP_TRY(hipGetLastError(), (void)hipDeviceSynchronize(); return false);
    if(!d->events.record(2)) { (void)hipDeviceSynchronize(); return false; }
    hipLaunchKernelGGL(cb_candidates_kernel, tiles, block, 0, NULL, p.W, p.H, p.tiles_x, p.nms_radius, p.threshold_256, R, Rmax, words);
    HIP_TRY(hipGetLastError(), (void)hipDeviceSynchronize(); return false);
    hipLaunchKernelGGL(cb_scan_kernel, dim3(1), dim3(CB_SCAN_THREADS), 0, NULL, p.chunks, p.scan_per_thread, words, bases);
    HIP_TRY(hipGetLastError(), (void)hipDeviceSynchronize(); return false);
    hipLaunchKernelGGL(cb_scatter_kernel, dim3(p.chunks), block, 0, NULL, p.W, p.words_per_row, (unsigned)p.max_candidates, words, bases, R, xy, cr);
    HIP_TRY(hipGetLastError(), (void)hipDeviceSynchronize(); return false);
    if(!d->events.record(3)) { (void)hipDeviceSynchronize(); return false; }
    if(p.bytes_per_pixel == 1) hipLaunchKernelGGL(HIP_KERNEL_NAME(cb_refine_kernel<uint8_t,  false>), dim3(p.refine_groups), block, 0, NULL, p.W, p.H, (unsigned)p.max_candidates, (const uint8_t*)d_image,  bases + p.chunks, xy, q, status, (int32_t*)NULL, 0);
    else                       hipLaunchKernelGGL(HIP_KERNEL_NAME(cb_refine_kernel<uint16_t, false>), dim3(p.refine_groups), block, 0, NULL, p.W, p.H, (unsigned)p.max_candidates, (const uint16_t*)d_image, bases + p.chunks, xy, q, status, (int32_t*)NULL, 0);
    HIP_TRY(hipGetLastError(), (void)hipDeviceSynchronize(); return false);
    if(!d->events.record(4)) { (void)hipDeviceSynchronize(); return false; }

    uint32_t total = 0;
    // (the copy waits for the launches)
    HIP_TRY(hipMemcpy(&total, bases + p.chunks, sizeof(total), hipMemcpyDeviceToHost), (void)hipDeviceSynchronize(); return false);
    if((size_t)total > (size_t)p.W*p.H) { set_error("find_chessboard_corners(): internal error: %u candidates of %d x %d pixels", total, p.W, p.H); return false; }
    const size_t N = total < (uint32_t)p.max_candidates ? total : (uint32_t)p.max_candidates;
    d->q.assign(2*N, 0.0); d->response.assign(N, 0); d->status.assign(N, 0);
    if(N > 0)
    {
        HIP_TRY(hipMemcpy(d->q.data(),        q,      2*N*sizeof(double), hipMemcpyDeviceToHost), return false);
        HIP_TRY(hipMemcpy(d->response.data(), cr,     N*sizeof(int32_t),  hipMemcpyDeviceToHost), return false);
        HIP_TRY(hipMemcpy(d->status.data(),   status, N*sizeof(int32_t),  hipMemcpyDeviceToHost), return false);
    }
    d->overflow = total > (uint32_t)p.max_candidates;
    d->N = (int)N;
    return true;
}

// level 0 alone: what a detector without a pyramid does, whatever levels this one has
static bool cb_run(mrcal_amd_chessboard_detector* d, const void* image)
{
    d->N = -1;
    d->pyramid_ran = false;
    if(image == NULL) { set_error("find_chessboard_corners(): the image is NULL"); return false; }
    if(!have_device()) return false;
    return cb_run_level(d, 0, image);
}

// p1: the levels 1..n from the level-0 image on the device
static bool cb_decimate(mrcal_amd_chessboard_detector* d)
{
    const ChessboardPyramidPlan& pp = d->pyramid;
    for(int l=1; l<=pp.levels; l++)
    {
        const ChessboardPlan& from = pp.level[l - 1];
        const ChessboardPlan& to   = pp.level[l];
        const uint8_t* in  = d->pool + from.image;
        uint8_t*       out = d->pool + to.image;
        const dim3 groups(pp.decimate_groups[l]), block(CB_THREADS);
        const bool u8 = to.bytes_per_pixel == 1;
        if(pp.decimate_wide[l])
        {
            const unsigned words_per_row = (unsigned)((size_t)from.W*from.bytes_per_pixel/CB_DECIMATE_BYTES);
            if(u8) hipLaunchKernelGGL(cb_decimate_wide_kernel<uint8_t>,  groups, block, 0, NULL, words_per_row, (unsigned)to.H, (const uint4*)in, (uint2*)out);
            else   hipLaunchKernelGGL(cb_decimate_wide_kernel<uint16_t>, groups, block, 0, NULL, words_per_row, (unsigned)to.H, (const uint4*)in, (uint2*)out);
        }
        else
        {
            if(u8) hipLaunchKernelGGL(cb_decimate_kernel<uint8_t>,  groups, block, 0, NULL, from.W, to.W, to.H, (const uint8_t*)in,  (uint8_t*)out);
            else   hipLaunchKernelGGL(cb_decimate_kernel<uint16_t>, groups, block, 0, NULL, from.W, to.W, to.H, (const uint16_t*)in, (uint16_t*)out);
        }
        HIP_TRY(hipGetLastError(), (void)hipDeviceSynchronize(); return false);
    }
    return true;
}

// p2 and p3. corners (board_height, board_width, 2) and levels are written when *found
static bool cb_find_board_pyramid(mrcal_amd_chessboard_detector* d, const void* image, int board_width, int board_height,
                                  double* corners, int32_t* levels, int* detection_level, int* found)
{
    d->N = -1;
    d->pyramid_ran = false;
    d->descended = false;
    if(image == NULL) { set_error("find_chessboard_corners(): the image is NULL"); return false; }
    if(!have_device()) return false;
    const ChessboardPyramidPlan& pp = d->pyramid;
    const ChessboardPlan& p0 = pp.level[0];
    for(float& ms : d->level_ms) ms = 0.f;
    *found = 0;
    *detection_level = -1;
    // (made at the first call of this kind: a detector that is never asked for levels has none of them)
    if(!d->pyramid_events.create()) return false;

    if(!d->pyramid_events.record(0)) return false;
    HIP_TRY(hipMemcpyAsync(d->pool + p0.image, image, (size_t)p0.W*p0.H*p0.bytes_per_pixel, hipMemcpyHostToDevice, NULL), (void)hipDeviceSynchronize(); return false);
    if(!d->pyramid_events.record(1)) { (void)hipDeviceSynchronize(); return false; }
    if(!d->pyramid_events.record(2)) { (void)hipDeviceSynchronize(); return false; }
    if(!cb_decimate(d)) return false;
    if(!d->pyramid_events.record(3)) { (void)hipDeviceSynchronize(); return false; }

    const int n = board_width*board_height;
    int L = pp.levels;
    for(; L >= 0; L--)
    {
        const auto t0 = std::chrono::steady_clock::now();
        if(!cb_run_level(d, L, NULL)) return false;
        const auto t1 = std::chrono::steady_clock::now();
        const bool here = chessboard_grid(d->N, d->q.data(), d->response.data(), d->status.data(), board_width, board_height, corners);
        const auto t2 = std::chrono::steady_clock::now();
        d->grid_ms     = std::chrono::duration<float, std::milli>(t2 - t1).count();
        d->level_ms[L] = std::chrono::duration<float, std::milli>(t2 - t0).count();
        if(here) break;
    }
    d->pyramid_ran = true;
    if(L < 0) return true;                              // (no board at any level: no error. Level 0 was looked at last)
    *found = 1;
    *detection_level = L;
    for(int c=0; c<n; c++) levels[c] = L;
    if(L == 0) return true;

    // the board's corners are candidates of this level: there are no more of them than max_candidates
    if(n > p0.max_candidates) { set_error("find_chessboard_corners(): internal error: a board of %d corners among %d candidates", n, p0.max_candidates); return false; }
    double*  dq     = (double*)(d->pool + pp.descent_q);
    int32_t* dlevel = (int32_t*)(d->pool + pp.descent_level);
    if(!d->pyramid_events.record(4)) return false;
    HIP_TRY(hipMemcpyAsync(dq,     corners, (size_t)n*2*sizeof(double), hipMemcpyHostToDevice, NULL), (void)hipDeviceSynchronize(); return false);
    HIP_TRY(hipMemcpyAsync(dlevel, levels,  (size_t)n*sizeof(int32_t),  hipMemcpyHostToDevice, NULL), (void)hipDeviceSynchronize(); return false);
    const dim3 groups(((unsigned)n + CB_THREADS/64 - 1)/(CB_THREADS/64)), block(CB_THREADS);
    for(int l=L-1; l>=0; l--)
    {
        const ChessboardPlan& p = pp.level[l];
        const uint8_t* I = d->pool + p.image;
        if(p.bytes_per_pixel == 1) hipLaunchKernelGGL(HIP_KERNEL_NAME(cb_refine_kernel<uint8_t,  true>), groups, block, 0, NULL, p.W, p.H, (unsigned)n, (const uint8_t*)I,  (const uint32_t*)NULL, (const int32_t*)NULL, dq, (int32_t*)NULL, dlevel, l);
        else                       hipLaunchKernelGGL(HIP_KERNEL_NAME(cb_refine_kernel<uint16_t, true>), groups, block, 0, NULL, p.W, p.H, (unsigned)n, (const uint16_t*)I, (const uint32_t*)NULL, (const int32_t*)NULL, dq, (int32_t*)NULL, dlevel, l);
        HIP_TRY(hipGetLastError(), (void)hipDeviceSynchronize(); return false);
    }
    if(!d->pyramid_events.record(5)) { (void)hipDeviceSynchronize(); return false; }
    // (the copies wait for the launches)
    HIP_TRY(hipMemcpy(corners, dq,     (size_t)n*2*sizeof(double), hipMemcpyDeviceToHost), (void)hipDeviceSynchronize(); return false);
    HIP_TRY(hipMemcpy(levels,  dlevel, (size_t)n*sizeof(int32_t),  hipMemcpyDeviceToHost), (void)hipDeviceSynchronize(); return false);
    d->descended = true;
    // the last accepted position, carried to level 0: up(q) = 2 q + 0.5, once a level
    for(int c=0; c<n; c++)
    {
        if(levels[c] < 0 || levels[c] > L) { set_error("find_chessboard_corners(): internal error: corner %d at level %d", c, levels[c]); return false; }
        for(int l=0; l<levels[c]; l++) { corners[2*c] = 2.0*corners[2*c] + 0.5; corners[2*c + 1] = 2.0*corners[2*c + 1] + 0.5; }
    }
    return true;
}

static mrcal_amd_chessboard_detector* cb_create(int width, int height, int bytes_per_pixel, const mrcal_amd_chessboard_params_t* params,
                                                int pyramid_levels, size_t free_device_bytes)
{
    last_error_string().clear();
    if(params == NULL) { set_error("find_chessboard_corners(): the parameters are NULL"); return NULL; }
    std::string why;
    ChessboardPyramidPlan plan;
    // (the refusals that need no device first)
    if(!chessboard_pyramid_plan(&plan, &why, width, height, bytes_per_pixel, params->threshold_256, params->nms_radius, params->max_candidates,
                                pyramid_levels, free_device_bytes != 0 ? free_device_bytes : SIZE_MAX))
    {
        set_error("%s", why.c_str());
        return NULL;
    }
    if(!have_device()) return NULL;
    if(free_device_bytes == 0)
    {
        size_t free_bytes = 0, total_bytes = 0;
        HIP_TRY(hipMemGetInfo(&free_bytes, &total_bytes), return NULL);
        if(!chessboard_pyramid_plan(&plan, &why, width, height, bytes_per_pixel, params->threshold_256, params->nms_radius, params->max_candidates,
                                    pyramid_levels, free_bytes))
        {
            set_error("%s", why.c_str());
            return NULL;
        }
    }
    mrcal_amd_chessboard_detector* d = new mrcal_amd_chessboard_detector;
    d->pyramid = plan;
    if(!d->mem.alloc(&d->pool, plan.bytes)) { delete d; return NULL; }
    // (the words past the image's are never written: no bit of them may be set)
    HIP_TRY(hipMemset(d->pool + plan.level[0].words, 0, plan.level[0].bases - plan.level[0].words), delete d; return NULL);
    if(!d->events.create()) { delete d; return NULL; }
    return d;
}

extern "C" {

mrcal_amd_chessboard_detector_t*
mrcal_amd_chessboard_detector_create(int width, int height, int bytes_per_pixel,
                                     const mrcal_amd_chessboard_params_t* params, size_t free_device_bytes)
{
    return cb_create(width, height, bytes_per_pixel, params, 0, free_device_bytes);
}

mrcal_amd_chessboard_detector_t*
mrcal_amd_chessboard_detector_create_pyramid(int width, int height, int bytes_per_pixel,
                                             const mrcal_amd_chessboard_params_t* params, int pyramid_levels, size_t free_device_bytes)
{
    return cb_create(width, height, bytes_per_pixel, params, pyramid_levels, free_device_bytes);
}

bool mrcal_amd_chessboard_detector_candidates(mrcal_amd_chessboard_detector_t* d, const void* image,
                                              int* N, int* overflow, double* q, int32_t* response, int32_t* status)
{
    last_error_string().clear();
    if(!cb_given(d)) return false;
    if(N == NULL || overflow == NULL) { set_error("find_chessboard_corners(): an argument is NULL"); return false; }
    if(!cb_run(d, image)) return false;
    const size_t n = (size_t)d->N;
    if(n > 0 && q != NULL)        memcpy(q,        d->q.data(),        2*n*sizeof(double));
    if(n > 0 && response != NULL) memcpy(response, d->response.data(), n*sizeof(int32_t));
    if(n > 0 && status != NULL)   memcpy(status,   d->status.data(),   n*sizeof(int32_t));
    *N = d->N;
    *overflow = d->overflow ? 1 : 0;
    return true;
}

bool mrcal_amd_chessboard_detector_find_board(mrcal_amd_chessboard_detector_t* d, const void* image,
                                              int board_width, int board_height, int* found, double* corners)
{
    last_error_string().clear();
    if(!cb_given(d)) return false;
    if(found == NULL || corners == NULL) { set_error("find_chessboard_corners(): an argument is NULL"); return false; }
    std::string why;
    if(!chessboard_board_ok(&why, board_width, board_height)) { set_error("%s", why.c_str()); return false; }
    if(!cb_run(d, image)) return false;
    const auto t0 = std::chrono::steady_clock::now();
    *found = chessboard_grid(d->N, d->q.data(), d->response.data(), d->status.data(), board_width, board_height, corners) ? 1 : 0;
    d->grid_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return true;
}

bool mrcal_amd_chessboard_detector_read_response(mrcal_amd_chessboard_detector_t* d, int32_t* response, int32_t* response_max,
                                                 int32_t* candidate_xy)
{
    last_error_string().clear();
    if(!cb_given(d)) return false;
    if(d->N < 0) { set_error("find_chessboard_corners(): no image has been looked at yet"); return false; }
    const ChessboardPlan& p = d->pyramid.level[d->level];       // (of the level looked at last: level 0 without a pyramid)
    if(response != NULL)     HIP_TRY(hipMemcpy(response, d->pool + p.response, (size_t)p.W*p.H*sizeof(int32_t), hipMemcpyDeviceToHost), return false);
    if(response_max != NULL) HIP_TRY(hipMemcpy(response_max, d->pool + p.response_max, sizeof(int32_t), hipMemcpyDeviceToHost), return false);
    if(candidate_xy != NULL && d->N > 0) HIP_TRY(hipMemcpy(candidate_xy, d->pool + p.xy, (size_t)d->N*2*sizeof(int32_t), hipMemcpyDeviceToHost), return false);
    return true;
}

bool mrcal_amd_chessboard_detector_stage_milliseconds(mrcal_amd_chessboard_detector_t* d, float* milliseconds)
{
    last_error_string().clear();
    if(!cb_given(d)) return false;
    if(d->N < 0) { set_error("find_chessboard_corners(): no image has been looked at yet"); return false; }
    for(int i = 0; i < 4; i++)
        if(!d->events.elapsed(&milliseconds[i], i, i + 1)) return false;
    // (with a pyramid the image was uploaded once, before the levels)
    if(d->pyramid_ran && !d->pyramid_events.elapsed(&milliseconds[0], 0, 1)) return false;
    milliseconds[4] = d->grid_ms;
    return true;
}

bool mrcal_amd_chessboard_detector_find_board_pyramid(mrcal_amd_chessboard_detector_t* d, const void* image,
                                                      int board_width, int board_height, double* corners, int32_t* levels,
                                                      int* detection_level, int* found)
{
    last_error_string().clear();
    if(!cb_given(d)) return false;
    if(found == NULL || corners == NULL || levels == NULL || detection_level == NULL) { set_error("find_chessboard_corners(): an argument is NULL"); return false; }
    std::string why;
    if(!chessboard_board_ok(&why, board_width, board_height)) { set_error("%s", why.c_str()); return false; }
    return cb_find_board_pyramid(d, image, board_width, board_height, corners, levels, detection_level, found);
}

bool mrcal_amd_chessboard_detector_read_level(mrcal_amd_chessboard_detector_t* d, int level, void* image_out)
{
    last_error_string().clear();
    if(!cb_given(d)) return false;
    if(image_out == NULL) { set_error("find_chessboard_corners(): an argument is NULL"); return false; }
    if(d->N < 0) { set_error("find_chessboard_corners(): no image has been looked at yet"); return false; }
    // (the levels above 0 are made by _find_board_pyramid() alone)
    if(level < 0 || level > (d->pyramid_ran ? d->pyramid.levels : 0))
    {
        set_error("find_chessboard_corners(): the last call made the levels 0..%d, and level %d was asked for", d->pyramid_ran ? d->pyramid.levels : 0, level);
        return false;
    }
    const ChessboardPlan& p = d->pyramid.level[level];
    HIP_TRY(hipMemcpy(image_out, d->pool + p.image, (size_t)p.W*p.H*p.bytes_per_pixel, hipMemcpyDeviceToHost), return false);
    return true;
}

bool mrcal_amd_chessboard_detector_pyramid_milliseconds(mrcal_amd_chessboard_detector_t* d, float* decimate, float* descent, float* per_level)
{
    last_error_string().clear();
    if(!cb_given(d)) return false;
    if(decimate == NULL || descent == NULL || per_level == NULL) { set_error("find_chessboard_corners(): an argument is NULL"); return false; }
    if(d->N < 0 || !d->pyramid_ran) { set_error("find_chessboard_corners(): no image has been looked at through the pyramid yet"); return false; }
    if(!d->pyramid_events.elapsed(decimate, 2, 3)) return false;
    *descent = 0.f;
    if(d->descended && !d->pyramid_events.elapsed(descent, 4, 5)) return false;
    for(int l=0; l<=d->pyramid.levels; l++) per_level[l] = d->level_ms[l];
    return true;
}

void mrcal_amd_chessboard_detector_destroy(mrcal_amd_chessboard_detector_t* d) { delete d; }

bool mrcal_amd_chessboard_grid(int N, const double* q, const int32_t* response, const int32_t* status,
                               int board_width, int board_height, int* found, double* corners)
{
    last_error_string().clear();
    if(N < 0 || (N > 0 && q == NULL) || found == NULL || corners == NULL) { set_error("find_chessboard_corners(): an argument is NULL"); return false; }
    std::string why;
    if(!chessboard_board_ok(&why, board_width, board_height)) { set_error("%s", why.c_str()); return false; }
    *found = chessboard_grid(N, q, response, status, board_width, board_height, corners) ? 1 : 0;
    return true;
}

} // extern "C"
