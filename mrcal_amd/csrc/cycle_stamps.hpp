// Cycle stamps inside the kernels of the trial step's chain, for the measurement builds (build.sh -D<FLAG> ->
// libmrcal_amd_dev.so; tools/README.md). DEVICE code only. The shipped library defines no flag: every CycleStamps in
// it is the empty one, and a kernel that declares it and calls it compiles to what it compiles to without.
#pragma once
#include <hip/hip_runtime.h>

namespace mrcal_amd {

// One constant per flag, true when build.sh was given -D<FLAG>. These are the only tests of the flags' names in the
// kernels' sources: a kernel says `if constexpr(ASM_TS)`. (The macro makes way for the constant of its name)
#ifdef BOARD_TS       // kernels.hip: the board kernel, into DeviceProblem::debug_ts
#undef BOARD_TS
constexpr bool BOARD_TS = true;
#else
constexpr bool BOARD_TS = false;
#endif
#ifdef ASM_TS         // assembly.hip: a frame's elimination, a pair chunk's reduction
#undef ASM_TS
constexpr bool ASM_TS = true;
#else
constexpr bool ASM_TS = false;
#endif
#ifdef SYRK_TS        // schur.hip: the dense and the sparse SYRK
#undef SYRK_TS
constexpr bool SYRK_TS = true;
#else
constexpr bool SYRK_TS = false;
#endif
#ifdef CHOL_TS        // cholesky_lds.hip: the camera block's factorization in LDS
#undef CHOL_TS
constexpr bool CHOL_TS = true;
#else
constexpr bool CHOL_TS = false;
#endif
#ifdef DIAG16_TS      // chol_diag16.hpp: the 16 x 16 diagonal block, column by column
#undef DIAG16_TS
constexpr bool DIAG16_TS = true;
#else
constexpr bool DIAG16_TS = false;
#endif
#ifdef LCH_TS         // cholesky_large.hip: a panel's diagonal block and its trailing tiles
#undef LCH_TS
constexpr bool LCH_TS = true;
#else
constexpr bool LCH_TS = false;
#endif
#ifdef SPL_TS         // assembly_splined.hip: the splined models' frame assembly
#undef SPL_TS
constexpr bool SPL_TS = true;
#else
constexpr bool SPL_TS = false;
#endif
#ifdef SPLG_TS        // assembly_splined.hip: the gather of a row of A
#undef SPLG_TS
constexpr bool SPLG_TS = true;
#else
constexpr bool SPLG_TS = false;
#endif

// Who reports: item i of n (a frame of the frames, a chunk of the chunks, a panel of the panels ...) - the first,
// the middle one and the last, whatever the problem's size - on the thread the caller names
__device__ __forceinline__ bool stamps_reporter(int i, int n, bool thread = true)
{
    return thread && (i == 0 || i == n/2 || i == n - 1);
}

// The one line a report is:   ts <kernel> <i>/<n>[ <j>/<m>] name=value name=value ...
// (tools/cycle_stamps.py reads it). Marks come first, as the cycles between one and the next; then the totals. The
// names are one string, a word per value; marks past the named ones are m<slot>, totals past them are not printed.
// ONE printf a line: the lines of workgroups that report at the same time do not mix. A report of many values is
// several lines with the same head (the line is built in 256 bytes a lane of scratch, not in as many as 64 marks take)
static __device__ __forceinline__
void stamps_print(const char* kernel, const char* names, int i, int n, int j, int m,
                  const long long* v, int N, int nmarks)
{
    char line[256];
    int  len = 0, nvalues = 0;
    auto put    = [&](char c) { if(len < (int)sizeof(line) - 1) line[len++] = c; };
    auto put_s  = [&](const char* s) { while(*s) put(*s++); };
    auto put_ll = [&](long long x)
    {
        char d[20]; int nd = 0;
        unsigned long long u = (x < 0) ? 0ull - (unsigned long long)x : (unsigned long long)x;
        if(x < 0) put('-');
        do { d[nd++] = (char)('0' + (int)(u % 10)); u /= 10; } while(u != 0);
        while(nd > 0) put(d[--nd]);
    };
    auto head = [&]()
    {
        len = nvalues = 0;
        put_s("ts "); put_s(kernel); put(' '); put_ll(i); put('/'); put_ll(n);
        if(m > 0) { put(' '); put_ll(j); put('/'); put_ll(m); }
    };
    auto flush = [&]() { line[len] = 0; if(nvalues > 0) printf("%s\n", line); };
    head();
    for(int s = (nmarks > 0) ? 1 : 0; s < N; s++)
    {
        while(*names == ' ') names++;
        if(s >= nmarks && *names == 0) break;
        if(len > (int)sizeof(line) - 64) { flush(); head(); }      // (a name and its value: 64 bytes at the most)
        put(' '); nvalues++;
        if(*names != 0) { while(*names != 0 && *names != ' ') put(*names++); }
        else            { put('m'); put_ll(s); }
        put('=');
        put_ll(s < nmarks ? v[s] - v[s-1] : v[s]);
    }
    flush();
}

// MARKS_IN_LOOPS: how many marks there will be is known only as the kernel runs (a mark per pass of a loop). The slots
// are then an array that mark() indexes, in scratch, as the arrays of those kernels always were: a StampSlots that the
// kernel declares beside the CycleStamps and hands to it. Without it every access is to a slot known at compile time
// and the stamps live in registers - scalar ones where the whole wave stamps - as the named locals of those kernels
// did. (An array inside the struct, indexed once by a variable, takes the whole struct to memory - the counter and
// the laps' totals too - and every stamp is then loads and stores inside what it measures: 700 cycles a mark)
template<bool ON, int N, bool MARKS_IN_LOOPS = false> struct CycleStamps;
template<bool ON, int N> struct StampSlots { long long v[N]; };
template<int N> struct StampSlots<false, N> {};

// the shipped one: nothing
template<int N, bool MARKS_IN_LOOPS> struct CycleStamps<false, N, MARKS_IN_LOOPS>
{
    __device__ __forceinline__ explicit CycleStamps(bool = true) {}
    __device__ __forceinline__ explicit CycleStamps(StampSlots<false, N>&, bool = true) {}
    __device__ __forceinline__ void mark() {}
    __device__ __forceinline__ void lap(int) {}
    __device__ __forceinline__ void count(int, long long) {}
    __device__ __forceinline__ long long wall() const { return 0; }
    __device__ __forceinline__ long long slot(int) const { return 0; }
    __device__ __forceinline__ void report(const char*, const char*, int, int, int = 0, int = 0) const {}
};

// N slots. mark() fills them from slot 0 up; lap() and count() add to the slot they name, which a kernel that
// also marks takes from behind its marks. `mine`: whether this thread stamps at all
template<int N> struct CycleStamps<true, N, false>
{
    long long v[N];
    long long last;         // the time of the last stamp, a mark or a lap; at first, of the declaration
    int       nmarks;
    bool      mine;

    __device__ __forceinline__ explicit CycleStamps(bool mine_ = true) : nmarks(0), mine(mine_)
    {
#pragma unroll
        for(int i = 0; i < N; i++) v[i] = 0;
        last = clock64();
    }
    // the clock (clock64(): per XCD) into the next free slot
    __device__ __forceinline__ void mark()
    {
        if(!mine || nmarks >= N) return;
        last = clock64();
#pragma unroll
        for(int k = 0; k < N; k++) if(k == nmarks) v[k] = last;       // (no variable index: see above)
        nmarks++;
    }
    // the cycles since the last stamp, onto slot i
    __device__ __forceinline__ void lap(int i) { if(mine) { const long long now = clock64(); v[i] += now - last; last = now; } }
    // an event counter
    __device__ __forceinline__ void count(int i, long long k) { if(mine) v[i] += k; }
    // the constant 100 MHz clock, the same on every XCD: a workgroup's place in time
    __device__ __forceinline__ long long wall() const { return (long long)wall_clock64(); }
    __device__ __forceinline__ long long slot(int i) const { return v[i]; }
    __device__ __forceinline__ void report(const char* kernel, const char* names, int i, int n, int j = 0, int m = 0) const
    {
        // (a copy: v itself stays in registers)
        long long c[N];
#pragma unroll
        for(int k = 0; k < N; k++) c[k] = v[k];
        stamps_print(kernel, names, i, n, j, m, c, N, nmarks);
    }
};

// marks alone, as many as the kernel's loops make of them (N at the most), into the kernel's StampSlots; a kernel whose
// thread 0 alone reports has thread 0 alone read the clock (`mine`)
template<int N> struct CycleStamps<true, N, true>
{
    long long* v;
    int        nmarks;
    bool       mine;

    __device__ __forceinline__ explicit CycleStamps(StampSlots<true, N>& slots, bool mine_ = true) : v(slots.v), nmarks(0), mine(mine_) {}
    __device__ __forceinline__ void mark() { if(mine && nmarks < N) v[nmarks++] = clock64(); }
    __device__ __forceinline__ void report(const char* kernel, const char* names, int i, int n, int j = 0, int m = 0) const
    {
        stamps_print(kernel, names, i, n, j, m, v, N, nmarks);
    }
};

} // namespace mrcal_amd
