// The work lists of the regional residual statistics (include/mrcal_amd.h, "regional statistics"; the kernels:
// regional_stats.hip). HOST code, nothing of HIP in it: tests/hostcheck/regional_stats_plan_check.cpp drives it
// under ASan + UBSan.
//
// All the cameras of a problem are binned in one pass: the cells of camera c are the keys cell0[c] ..
// cell0[c + 1] - 1, row-major (key = cell0[c] + j*gridn_width + i). The corners are taken in chunks of RS_CHUNK
// consecutive corners (corner g = iobservation*H*W + icorner, the order of the measurements):
//   hist   [Nchunks][Ncells] int32   entries of a chunk per cell, then (scanned down the chunks) the entries of that
//                                    cell in all EARLIER chunks
//   start  [Ncells + 1]      int32   the first entry of each cell in the sorted list (one workgroup scans them)
//   sorted [Nentries_max]    int32   the measurement index of the x residual of every entry, cell by cell, ascending
// A corner is an entry of every cell whose two inequalities it meets. In exact arithmetic that is at most one cell;
// with the centres rounded a corner within an ulp of a border can meet those of the two cells either side of it, in x
// and in y: RS_SLOTS = 4 keys a corner at the most, and Nentries_max = 4 Ncorners.
#pragma once
#include <stdint.h>
#include <math.h>
#include <string>
#include <vector>

namespace mrcal_amd {

constexpr int RS_CHUNK        = 2048;        // corners of a chunk: one wavefront ranks them, 64 at a time
constexpr int RS_SLOTS        = 4;           // keys a corner can have
constexpr int RS_SCAN_THREADS = 1024;        // the one workgroup that scans the cells
constexpr int RS_MAX_CELLS    = 1 << 20;     // of all cameras together
constexpr int RS_SMALL_COUNT  = 5;           // a cell with this many values or fewer reports mean = stdev = 0

// what the kernels know of one camera
struct RegionalCamera
{
    int32_t gridn_width, gridn_height;
    int32_t cell0;                   // the key of cell (0,0)
    int32_t centre0;                 // where cx[gridn_width], then cy[gridn_height] start in the table of centres
    double  half_w, half_h;          // wcell/2, hcell/2
    double  wcell, hcell;
};

struct RegionalStatsPlan
{
    int     Ncameras = 0;
    int64_t Ncorners = 0;            // Nobservations_board * H * W
    int64_t Nentries_max = 0;        // RS_SLOTS * Ncorners
    int     Nchunks = 0;
    int     Ncells = 0;
    int64_t hist_ints = 0;           // Nchunks * Ncells
    int     scan_items_per_thread = 0;       // ceil(Ncells / RS_SCAN_THREADS)
    std::vector<RegionalCamera> cameras;
    std::vector<double>         centres;     // per camera cx[], cy[]
};

// THE formula of a centre: centre i of n over an imager of `size` pixels is i*((size-1)/(n-1)), one division and one
// multiplication in double, and size-1 itself for i = n-1: np.linspace(0, size-1, n)
inline double regional_cell_centre(int i, int n, int size)
{
    if(i == n - 1) return (double)(size - 1);
    const double step = (double)(size - 1)/(double)(n - 1);
    return (double)i*step;
}

// gridn_height <= 0: every camera's own int(round(H/W*gridn_width)), half to even. false: *err says why
inline bool plan_regional_stats(RegionalStatsPlan* plan, int Ncameras, const int* imagersizes /* [Ncameras][2] */,
                                int64_t Nobservations_board, int corners_per_board, int gridn_width, int gridn_height,
                                std::string* err)
{
    *plan = RegionalStatsPlan();
    if(Ncameras <= 0) { *err = "no cameras"; return false; }
    if(gridn_width < 2)
    {
        *err = "gridn_width must be >= 2: got " + std::to_string(gridn_width);
        return false;
    }
    plan->Ncameras = Ncameras;
    int64_t Ncells = 0;
    for(int c = 0; c < Ncameras; c++)
    {
        const int W = imagersizes[2*c], H = imagersizes[2*c + 1];
        if(W < 2 || H < 2)
        {
            *err = "camera " + std::to_string(c) + ": the imager must be at least 2x2 pixels";
            return false;
        }
        int64_t gh = gridn_height;
        if(gridn_height <= 0) gh = (int64_t)nearbyint((double)H/(double)W*(double)gridn_width);
        if(gh < 2)
        {
            *err = "gridn_height must be >= 2: got " + std::to_string(gh) + " for camera " + std::to_string(c);
            return false;
        }
        if(gh > RS_MAX_CELLS || Ncells + (int64_t)gridn_width*gh > RS_MAX_CELLS)
        {
            *err = "the grids of all cameras together have more than " + std::to_string(RS_MAX_CELLS) + " cells";
            return false;
        }
        RegionalCamera cam;
        cam.gridn_width  = gridn_width;
        cam.gridn_height = (int32_t)gh;
        cam.cell0   = (int32_t)Ncells;
        cam.centre0 = (int32_t)plan->centres.size();
        cam.wcell   = (double)(W - 1)/(double)(gridn_width - 1);
        cam.hcell   = (double)(H - 1)/(double)(gh - 1);
        cam.half_w  = cam.wcell/2.;
        cam.half_h  = cam.hcell/2.;
        for(int i = 0; i < gridn_width; i++) plan->centres.push_back(regional_cell_centre(i, gridn_width, W));
        for(int j = 0; j < (int)gh;     j++) plan->centres.push_back(regional_cell_centre(j, (int)gh, H));
        plan->cameras.push_back(cam);
        Ncells += (int64_t)gridn_width*gh;
    }
    plan->Ncells = (int)Ncells;
    if(Nobservations_board < 0 || corners_per_board <= 0) { *err = "no board observations"; return false; }
    plan->Ncorners = Nobservations_board*(int64_t)corners_per_board;
    // (entries and measurement indices are int32)
    if(plan->Ncorners > (int64_t)INT32_MAX/RS_SLOTS)
    {
        *err = "more than " + std::to_string(INT32_MAX/RS_SLOTS) + " corners";
        return false;
    }
    plan->Nentries_max = plan->Ncorners*RS_SLOTS;
    plan->Nchunks      = (int)((plan->Ncorners + RS_CHUNK - 1)/RS_CHUNK);
    plan->hist_ints    = (int64_t)plan->Nchunks*plan->Ncells;
    plan->scan_items_per_thread = (plan->Ncells + RS_SCAN_THREADS - 1)/RS_SCAN_THREADS;
    return true;
}

} // namespace mrcal_amd
