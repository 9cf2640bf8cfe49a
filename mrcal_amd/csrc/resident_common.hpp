// What the resident objects of the feature paths (rectification ... lens-model fit) share on the HOST: the test for a
// device, and the HIP events that time the stages of a run. No kernel is in here, and no stream or pool: the device
// memory is DeviceBuffers' (device_memory.hpp). The solver's own events (problem.cpp, solver.cpp) are part of the
// step's fork and join, and are not these.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/mrcal_amd.h"
#include "host_state.hpp"
#include "device_memory.hpp"

namespace mrcal_amd {

inline bool have_device()
{
    if(mrcal_amd_device_count() > 0) return true;
    set_error("no HIP device is visible: libmrcal_amd has no CPU fallback");
    return false;
}

// N events around the N-1 stages of a run: event i is recorded where stage i begins, event i+1 where it ends. The
// functions that queue the stages take a StageEvents*, and NULL means "do not record"
template<int N>
struct StageEvents
{
    hipEvent_t event[N] = {};
    bool       timed    = false;       // a whole run has been recorded: elapsed() has something to report

    StageEvents() {}
    StageEvents(const StageEvents&)            = delete;
    StageEvents& operator=(const StageEvents&) = delete;
    ~StageEvents() { for(hipEvent_t e : event) if(e != NULL) (void)hipEventDestroy(e); }

    // makes the events that are not there yet; false: the error is set. An object that times every run calls it
    // when it is created, one that times on request only when it is asked to
    bool create()
    {
        for(hipEvent_t& e : event)
            if(e == NULL) HIP_TRY(hipEventCreate(&e), return false);
        return true;
    }
    bool record(int i, hipStream_t stream = NULL)
    {
        HIP_TRY(hipEventRecord(event[i], stream), return false);
        return true;
    }
    // the milliseconds between two recorded events, both complete
    bool elapsed(float* milliseconds, int from, int to) const
    {
        HIP_TRY(hipEventElapsedTime(milliseconds, event[from], event[to]), return false);
        return true;
    }
};

template<int N>
inline bool record(StageEvents<N>* events, int i, hipStream_t stream = NULL)
{
    return events == NULL || events->record(i, stream);
}

} // namespace mrcal_amd
