// Who owns device memory. HOST code.
//
// Every hipMalloc / hipHostMalloc of the library is made through a DeviceBuffers: the object that needs the memory
// (a problem, a factorization, an uncertainty context) has one as a member, a function that needs temporaries has a
// local one, and whatever is still held when the owner goes is freed then - on every return path. The structs the
// kernels take by value (OpDev, AssemblyPlan, FactorBuffers ...) stay plain structs of pointers: an owner is handed
// the ADDRESS of the field and fills it.
//
// One hipMalloc per buffer: nothing is pooled, carved out of a slab or kept for the next object.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include <vector>
#include "host_state.hpp"

#define HIP_TRY(expr, onfail)                                           \
    do {                                                                \
        hipError_t _e = (expr);                                         \
        if(_e != hipSuccess)                                            \
        {                                                               \
            set_error("%s:%d: %s failed: %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); \
            onfail;                                                     \
        }                                                               \
    } while(0)

namespace mrcal_amd {

class DeviceBuffers
{
    struct Held { void* p; bool pinned; };
    std::vector<Held> held;          // in the order they were allocated
    int device = -1;                 // the device of the first allocation: the frees happen with it current
    inline static std::atomic<long> Nlive{0};

    bool holds(const void* p) const
    {
        for(const Held& h : held) if(h.p == p) return true;
        return false;
    }
    template<class T> bool take(T** p, size_t n, bool pinned)
    {
        if(*p != NULL && holds(*p))
        {
            set_error("internal error: a buffer this owner still holds would be allocated again (release() it first)");
            return false;
        }
        *p = NULL;
        if(n == 0) n = 1;
        if(device < 0) (void)hipGetDevice(&device);
        if(pinned) HIP_TRY(hipHostMalloc((void**)p, n*sizeof(T)), return false);
        else       HIP_TRY(hipMalloc((void**)p, n*sizeof(T)),     return false);
        held.push_back(Held{ (void*)*p, pinned });
        Nlive++;
        return true;
    }
    // frees held[i0..i1) with the owner's device current
    void give_back(size_t i0, size_t i1)
    {
        if(i0 >= i1) return;
        int cur = device;
        (void)hipGetDevice(&cur);
        if(cur != device) (void)hipSetDevice(device);
        for(size_t i = i0; i < i1; i++)
        {
            if(held[i].pinned) (void)hipHostFree(held[i].p);
            else               (void)hipFree(held[i].p);
        }
        Nlive -= (long)(i1 - i0);
        held.erase(held.begin() + i0, held.begin() + i1);
        if(cur != device) (void)hipSetDevice(cur);
    }

public:
    DeviceBuffers() {}
    DeviceBuffers(const DeviceBuffers&) = delete;
    DeviceBuffers& operator=(const DeviceBuffers&) = delete;
    ~DeviceBuffers() { free_all(); }

    // n elements of device memory (n == 0: one element). *p must not be a buffer this owner holds
    template<class T> bool alloc(T** p, size_t n) { return take(p, n, false); }
    // ... all of it zero
    template<class T> bool alloc_zeroed(T** p, size_t n)
    {
        if(!alloc(p, n)) return false;
        HIP_TRY(hipMemset(*p, 0, (n > 0 ? n : 1)*sizeof(T)), return false);
        return true;
    }
    // ... holding the n elements at host (host == NULL: left as allocated)
    template<class T> bool upload(T** p, const T* host, size_t n)
    {
        if(!alloc(p, n)) return false;
        if(n > 0 && host != NULL)
            HIP_TRY(hipMemcpy(*p, host, n*sizeof(T), hipMemcpyHostToDevice), return false);
        return true;
    }
    // ... holding a list of the host's (an empty list: one element that is zero)
    template<class T> bool upload(T** p, const std::vector<T>& v)
    {
        return v.empty() ? alloc_zeroed(p, 1) : upload(p, v.data(), v.size());
    }
    // n elements of pinned host memory
    template<class T> bool alloc_pinned(T** p, size_t n) { return take(p, n, true); }

    // gives one buffer back before the owner goes; *p is NULL afterwards. Whatever may still be using the buffer on
    // the device is the caller's to wait for
    template<class T> void release(T** p)
    {
        for(size_t i = 0; i < held.size(); i++)
            if(held[i].p == (void*)*p) { give_back(i, i + 1); break; }
        *p = NULL;
    }
    void free_all() { give_back(0, held.size()); }

    // buffers held by all the owners of the process at this moment
    static long live() { return Nlive.load(); }
};

// a CSR matrix of the host on the device: rowptr [Nrows + 1], colidx and values [rowptr[Nrows]]
struct CsrDev { int32_t* Jp = NULL; int32_t* Ji = NULL; double* Jx = NULL; };
inline bool upload_csr(DeviceBuffers& mem, CsrDev* J, int Nrows, const int32_t* rowptr, const int32_t* colidx, const double* values)
{
    const size_t nnz = (size_t)rowptr[Nrows];
    return mem.upload(&J->Jp, rowptr, (size_t)Nrows + 1) && mem.upload(&J->Ji, colidx, nnz) && mem.upload(&J->Jx, values, nnz);
}

} // namespace mrcal_amd
