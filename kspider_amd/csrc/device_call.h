// What every consumer of the join's edges does on the host before its first kernel launch (cluster.hip, export.hip, repr.hip,
// cut.hip, sweep.hip, tree.hip, derep.hip): check a HIP call, choose the device, size a grid of chunk-loop workgroups, ask
// whether an allocation fits, and own device memory until the call returns.  Also the growing device buffer and the HIP check
// of the engine and of the multi-device job (engine.hip, multi.hip), and the owner of the HIP events that time the phases of a
// call (Events: query.hip, gather.hip), so that those calls leave by `return`.  Host code only: no kernel, nothing __device__.
#ifndef KSPIDER_DEVICE_CALL_H
#define KSPIDER_DEVICE_CALL_H
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "engine_internal.h"

// a failing HIP call of a function with `int rc` and a `done:` label: the error text, KSP_E_HIP, and out through the label
#define KSP_TRY_HIP(call)                                                                \
    do {                                                                                 \
        hipError_t err__ = (call);                                                       \
        if (err__ != hipSuccess) {                                                       \
            ksp::set_error(std::string(#call) + ": " + hipGetErrorString(err__));        \
            rc = KSP_E_HIP;                                                              \
            goto done;                                                                   \
        }                                                                                \
    } while (0)

// a failing HIP call of a function that returns a KSP_* code: the error text and KSP_E_HIP
#define KSP_HIP(call)                                                                              \
    do {                                                                                           \
        hipError_t err__ = (call);                                                                 \
        if (err__ != hipSuccess) {                                                                 \
            ksp::set_error(std::string(#call) + ": " + hipGetErrorString(err__));                  \
            return KSP_E_HIP;                                                                      \
        }                                                                                          \
    } while (0)

namespace ksp {

// device memory of the current device that grows when more is asked for (what it held is not kept) and is freed by release()
struct Buf {
    void* p = nullptr;
    size_t bytes = 0;
    int ensure(size_t need) {
        if (need <= bytes) return KSP_OK;
        if (p) { (void)hipFree(p); p = nullptr; bytes = 0; }
        size_t want = need + need / 8 + 256;
        KSP_HIP(hipMalloc(&p, want));
        bytes = want;
        return KSP_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
    template <class T> T* as() const { return (T*)p; }
};

// `device` becomes the current device of the calling thread, or KSP_E_HIP with "WHO: no such device"
inline int set_device(const char* who, const int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) { set_error(std::string(who) + ": no such device"); return KSP_E_HIP; }
    if (hipSetDevice(device) != hipSuccess) { set_error(std::string(who) + ": hipSetDevice"); return KSP_E_HIP; }
    return KSP_OK;
}

// the device of the file drivers: $KSPIDER_DEVICE, 0 when unset
inline int device_from_env() {
    const char* dv = std::getenv("KSPIDER_DEVICE");
    return dv ? std::atoi(dv) : 0;
}

// Workgroups of a pass whose workgroups loop over chunks: one per chunk up to the cap, the rest by the chunk loop.
struct WorkgroupCap {
    uint64_t cap = 1;
    unsigned grid_of(const uint64_t n_chunks) const { return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(n_chunks, cap), 0x7FFFFFFFull)); }
};
// The cap on the CURRENT device: 8 workgroups per CU (32 waves of 256-thread workgroups: a full CU), or $env_name when it is
// 1 or more (tests / diagnostics: a small grid, so that every workgroup loops).  The variable is read by every call.
inline int workgroup_cap(const char* env_name, const char* who, WorkgroupCap& g) {
    const char* mw = std::getenv(env_name);
    const long long cap_env = mw ? std::atoll(mw) : 0;
    int device = 0, cus = 0;
    if (hipGetDevice(&device) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) {
        set_error(std::string(who) + ": cannot read the device's CU count");
        return KSP_E_HIP;
    }
    g.cap = cap_env >= 1 ? (uint64_t)cap_env : 8ull * (uint64_t)std::max(cus, 1);
    return KSP_OK;
}

// `bytes` more of device memory on the CURRENT device, or KSP_E_LIMIT with "WHO: needs N bytes of device memory (WHAT), F are
// free"; `what` may be empty.  *free_out (may be NULL): the free bytes, 0 when they could not be read.
inline int device_fits(const char* who, const uint64_t bytes, const char* what, uint64_t* free_out = nullptr) {
    size_t free_b = 0, total_b = 0;
    if (free_out) *free_out = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { set_error(std::string(who) + ": hipMemGetInfo"); return KSP_E_HIP; }
    if (free_out) *free_out = free_b;
    if (bytes > (uint64_t)free_b) {
        set_error(std::string(who) + ": needs " + std::to_string(bytes) + " bytes of device memory" + (*what ? " (" + std::string(what) + ")" : std::string()) + ", " +
                  std::to_string(free_b) + " are free");
        return KSP_E_LIMIT;
    }
    return KSP_OK;
}

// The device memory of one call.  What alloc() hands out is freed by the destructor, or earlier by release(): a pointer that is
// only ever obtained here cannot be forgotten in a free list.
class DeviceArena {
    std::vector<void*> owned_;

public:
    DeviceArena() = default;
    DeviceArena(const DeviceArena&) = delete;
    DeviceArena& operator=(const DeviceArena&) = delete;
    ~DeviceArena() {
        for (void* p : owned_)
            if (p) (void)hipFree(p);
    }
    // *p = `bytes` of device memory of the current device (what hipMalloc gives for 0 bytes: NULL), or KSP_E_HIP and the error
    int alloc_bytes(void** p, const size_t bytes) {
        *p = nullptr;
        owned_.push_back(nullptr);   // (the slot first: nothing is allocated yet should this throw)
        const hipError_t err = hipMalloc(&owned_.back(), bytes);
        if (err != hipSuccess) {
            owned_.pop_back();
            set_error("hipMalloc of " + std::to_string(bytes) + " bytes: " + hipGetErrorString(err));
            return KSP_E_HIP;
        }
        *p = owned_.back();
        return KSP_OK;
    }
    template <class T>
    int alloc(T** p, const size_t count) { return alloc_bytes((void**)p, count * sizeof(T)); }
    // frees p now (hipFree waits for the device, as it does in the destructor); p may be NULL
    hipError_t release(void* p) {
        if (!p) return hipSuccess;
        const auto it = std::find(owned_.begin(), owned_.end(), p);
        if (it != owned_.end()) owned_.erase(it);
        return hipFree(p);
    }
};

// N HIP events of one call: create() makes them, the destructor destroys the ones that were made
template <int N>
struct Events {
    hipEvent_t ev[N] = {};
    Events() = default;
    Events(const Events&) = delete;
    Events& operator=(const Events&) = delete;
    ~Events() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    int create() {
        for (hipEvent_t& e : ev) KSP_HIP(hipEventCreate(&e));
        return KSP_OK;
    }
    hipEvent_t operator[](const int i) const { return ev[i]; }
};

// two host arrays of n node indices as *d_a, *d_b in the arena (the (a, b) form of an edge list)
inline int upload_pairs(DeviceArena& arena, const uint32_t* h_a, const uint32_t* h_b, const uint64_t n, uint32_t** d_a, uint32_t** d_b) {
    int rc = KSP_OK;
    if ((rc = arena.alloc(d_a, (size_t)n)) || (rc = arena.alloc(d_b, (size_t)n))) return rc;
    KSP_HIP(hipMemcpy(*d_a, h_a, (size_t)n * 4, hipMemcpyHostToDevice));
    KSP_HIP(hipMemcpy(*d_b, h_b, (size_t)n * 4, hipMemcpyHostToDevice));
    return KSP_OK;
}

}  // namespace ksp
#endif
