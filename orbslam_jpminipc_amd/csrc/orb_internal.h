// orb_internal.h — host-side plumbing shared by the translation units of liborb_hip.so
// (not part of the C ABI).  What is only declared here (the last error, the per-thread contexts,
// the completion flag) is defined in orb_runtime.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <cmath>
#include <string>

#include "../../include/orb_abi.h"
#include "orb_staging.h"

// Records `msg` as the calling thread's orb_last_error() and returns `code`.
__attribute__((visibility("hidden"))) int orb_internal_set_error(int code, const std::string& msg);

// A HIP call that makes the enclosing function return ORB_EDEVICE, with the call's text and HIP's
// message as the error, when it fails.
#define ORB_HIPCHK(expr)                                                                                    \
    do {                                                                                                    \
        hipError_t e_ = (expr);                                                                             \
        if (e_ != hipSuccess)                                                                               \
            return orb_internal_set_error(ORB_EDEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));  \
    } while (0)

// fx fy cx cy of an entry point `who`: all finite, the focal lengths not 0; ORB_EINVAL (message set)
// otherwise.  `which` names the camera where a call takes more than one ("K1"), "" where it takes one.
inline int orb_check_camera(const char* who, const char* which, const float* K4) {
    static const char* const name[4] = {"fx", "fy", "cx", "cy"};
    for (int k = 0; k < 4; ++k)
        if (!std::isfinite(K4[k]) || (k < 2 && K4[k] == 0.0f))
            return orb_internal_set_error(ORB_EINVAL, std::string(who) + ": " + which + (*which ? " " : "") + name[k] +
                                                          " = " + std::to_string(K4[k]) +
                                                          (k < 2 ? " must be finite and not 0" : " must be finite"));
    return ORB_OK;
}

// Per-thread, per-device state of the synchronous host-buffer entry points (matcher family,
// single-pair SearchForInitialization): a private non-blocking stream, a grow-only device
// arena and a grow-only pinned host staging buffer.  Each calling thread gets its own (the
// reference runs matchers concurrently from Tracking, LocalMapping and LoopClosing,
// main.cc:164-193), so calls from different threads overlap on the device instead of
// serialising; a context is returned to a pool when its thread exits and reused by the next
// thread (no HIP call at thread exit).  Calls only ever synchronise their own stream.
struct OrbHostCtx {
    int device = -1;
    hipStream_t stream = nullptr;
    uint8_t* buf = nullptr;     // device arena
    size_t cap = 0;
    uint8_t* pinned = nullptr;  // host staging (hipHostMalloc)
    size_t pcap = 0;
    // Grow the arena / staging to at least the given sizes (contents not preserved); creates
    // the stream on first use.  ORB_OK or ORB_EDEVICE (message set).
    int reserve(size_t dev_bytes, size_t host_bytes);
};
__attribute__((visibility("hidden"))) OrbHostCtx* orb_internal_thread_ctx(int device);

// The completion flag of a host call whose last kernel publishes it (orb_device.h, publish_done): an
// int in the context's pinned staging that the host spins on instead of synchronising the stream
// (~1 us after the kernel's write, where a synchronisation takes several).  One sequence per thread
// for every user (a thread's calls are one after another, on one staging), never 0, so a flag left
// by an earlier call, at this offset or another, is never taken for this call's.  The caller
// synchronises its stream when wait() gives false (an error, or a kernel past the bound); the staging
// is reused only after the flag or that synchronisation.
class __attribute__((visibility("hidden"))) OrbDoneFlag {
    volatile int* flag_ = nullptr;
    int seq_ = 0;

public:
    // The thread's sequence advanced (wrapping to 1), the flag at `at` cleared; the sequence to give the kernel.
    int arm(void* at);
    // Spins (acquire loads) until the flag holds the sequence: true; false after 2 ms, the clock read
    // every 1024 spins.
    bool wait() const;
};

// One synchronous host-buffer call on the calling thread's context of `device` (< 0: the current one):
// the planned arena reserved (device: all of it; pinned staging: in + out, the scratch is not
// mirrored) and bound, or `err` set (message recorded) and nothing to use.  Then: send() or put() the
// inputs, upload(), launch on stream() with dev() pointers, finish(), get() the outputs.
class OrbHostCall : public OrbStage {
    OrbHostCtx* C = nullptr;
    int open(const OrbStagePlan& plan, int device) {
        int ndev = 0;
        ORB_HIPCHK(hipGetDeviceCount(&ndev));
        if (device < 0) ORB_HIPCHK(hipGetDevice(&device));
        C = device < ndev ? orb_internal_thread_ctx(device) : nullptr;
        if (!C) return orb_internal_set_error(ORB_EINVAL, "device ordinal out of range");
        ORB_HIPCHK(hipSetDevice(device));
        if (int r = C->reserve(plan.total(), plan.out_end())) return r;
        bind(plan, C->buf, C->pinned);
        return ORB_OK;
    }

public:
    const int err;
    OrbHostCall(const OrbStagePlan& plan, int device) : err(open(plan, device)) {}
    hipStream_t stream() const { return C->stream; }
    // the in-span to the device, in one copy
    int upload() const {
        const uint8_t* hp = h_;
        const size_t in_end = in_end_;
        ORB_HIPCHK(hipMemcpyAsync(C->buf, hp, in_end, hipMemcpyHostToDevice, C->stream));
        return ORB_OK;
    }
    // After the launches, which gave `r` (an error of ours, message set) and `e`: the out-span to the
    // host in one copy when both are clean, and the stream synchronised in every case, because the next
    // call on this thread reuses the staging.  `r` wins, then `e` or the copy's error, then the
    // synchronise's; a HIP error is recorded as ORB_EDEVICE with `prefix` before HIP's text.
    int finish(int r, hipError_t e, const std::string& prefix) const {
        if (r == ORB_OK && e == hipSuccess)
            e = hipMemcpyAsync(h_ + in_end_, d_ + in_end_, out_end_ - in_end_, hipMemcpyDeviceToHost, C->stream);
        const hipError_t es = hipStreamSynchronize(C->stream);
        if (r) return r;
        if (e == hipSuccess) e = es;
        if (e != hipSuccess) return orb_internal_set_error(ORB_EDEVICE, prefix + hipGetErrorString(e));
        return ORB_OK;
    }
};

// A stream-ordered scratch block for the regions that `regions(OrbLayout&)` names: `regions` runs
// once without a base, for the size, and once on the allocation, for the pointers.  *block is what to
// hipFreeAsync after the last kernel (NULL when no region was needed); ORB_ENOMEM with `what` before
// HIP's text when the allocation fails.
template <class F>
int orb_scratch_alloc(void** block, hipStream_t st, const std::string& what, F&& regions) {
    *block = nullptr;
    if (const size_t bytes = orb_layout_size(regions)) {
        const hipError_t e = hipMallocAsync(block, bytes, st);
        if (e != hipSuccess) return orb_internal_set_error(ORB_ENOMEM, what + hipGetErrorString(e));
    }
    OrbLayout L(*block);
    regions(L);
    return ORB_OK;
}

// The device a vocabulary handle lives on (orb_voc.hip), for the units that take one (orb_kfdb.hip).
struct orb_vocabulary;
__attribute__((visibility("hidden"))) int orb_internal_vocabulary_device(const orb_vocabulary* v);
