// orb_internal.h — host-side plumbing shared by the translation units of liborb_hip.so
// (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <cmath>
#include <string>

#include "../../include/orb_abi.h"

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

// Sizes of the regions of a staging buffer or a scratch allocation: rounded up to 256 B.
inline size_t orb_align256(size_t x) { return (x + 255) & ~(size_t)255; }

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

// The device a vocabulary handle lives on (orb_voc.hip), for the units that take one (orb_kfdb.hip).
struct orb_vocabulary;
__attribute__((visibility("hidden"))) int orb_internal_vocabulary_device(const orb_vocabulary* v);
