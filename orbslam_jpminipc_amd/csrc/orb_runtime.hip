// orb_runtime.hip — what every translation unit of liborb_hip.so stands on, and no kernel: the
// calling thread's last error (orb_last_error, orb_internal_set_error), the per-thread, per-device
// host contexts of the synchronous host-buffer entry points (OrbHostCtx, orb_internal_thread_ctx) and
// the host side of their completion flag (OrbDoneFlag).  orb_internal.h declares all of it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/orb_abi.h"
#include "orb_internal.h"

// ---- error plumbing ----------------------------------------------------------------------
static thread_local std::string g_last_error = "";

int orb_internal_set_error(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}

extern "C" const char* orb_last_error(void) { return g_last_error.c_str(); }

// ---- per-thread host contexts (orb_internal.h) -------------------------------------------
int OrbHostCtx::reserve(size_t dev_bytes, size_t host_bytes) {
    if (!stream) {
        hipError_t e = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking);
        if (e != hipSuccess) return orb_internal_set_error(ORB_EDEVICE, std::string("hipStreamCreate: ") + hipGetErrorString(e));
    }
    if (dev_bytes > cap) {
        const size_t want = std::max(dev_bytes, cap * 2);
        if (buf) (void)hipFree(buf);
        buf = nullptr;
        cap = 0;
        hipError_t e = hipMalloc(&buf, want);
        if (e != hipSuccess) return orb_internal_set_error(ORB_EDEVICE, std::string("hipMalloc: ") + hipGetErrorString(e));
        cap = want;
    }
    if (host_bytes > pcap) {
        const size_t want = std::max(host_bytes, pcap * 2);
        if (pinned) (void)hipHostFree(pinned);
        pinned = nullptr;
        pcap = 0;
        hipError_t e = hipHostMalloc((void**)&pinned, want, hipHostMallocDefault);
        if (e != hipSuccess) return orb_internal_set_error(ORB_EDEVICE, std::string("hipHostMalloc: ") + hipGetErrorString(e));
        pcap = want;
    }
    return ORB_OK;
}

namespace {
// Contexts are never destroyed (no HIP teardown at exit); a thread's contexts go back to the
// pool when it exits.
struct CtxPool {
    std::mutex mu;
    std::vector<OrbHostCtx*> free[64];
};
CtxPool& ctx_pool() {
    static CtxPool* p = new CtxPool();
    return *p;
}
struct ThreadCtxs {
    OrbHostCtx* c[64] = {};
    ~ThreadCtxs() {
        CtxPool& P = ctx_pool();
        std::lock_guard<std::mutex> lk(P.mu);
        for (int d = 0; d < 64; ++d)
            if (c[d]) P.free[d].push_back(c[d]);
    }
};
thread_local ThreadCtxs t_ctxs;
}  // namespace

OrbHostCtx* orb_internal_thread_ctx(int device) {
    if (device < 0 || device >= 64) return nullptr;
    OrbHostCtx*& c = t_ctxs.c[device];
    if (!c) {
        CtxPool& P = ctx_pool();
        std::lock_guard<std::mutex> lk(P.mu);
        if (!P.free[device].empty()) {
            c = P.free[device].back();
            P.free[device].pop_back();
        } else {
            c = new OrbHostCtx();
            c->device = device;
        }
    }
    return c;
}

// ---- completion flag (orb_internal.h) ----------------------------------------------------
int OrbDoneFlag::arm(void* at) {
    static thread_local int seq = 0;
    seq = seq == 0x7fffffff ? 1 : seq + 1;
    flag_ = (volatile int*)at;
    *flag_ = 0;
    return seq_ = seq;
}

bool OrbDoneFlag::wait() const {
    const auto t0 = std::chrono::steady_clock::now();
    for (int spin = 0;; ++spin) {
        if (__atomic_load_n(flag_, __ATOMIC_ACQUIRE) == seq_) return true;
        if ((spin & 1023) == 1023 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) return false;
    }
}
