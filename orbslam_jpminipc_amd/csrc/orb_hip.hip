// orb_hip.hip — MI355X (gfx950) ORB front end: kernels + the C ABI of include/orb_abi.h.
//
// Pipeline for a batch of B same-size frames (all device-resident, one HIP stream):
//   k_pyr0        level 0 + reflect-101 padding          (ORBextractor.cc:814-815)
//   k_pyr_resize  level l from level l-1, fused padding   (ORBextractor.cc:800-807), l = 1..L-1
//                 (k_pyr_resize_tail: the small levels of a large batch in one launch)
//   k_fast        per level tile: FAST strength at fastTh and the per-cell 3x3 NMS; survivors
//                 appended to their cell's slots          (ORBextractor.cc:560-607)
//   k_rerun       FAST(7) re-run of cells with <= 3 survivors (609-614), spread over several
//                 workgroups per (frame, level)
//   k_select      per (frame, level): raster order per cell, quota redistribution, retainBest
//                 per cell and per level — exact libstdc++ nth_element replay (622-701)
//   k_orient_desc per keypoint (one wave): IC angle on the raw level, rBRIEF on the
//                 7x7 sigma-2 blur evaluated at the sample points, keypoint record
//                                                          (ORBextractor.cc:124-194, 705-777)
// k_fast and k_pyr_stream (the whole pyramid of a frame in one pass, large batches) live in
// orb_ilp.hip, which is compiled under its own scheduler flags, and are launched through its
// orb_ilp_* functions; orb_extract.h holds what the two units share.  SearchForInitialization
// (k_match_init) is orb_sfi.hip.
//
// Reference behaviour that lives in OpenCV 2.4 / libstdc++ / glibc is restated per
// SURVEY.md Appendix A; DESIGN.md lists every arithmetic rule and where it is pinned.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/orb_abi.h"
#include "../../include/orb_debug.h"
#include "nth_select.h"
#include "orb_internal.h"
#include "orb_device.h"
#include "orb_extract.h"
#include "pattern31.inc"

#ifndef KR_TIMING  // 1: per-level, per-phase s_memrealtime sums of k_rerun's cell re-runs (experiments)
#define KR_TIMING 0
#endif
#if KR_TIMING
__device__ unsigned long long g_krtime[ORB_MAX_LEVELS][8];
#define KR_T(i) const unsigned long long krt##i = __builtin_amdgcn_s_memrealtime()
#else
#define KR_T(i)
#endif
#ifndef KS_TIMING  // 1: per-level, per-phase s_memrealtime sums of k_select's workgroups (experiments)
#define KS_TIMING 0
#endif
#if KS_TIMING
__device__ unsigned long long g_kstime[ORB_MAX_LEVELS][8];
#define KS_T(i) const unsigned long long kst##i = __builtin_amdgcn_s_memrealtime()
#else
#define KS_T(i)
#endif
// Only switches that keep the output exact (sizes, register targets, timing probes) exist in
// this translation unit; ablations that change the output are not part of the product source.

// ======================================================================================
// error plumbing
// ======================================================================================
static thread_local std::string g_last_error = "";

int orb_internal_set_error(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}

// ======================================================================================
// kernels
// ======================================================================================
using namespace orbdev;

// bit_pattern_31_ (ORBextractor.cc:197-455) as floats, pair-major: c_patternf[2 (64 q + l) + {0, 1}]
// = (x, y) of point 8 l + q, i.e. lane l's eight points are one float2 in each of eight 512-B
// rows (k_orient_desc loads each row with one fully coalesced global_load_dwordx2, §6.1)
__constant__ float c_patternf[1024];
// IC_Angle (ORBextractor.cc:124-151 with umax, 495-510) over the 31 x 9 patch dwords n = 9 r + c
// (five 64-lane steps, n < 320; n >= 279 carry zero coefficients): c_icoff[n] = the dword's byte
// offset in k_orient_desc's window from the patch's first dword; per byte alignment sh of the
// patch in its dword row, c_ic10 / c_ic01[320 sh + n] = the signed byte coefficients u = 4c + i -
// sh - 15 / v = r - 15 of byte i where it lies inside the disc (|u| <= umax[|v|]), else 0
__constant__ uint32_t c_icoff[320];
__constant__ uint32_t c_ic10[4 * 320];
__constant__ uint32_t c_ic01[4 * 320];
// k_orient_desc's row-pass B fragments: [N-tile t][lane l] = bytes j of B[16(l >> 4) + j][16t + (l & 15)]
__constant__ uint4 c_rowB[4 * 64];  // 279 patch dwords per alignment, zero-padded to 5 x 64
// ---- pyramid --------------------------------------------------------------------------
// Level 0: copyMakeBorder(image, 16, BORDER_REFLECT_101); one thread per 16-byte chunk of a
// padded row (pitch is a multiple of 16).  Interior chunks (source columns [x-16, x) inside the
// row) are one 16-, four 4- or sixteen 1-byte loads depending on the source alignment and one
// 16-byte store; the two border chunks per side reflect byte by byte.
__global__ void __launch_bounds__(256) k_pyr0(const uint8_t* __restrict__ imgs, int stride, long long fpitch,
                                              uint8_t* __restrict__ pyr, Geom g) {
    const LevelGeom& lg = g.lv[0];
    const int nchunk = lg.pitch >> 4;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int py = i / nchunk, x16 = (i - py * nchunk) << 4;
    if (py >= lg.ph) return;
    const int b = blockIdx.y;
    const uint8_t* src = imgs + (long long)b * fpitch + (long long)reflect101(py - EDGE, lg.h) * stride;
    uint4 out;
    if (x16 >= EDGE && x16 <= lg.w) {
        const uint8_t* p = src + (x16 - EDGE);
        const uintptr_t a = (uintptr_t)p;
        if ((a & 15u) == 0) {
            out = *(const uint4*)p;
        } else if ((a & 3u) == 0) {
            const uint32_t* q = (const uint32_t*)p;
            out = make_uint4(q[0], q[1], q[2], q[3]);
        } else {
            uint32_t w[4];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                w[k] = (uint32_t)p[4 * k] | ((uint32_t)p[4 * k + 1] << 8) | ((uint32_t)p[4 * k + 2] << 16) |
                       ((uint32_t)p[4 * k + 3] << 24);
            out = make_uint4(w[0], w[1], w[2], w[3]);
        }
    } else {
        uint32_t w[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            uint32_t word = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int px = x16 + 4 * k + j;
                uint32_t v = 0;
                if (px < lg.w + 2 * EDGE) v = src[reflect101(px - EDGE, lg.w)];
                word |= v << (8 * j);
            }
            w[k] = word;
        }
        out = make_uint4(w[0], w[1], w[2], w[3]);
    }
    *(uint4*)(pyr + lg.base + (long long)b * lg.fstride + (long long)py * lg.pitch + x16) = out;
}

// Level 0 from 3- or 4-channel frames: Tracking::GrabImage's cvtColor(.., CV_RGB2GRAY /
// CV_BGR2GRAY) (Tracking.cc:202-207) fused with the padding.  OpenCV 2.4's RGB2Gray<uchar> is an
// exact fixed-point sum, (c0*p[0] + 9617*p[1] + c2*p[2] + 2^13) >> 14 with R2Y = 4899,
// G2Y = 9617, B2Y = 1868 (yuv_shift 14): (c0, c2) = (R2Y, B2Y) for RGB order, (B2Y, R2Y) for BGR.
__global__ void __launch_bounds__(256) k_pyr0_color(const uint8_t* __restrict__ imgs, int stride, long long fpitch,
                                                    int cn, int c0, int c2, uint8_t* __restrict__ pyr, Geom g) {
    const LevelGeom& lg = g.lv[0];
    const int b = blockIdx.z, py = blockIdx.y * 4 + threadIdx.y;
    const int x4 = (blockIdx.x * 64 + threadIdx.x) * 4;
    if (x4 >= lg.pitch || py >= lg.ph) return;
    const uint8_t* src = imgs + (long long)b * fpitch + (long long)reflect101(py - EDGE, lg.h) * stride;
    uint32_t word = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int px = x4 + i;
        uint32_t v = 0;
        if (px < lg.w + 2 * EDGE) {
            const uint8_t* p = src + (long long)reflect101(px - EDGE, lg.w) * cn;
            v = (uint32_t)((c0 * p[0] + 9617 * p[1] + c2 * p[2] + (1 << 13)) >> 14);
        }
        word |= v << (8 * i);
    }
    *(uint32_t*)(pyr + lg.base + (long long)b * lg.fstride + (long long)py * lg.pitch + x4) = word;
}

// Stage `rows` x `units` 16-byte units (global row pitch gsu units, LDS row pitch the same
// `units`) with 256 threads, up to RZ_SB units per thread all in flight before any LDS write:
// a k_pyr_resize source tile is one memory round trip.
#define RZ_SB 8
__device__ __forceinline__ void stage_tile16(uint4* __restrict__ dst, const uint4* __restrict__ src, long long gsu,
                                             int rows, int units, int tid) {
    const int total = rows * units;
    const int dr = 256 / units, dc = 256 - dr * units;
    for (int base = 0; base < total; base += RZ_SB * 256) {
        const int i0 = base + tid;
        const int r0 = i0 / units, c0 = i0 - r0 * units;
        // every slot is loaded (past-the-end slots re-read unit 0): a conditionally assigned
        // uint4 array was placed in scratch, one private-memory round trip per tile
        uint4 v[RZ_SB];
        int r = r0, c = c0;
#pragma unroll
        for (int k = 0; k < RZ_SB; ++k) {
            const bool ok = i0 + k * 256 < total;
            v[k] = src[ok ? (long long)r * gsu + c : 0ll];
            r += dr;
            c += dc;
            if (c >= units) {
                c -= units;
                ++r;
            }
        }
#pragma unroll
        for (int k = 0; k < RZ_SB; ++k)
            if (i0 + k * 256 < total) dst[i0 + k * 256] = v[k];
    }
}


// Level l >= 1: cv::resize(level l-1, (w_l, h_l), INTER_LINEAR) for 8U:
// fixed-point HResizeLinear rows; vertical SSE2 body (VResizeLinearVec_32s8u) for x < xs,
// scalar FixedPtCast<int,uchar,22> tail; then copyMakeBorder(REFLECT_101 | ISOLATED), fused
// by evaluating the resize at the reflected coordinate of every padded pixel.
// One workgroup per RZ_TW x RZ_TH tile of the padded level: the source rectangle the tile
// reads (host table: first 16-byte column, 16-byte units, first row, rows) is staged into LDS
// in one round trip of 16-byte loads; a thread owns 4 padded columns (taps in registers) and walks the
// RZ_TH / 4 rows of its wave.  As in OpenCV, a source row's horizontal sums are computed once
// and kept (two rows in registers) while consecutive output rows reuse them.
// Every coefficient is in [0, 2050] with a0 + a1, b0 + b1 <= 2050 (checked on the host), so
// no intermediate of the reference's saturating chain can saturate: H <= 255 * 2050 = 522750,
// (H >> 4) * b < 2^27, the SSE2 sum <= 1023 and the scalar sum < 2^31; both end in [0, 255].
// The SSE2 path's (h * b) >> 16 is then mulhi(h, b << 16).
#define RZ_TW 256  // 64 lanes x 4 columns
#ifndef RZ_TH
#define RZ_TH 32
#endif
#ifndef RZ_THS
#define RZ_THS 4  // tile rows for batches below KR_SHORT_BATCH (B=1 640x480: 0.074 -> 0.035 ms for levels 1-7)
#endif
#ifndef KR_SHORT_BATCH
#define KR_SHORT_BATCH 8
#endif
// The two levels arrive by value: a Geom indexed by the runtime level was copied to scratch
// (144 B per lane of private-memory traffic per thread).
template <int TH>
__global__ void __launch_bounds__(256) k_pyr_resize(uint8_t* __restrict__ pyr, const int* __restrict__ rtab,
                                                    const LevelGeom lg, const LevelGeom ls) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_src[];
    const int b = blockIdx.z, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int* tt = rtab + (TH == RZ_TH ? lg.rtile : lg.rtileS) + 4 * (blockIdx.y * gridDim.x + blockIdx.x);
    const int colStart = tt[0], words = tt[1], rowMin = tt[2], nrows = tt[3];
    const uint8_t* S = pyr + ls.base + (long long)b * ls.fstride + (long long)EDGE * ls.pitch + EDGE;
    stage_tile16((uint4*)s_src, (const uint4*)(S + (long long)rowMin * ls.pitch + colStart), ls.pitch >> 4, nrows,
                 words, tid);
    const int* xofs = rtab + lg.rtab;
    const int* alpha = xofs + lg.w;
    const int* yofs = alpha + lg.w;
    const int* beta = yofs + lg.h;
    // the wave's TH / 4 row coefficients, one row per lane, fetched while the tile loads
    // (read back with readlane: no dependent global load inside the row walk)
    const int pyA = blockIdx.y * TH + wave * (TH / 4);
    const int pyB = min(pyA + TH / 4, lg.ph);
    int rowSy = 0, rowBeta = 0;
    if (lane < TH / 4 && pyA + lane < pyB) {
        const int ly = reflect101(pyA + lane - EDGE, lg.h);
        rowSy = yofs[ly];
        rowBeta = beta[ly];
    }
    const int x4 = blockIdx.x * RZ_TW + 4 * lane;
    uint32_t o0[4], o1[4], a0[4], a1[4];
    uint32_t liveMask = 0;
    bool allSimd = true;
    uint32_t simdBytes = 0;  // 0xFF in the byte of every SSE2 column
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int px = x4 + i;
        if (px < lg.w + 2 * EDGE) liveMask |= 0xFFu << (8 * i);
        const int lx = reflect101(min(px, lg.w + 2 * EDGE - 1) - EDGE, lg.w);
        const int sx = xofs[lx];
        if (lx < lg.xmax) {
            const int aa = alpha[lx];
            a0[i] = (uint32_t)(aa & 0xFFFF);
            a1[i] = (uint32_t)(aa >> 16) & 0xFFFFu;
        } else {  // HResizeLinear tail: S[sx] * ONE (sx + 1 may be past the row: not read)
            a0[i] = 2048;
            a1[i] = 0;
        }
        o0[i] = (uint32_t)(sx - colStart);
        o1[i] = (uint32_t)((a1[i] ? sx + 1 : sx) - colStart);
        allSimd = allSimd && lx < lg.xs_resize;
        if (lx < lg.xs_resize) simdBytes |= 0xFFu << (8 * i);
    }
    __syncthreads();
    if (x4 >= lg.pitch) return;
    // a wave holding a scalar-tail column computes both formulas for all its lanes and selects per
    // byte (wave-uniform: no divergent path per row); the other waves the SSE2 one alone
    const bool waveTail = __ballot(!allSimd) != 0ull;
    const bool shift4 = allSimd && !waveTail;
    const uint8_t* L = (const uint8_t*)s_src;
    const int LP = words * 16;
    // horizontal sums of source row r: H >> 4 on the SSE2 columns, H on the scalar tail
    auto hrow = [&](int r, uint32_t* h) {
        const uint8_t* R = L + (r - rowMin) * LP;
#pragma unroll
        for (int i = 0; i < 4; ++i) h[i] = (uint32_t)R[o0[i]] * a0[i] + (uint32_t)R[o1[i]] * a1[i];
        if (shift4) {
#pragma unroll
            for (int i = 0; i < 4; ++i) h[i] >>= 4;
        }
    };
    uint8_t* D = pyr + lg.base + (long long)b * lg.fstride + x4;
    // one output row from the horizontal sums hA (source row s0) and hB (s1)
    auto vrow = [&](const int py, const uint32_t bb, const uint32_t* hA, const uint32_t* hB) {
        const uint32_t b0 = bb & 0xFFFFu, b1 = bb >> 16;
        uint32_t word;
        if (!waveTail) {
            const uint32_t B0 = b0 << 16, B1 = b1 << 16;
            uint32_t r[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) r[i] = (__umulhi(hA[i], B0) + __umulhi(hB[i], B1) + 2u) >> 2;
            word = r[0] | (r[1] << 8) | (r[2] << 16) | (r[3] << 24);
        } else {  // hA / hB are full sums in this wave
            uint32_t ws = 0, wc = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                ws |= ((__umulhi(hA[i] >> 4, b0 << 16) + __umulhi(hB[i] >> 4, b1 << 16) + 2u) >> 2) << (8 * i);
                wc |= ((hA[i] * b0 + hB[i] * b1 + (1u << 21)) >> 22) << (8 * i);
            }
            word = bfi(simdBytes, ws, wc);
        }
        *(uint32_t*)(D + (long long)py * lg.pitch) = word & liveMask;
    };
    // rows in pairs with the source register sets in alternating roles (k_pyr_stream's
    // build_quad): a downscale row's second source row is the next row's first, already in the
    // set that row reads first, so no sums are copied between sets (tP / tQ: rows held)
    int tP = -1, tQ = -1;
    uint32_t hP[4] = {0, 0, 0, 0}, hQ[4] = {0, 0, 0, 0};
    auto src_rows = [&](const int py, int& s0, int& s1, uint32_t& bb) {
        const int sy = __builtin_amdgcn_readlane(rowSy, py - pyA);
        bb = (uint32_t)__builtin_amdgcn_readlane(rowBeta, py - pyA);
        s0 = min(max(sy, 0), ls.h - 1);
        s1 = min(max(sy + 1, 0), ls.h - 1);
    };
    for (int py = pyA; py < pyB; py += 2) {
        {
            int s0, s1;
            uint32_t bb;
            src_rows(py, s0, s1, bb);
            if (tP != s0) hrow(s0, hP), tP = s0;
            if (tQ != s1) hrow(s1, hQ), tQ = s1;
            vrow(py, bb, hP, hQ);
        }
        if (py + 1 < pyB) {
            int s0, s1;
            uint32_t bb;
            src_rows(py + 1, s0, s1, bb);
            if (tQ != s0) hrow(s0, hQ), tQ = s0;
            if (tP != s1) hrow(s1, hP), tP = s1;
            vrow(py + 1, bb, hQ, hP);
        }
    }
}

// Levels lf .. L-1 of one frame per 1024-thread workgroup (the small levels: one launch
// instead of one per level, each of which was latency-bound at a few thousand pixels per
// frame).  Level lf reads level lf-1 from HBM; every later level reads its source ROI from
// LDS, where the previous level left it (ping-pong buffers A / B); the level's resize tables
// are staged in LDS too.  Per padded pixel the arithmetic is k_pyr_resize's: HResizeLinear
// taps (tail columns S[sx] * 2048), then the SSE2 vertical body (((H >> 4) * b) >> 16 summed,
// + 2 >> 2) on columns lx < xs, the scalar FixedPtCast (+ 2^21 >> 22) on the others.
#define RT_THREADS 1024
#define RT_LDS_MAX (150 * 1024)
__global__ void __launch_bounds__(RT_THREADS) k_pyr_resize_tail(uint8_t* __restrict__ pyr,
                                                                const int* __restrict__ rtab, Geom g, int lf,
                                                                int bufA, int bufB) {
    extern __shared__ __attribute__((aligned(16))) uint8_t s_rt[];
    const int b = blockIdx.x, tid = threadIdx.x;
    int* tab = (int*)(s_rt + bufA + bufB);
    for (int l = lf; l < g.L; ++l) {
        const LevelGeom lg = g.lv[l], ls = g.lv[l - 1];
        const int w = lg.w, h = lg.h, sw = ls.w, sh = ls.h;
        const int* src = rtab + lg.rtab;
        for (int i = tid; i < 2 * (w + h); i += RT_THREADS) tab[i] = src[i];
        __syncthreads();
        const int *xofs = tab, *alpha = tab + w, *yofs = tab + 2 * w, *beta = yofs + h;
        const uint8_t* Sg = pyr + ls.base + (long long)b * ls.fstride + (long long)EDGE * ls.pitch + EDGE;
        // level l-lf even -> buffer A at 0, odd -> buffer B at bufA (bufB: B's size)
        const uint8_t* Sl = s_rt + (((l - 1 - lf) & 1) ? bufA : 0);  // level l-1's ROI (l > lf)
        uint8_t* Dl = (l + 1 < g.L) ? s_rt + (((l - lf) & 1) ? bufA : 0) : nullptr;
        const long long spitch = l > lf ? sw : ls.pitch;
        const uint8_t* S = l > lf ? Sl : Sg;
        uint8_t* D = pyr + lg.base + (long long)b * lg.fstride;
        const int nw = lg.pitch >> 2, rowsPerPass = RT_THREADS / nw;
        const int r0 = tid / nw, c4 = (tid - r0 * nw) * 4;
        if (r0 < rowsPerPass) {
            int sx[4], sx1[4];
            uint32_t a0[4], a1[4];
            bool simd[4], live[4], roiX[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int px = c4 + j;
                live[j] = px < w + 2 * EDGE;
                roiX[j] = px >= EDGE && px < EDGE + w;
                const int lx = reflect101(min(px, w + 2 * EDGE - 1) - EDGE, w);
                sx[j] = xofs[lx];
                if (lx < lg.xmax) {
                    const int aa = alpha[lx];
                    a0[j] = (uint32_t)(aa & 0xFFFF);
                    a1[j] = (uint32_t)(aa >> 16) & 0xFFFFu;
                } else {
                    a0[j] = 2048;
                    a1[j] = 0;
                }
                sx1[j] = a1[j] ? sx[j] + 1 : sx[j];
                simd[j] = lx < lg.xs_resize;
            }
            // four rows per step, all their source bytes loaded before any is used: the first
            // fused level reads HBM / L2, and a thread's rows would otherwise be one exposed
            // round trip each
            for (int py0 = r0; py0 < lg.ph; py0 += 4 * rowsPerPass) {
                uint32_t v[4][4][4];
                uint32_t bk[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int py = min(py0 + k * rowsPerPass, lg.ph - 1);
                    const int ly = reflect101(py - EDGE, h);
                    const int sy = yofs[ly];
                    bk[k] = (uint32_t)beta[ly];
                    const uint8_t* R0 = S + min(max(sy, 0), sh - 1) * spitch;
                    const uint8_t* R1 = S + min(max(sy + 1, 0), sh - 1) * spitch;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        v[k][j][0] = R0[sx[j]];
                        v[k][j][1] = R0[sx1[j]];
                        v[k][j][2] = R1[sx[j]];
                        v[k][j][3] = R1[sx1[j]];
                    }
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int py = py0 + k * rowsPerPass;
                    if (py >= lg.ph) break;
                    const uint32_t b0 = bk[k] & 0xFFFFu, b1 = bk[k] >> 16;
                    const bool roiY = Dl && py >= EDGE && py < EDGE + h;
                    uint32_t word = 0;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const uint32_t hA = v[k][j][0] * a0[j] + v[k][j][1] * a1[j];
                        const uint32_t hB = v[k][j][2] * a0[j] + v[k][j][3] * a1[j];
                        const uint32_t r = simd[j]
                                               ? (__umulhi(hA >> 4, b0 << 16) + __umulhi(hB >> 4, b1 << 16) + 2u) >> 2
                                               : (hA * b0 + hB * b1 + (1u << 21)) >> 22;
                        if (live[j]) word |= r << (8 * j);
                        if (roiY && roiX[j]) Dl[(py - EDGE) * w + (c4 + j - EDGE)] = (uint8_t)r;
                    }
                    *(uint32_t*)(D + (long long)py * lg.pitch + c4) = word;
                }
            }
        }
        __syncthreads();  // level l complete in LDS; the tables are free
    }
}

// k_pyr_stream (orb_ilp.hip): when the host uses it, and the LDS its plan aims for
#ifndef KR_STREAM_BATCH  // smallest batch that uses k_pyr_stream (one workgroup per frame)
#define KR_STREAM_BATCH 256
#endif
#ifndef PS_LDS_TARGET
#define PS_LDS_TARGET (76 * 1024)  // two workgroups per CU
#endif

// cv::FAST's full pre-test (all eight even circle points): a 9-arc holds a point of every
// antipodal pair {k, k+8}, so bright <=> min over the four pairs of their max > v + t and dark
// <=> max over the pairs of their min < v - t are necessary.  Stronger than compass_half (two
// pairs), for the FAST(7) re-runs whose low threshold lets most noisy pixels through the compass.
__device__ __forceinline__ uint32_t compass8_half(uint32_t v, uint32_t q0, uint32_t q8, uint32_t q4, uint32_t q12,
                                                  uint32_t q2, uint32_t q10, uint32_t q6, uint32_t q14, uint32_t tt) {
    const u16x2 a0 = __builtin_bit_cast(u16x2, q0), a8 = __builtin_bit_cast(u16x2, q8);
    const u16x2 a4 = __builtin_bit_cast(u16x2, q4), a12 = __builtin_bit_cast(u16x2, q12);
    const u16x2 a2 = __builtin_bit_cast(u16x2, q2), a10 = __builtin_bit_cast(u16x2, q10);
    const u16x2 a6 = __builtin_bit_cast(u16x2, q6), a14 = __builtin_bit_cast(u16x2, q14);
    const i16x2 M = __builtin_bit_cast(
        i16x2, __builtin_elementwise_min(
                   __builtin_elementwise_min(__builtin_elementwise_max(a0, a8), __builtin_elementwise_max(a4, a12)),
                   __builtin_elementwise_min(__builtin_elementwise_max(a2, a10), __builtin_elementwise_max(a6, a14))));
    const i16x2 m = __builtin_bit_cast(
        i16x2, __builtin_elementwise_max(
                   __builtin_elementwise_max(__builtin_elementwise_min(a0, a8), __builtin_elementwise_min(a4, a12)),
                   __builtin_elementwise_max(__builtin_elementwise_min(a2, a10), __builtin_elementwise_min(a6, a14))));
    const i16x2 vv = __builtin_bit_cast(i16x2, v);
    const i16x2 X = __builtin_elementwise_max((i16x2)(M - vv), (i16x2)(vv - m));
    return __builtin_bit_cast(uint32_t, (i16x2)(__builtin_bit_cast(i16x2, tt) - X));
}
// the eight-point pre-test of one dword from its centre row (dwords -1, 0, +1: lf, cc, rg), the rows
// 3 below / above (dn, up) and the rows 2 below / above (dwords -1, 0, +1: d2*, u2*)
__device__ __forceinline__ uint32_t compass8(uint32_t lf, uint32_t cc, uint32_t rg, uint32_t dn, uint32_t up,
                                             uint32_t d2l, uint32_t d2c, uint32_t d2r, uint32_t u2l, uint32_t u2c,
                                             uint32_t u2r, uint32_t tt) {
    const uint32_t q4 = __builtin_amdgcn_alignbyte(rg, cc, 3), q12 = __builtin_amdgcn_alignbyte(cc, lf, 1);
    // circle points 2 = (+2, +2), 14 = (+2, -2) on the row 2 below; 6 = (-2, +2), 10 = (-2, -2) 2 above
    const uint32_t q2 = __builtin_amdgcn_alignbyte(d2r, d2c, 2), q14 = __builtin_amdgcn_alignbyte(d2c, d2l, 2);
    const uint32_t q6 = __builtin_amdgcn_alignbyte(u2r, u2c, 2), q10 = __builtin_amdgcn_alignbyte(u2c, u2l, 2);
    return compass_mask(compass8_half(even_bytes(cc), even_bytes(dn), even_bytes(up), even_bytes(q4), even_bytes(q12),
                                      even_bytes(q2), even_bytes(q10), even_bytes(q6), even_bytes(q14), tt),
                        compass8_half(odd_bytes(cc), odd_bytes(dn), odd_bytes(up), odd_bytes(q4), odd_bytes(q12),
                                      odd_bytes(q2), odd_bytes(q10), odd_bytes(q6), odd_bytes(q14), tt));
}

// The reference's `FAST(cellImage, keys, 7, true)` re-run of a cell that kept <= 3 corners at
// fastTh (ORBextractor.cc:609-614), by a whole 256-thread workgroup: the cell ROI with its
// 3 px ring is staged into LDS with 16-byte loads, the strength plane at t = 7 computed, 3x3
// strict NMS inside the detection region (out-of-region neighbours 0, as cv::FAST on the cell
// Mat), survivors written in raster order as ((S - 1) << 24) | (y << 12) | x.  Returns the
// survivor count (all threads).  smem: Sp (dwp x dh, 16-B padded) | Bm (dh x bw survivor mask
// words) | rowc | In (the ROI staged from its 16-B aligned start with 16-B loads: the dword
// staging before needed 128 VGPRs for its 20 loads in flight per thread, 4 waves per SIMD; 16-B
// units need 50: re-runs 0.174 -> 0.123 ms per 512 KITTI frames, 2.61 -> 2.02 per 4096 720p),
// rerun_lds() bytes.  Output: each survivor sets its bit in its row's mask
// and counts into its row; after the row prefix one thread per mask word writes that word's
// survivors at the row's offset + the set bits of the row's earlier words (no per-row scan of
// the cell, no list, no returning atomics in the NMS).
#define RR_Q 320  // per-wave queue of compass survivors (< 64 carried + 4 x 64 new), + a trash slot
inline size_t rerun_lds(int dw, int dh) {
    const size_t dwp = (size_t)((dw + 3) & ~3);
    const size_t inW = (size_t)((15 + dw + 6 + 15) & ~15), spBytes = (dwp * dh + 15) & ~(size_t)15;
    const size_t bmBytes = 4 * (size_t)((dh * ((dw + 31) >> 5) + 3) & ~3);
    return spBytes + bmBytes + 4 * (size_t)((dh + 3) & ~3) + inW * (dh + 6) + 16 + 4 * (4 + 4 * (RR_Q + 8));
}
// Stage `rows` x `units` 16-B units (global row pitch gsu units) into LDS (row pitch = units):
// SB4 units per thread per batch, all loads of a batch in flight before any LDS write
template <int NT, int SB4>
__device__ __forceinline__ void stage_units_to_lds(uint4* __restrict__ dst, const uint4* __restrict__ src, long long gsu,
                                                   int rows, int units, int tid) {
    const int total = rows * units;
    const int dr = NT / units, dc = NT - dr * units;
    for (int base = 0; base < total; base += SB4 * NT) {
        const int i0 = base + tid;
        const int r0 = i0 / units, c0 = i0 - r0 * units;
        uint4 v[SB4];
        int r = r0, c = c0;
#pragma unroll
        for (int k = 0; k < SB4; ++k) {
            const bool ok = base + k * NT + tid < total;
            v[k] = src[ok ? (long long)r * gsu + c : 0ll];
            r += dr;
            c += dc;
            if (c >= units) {
                c -= units;
                ++r;
            }
        }
#pragma unroll
        for (int k = 0; k < SB4; ++k)
            if (base + k * NT + tid < total) dst[base + k * NT + tid] = v[k];
    }
}
__device__ int cell_fast_rerun(const uint8_t* __restrict__ det, int pitch, int dw, int dh, int rx0, int ry0, int t,
                               uint8_t* smem, uint32_t* __restrict__ out, int tid, int level) {
    const int wave = tid >> 6, lane = tid & 63;
    KR_T(0);
    const int dwp = (dw + 3) & ~3, rw = dwp >> 2, nw = (dh * dwp) >> 2;
    uint8_t* Sp = smem;
    const int spWords = ((dh * dwp + 15) & ~15) >> 2;  // In stays 16-B aligned
    uint32_t* Bm = (uint32_t*)Sp + spWords;  // survivor bits, bw words per row
    const int bw = (dw + 31) >> 5;
    const int bmWords = (dh * bw + 3) & ~3;
    int* rowc = (int*)(Bm + bmWords);
    uint8_t* In = (uint8_t*)(rowc + ((dh + 3) & ~3));
    const int o = (int)((uintptr_t)(det - 3) & 15);  // 16-B alignment of the staged ROI
    const int inW = (o + dw + 6 + 15) & ~15;
    {
        // 16-B units from the aligned start (the pitch is a multiple of 16; the over-read stays
        // in the row's padding or the next row, and its bytes are never used)
        const uint4* src = (const uint4*)(det - 3 * (long long)pitch - 3 - o);
        stage_units_to_lds<256, 4>((uint4*)In, src, pitch >> 4, dh + 6, inW >> 4, tid);
        // Sp and Bm's area (contiguous from the 16-B aligned smem) zeroed with 16-B stores: a
        // pixel the compass rejects keeps strength 0
        const int nz = spWords + bmWords;
        const int z16 = nz >> 2;
        for (int i = tid; i < z16; i += 256) ((uint4*)Sp)[i] = make_uint4(0u, 0u, 0u, 0u);
        for (int i = 4 * z16 + tid; i < nz; i += 256) ((uint32_t*)Sp)[i] = 0u;
        for (int i = tid; i < dh; i += 256) rowc[i] = 0;
    }
    __syncthreads();
    KR_T(1);
    // the strength plane (corner at t <=> S > t; the NMS below reads only S > t, so a pixel
    // known not to be a corner may hold 0): per wave, 64 staged dwords (4 pixels each) at a
    // time through the compass test of cv::FAST at t in packed 16-bit arithmetic (compass8: a
    // 9-arc holds a point of every antipodal pair of the eight even circle points, a necessary
    // condition), survivors queued as pixel indices, the exact strength computed in
    // full 64-lane passes from the top of the queue (LDS accesses of one wave complete in order)
    {
        uint32_t* q = (uint32_t*)(In + inW * (dh + 6)) + 4 + wave * (RR_Q + 8);  // after the staged ROI
        // i / d = umulhi(i, ceil(2^32 / d)) for d >= 2 (the reciprocal of 1 does not fit 32 bits)
        const uint32_t m = (uint32_t)((0x100000000ull + dw - 1) / (uint64_t)dw);
        // staged dword columns holding detection pixels: In byte c = xx + 3 + o, xx in [0, dw)
        const int wd0 = (3 + o) >> 2, nd = ((dw + 2 + o) >> 2) - wd0 + 1;
        const uint32_t md = (uint32_t)((0x100000000ull + nd - 1) / (uint64_t)nd);
        const int total = dh * nd, iw = inW >> 2;
        const uint32_t tt = (uint32_t)t | ((uint32_t)t << 16);
        const uint32_t* In32 = (const uint32_t*)In;
        int np = 0;
        auto pass = [&](int base, int n) {  // q[base .. base + n), n <= 64
            if (lane < n) {
                const int i = q[base + lane];
                const int yy = dw > 1 ? (int)__umulhi((uint32_t)i, m) : i, xx = i - yy * dw;
                const int S = fast_strength_packed(In + (yy + 3) * inW + xx + 3 + o, inW);
                Sp[yy * dwp + xx] = (uint8_t)(S > t ? S : 0);  // only corners at t carry a strength
            }
        };
        // one strength call site (the last round flushes the queue's remainder)
        for (int i0 = wave * 64;; i0 += 256) {
            const bool last = i0 >= total;  // wave-uniform
            if (!last) {
                const int i = i0 + lane;
                uint32_t mask = 0u;
                int px0 = 0;
                if (i < total) {
                    const int yy = nd > 1 ? (int)__umulhi((uint32_t)i, md) : i, wd = wd0 + i - yy * nd;
                    const uint32_t* row = In32 + (yy + 3) * iw + wd;
                    const uint32_t cc = row[0], lf = row[-1], rg = row[1], up = row[-3 * iw], dn = row[3 * iw];
                    const int xx0 = 4 * wd - 3 - o;  // detection column of byte 0
                    const int lo = max(0, -xx0), hi = min(4, dw - xx0);
                    const uint32_t cols = ((1u << hi) - 1u) & ~((1u << lo) - 1u);
                    const uint32_t* d2 = row + 2 * iw;
                    const uint32_t* u2 = row - 2 * iw;
                    mask = compass8(lf, cc, rg, dn, up, d2[-1], d2[0], d2[1], u2[-1], u2[0], u2[1], tt) & cols;
                    px0 = yy * dw + xx0;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bool c = (mask >> j) & 1u;
                    const uint64_t bm = __ballot(c);
                    q[select_by_mask(bm, RR_Q, np + lanes_below(bm))] = (uint32_t)(px0 + j);  // RR_Q: trash slot
                    np += __popcll(bm);
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            while (np >= 64 || (last && np > 0)) {
                const int n = min(np, 64);
                np -= n;
                pass(np, n);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if (last) break;
        }
    }
    __syncthreads();
    KR_T(2);
    // 3x3 NMS on the corners only: Sp holds S where S > t and 0 elsewhere, so cv::FAST's strict
    // test s0 - 1 > (n > t ? n - 1 : 0) reads the plane as is (out-of-cell neighbours 0).  Each
    // wave scans its share of the plane's dwords, ballot-compacts the nonzero pixels into its
    // queue (the strength pass is done with it) and runs the NMS one corner per lane, all nine
    // reads issued together; a survivor sets its bit in its row's mask and counts into its row
    // (LDS atomics); the per-word pass below turns the masks into raster-order records
    {
        uint32_t* q = (uint32_t*)(In + inW * (dh + 6)) + 4 + wave * (RR_Q + 8);
        const uint32_t* Sp32 = (const uint32_t*)Sp;
        const uint32_t mr = rw > 1 ? (uint32_t)((0x100000000ull + rw - 1) / (uint64_t)rw) : 0u;
        auto nms = [&](int n) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            for (int k0 = 0; k0 < n; k0 += 64) {
                if (k0 + lane < n) {
                    const uint32_t code = q[k0 + lane];
                    const int yy = (int)(code >> 16), xx = (int)(code & 0xFFFFu);
                    const uint8_t* sp = Sp + yy * dwp + xx;
                    const int s0 = sp[0];
                    const bool xl = xx > 0, xr = xx + 1 < dw, yu = yy > 0, yd = yy + 1 < dh;
                    const int n0 = (yu && xl) ? sp[-dwp - 1] : 0, n1 = yu ? sp[-dwp] : 0, n2 = (yu && xr) ? sp[-dwp + 1] : 0;
                    const int n3 = xl ? sp[-1] : 0, n4 = xr ? sp[1] : 0;
                    const int n5 = (yd && xl) ? sp[dwp - 1] : 0, n6 = yd ? sp[dwp] : 0, n7 = (yd && xr) ? sp[dwp + 1] : 0;
                    const int m = max(max(max(n0, n1), max(n2, n3)), max(max(n4, n5), max(n6, n7)));
                    if (s0 > m) {  // s0 > t: a stored strength
                        atomicOr(&Bm[yy * bw + (xx >> 5)], 1u << (xx & 31));
                        atomicAdd(&rowc[yy], 1);
                    }
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        };
        int cn = 0;
        for (int i0 = wave * 64; i0 < nw; i0 += 256) {  // wave-uniform
            const int i = i0 + lane;
            uint32_t w4 = 0u;
            int yy = 0, wd = 0;
            if (i < nw) {
                yy = rw > 1 ? (int)__umulhi((uint32_t)i, mr) : i;
                wd = i - yy * rw;
                w4 = Sp32[i];
            }
            if (__ballot(w4 != 0u) == 0ull) continue;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool v = ((w4 >> (8 * j)) & 0xFFu) != 0u;
                const uint64_t m = __ballot(v);
                q[select_by_mask(m, RR_Q, cn + lanes_below(m))] = ((uint32_t)yy << 16) | (uint32_t)(4 * wd + j);
                cn += __popcll(m);
            }
            if (cn > RR_Q - 256) {
                nms(cn);
                cn = 0;
            }
        }
        if (cn) nms(cn);
    }
    __syncthreads();
    KR_T(3);
    __shared__ int s_total;
    if (wave == 0) {
        int carry = 0;
        for (int r0 = 0; r0 < dh; r0 += 64) {
            const int r = r0 + lane;
            const int v = r < dh ? rowc[r] : 0;
            const int incl = wave_incl_scan(v);
            if (r < dh) rowc[r] = carry + incl - v;
            carry += __builtin_amdgcn_readlane(incl, 63);
        }
        if (lane == 0) s_total = carry;
    }
    __syncthreads();
    const int totalK = s_total;
    // one thread per mask word: its survivors' raster positions start at the row's offset + the
    // set bits of the row's earlier words (each record: the stored strength and the position)
    for (int i = tid; i < dh * bw; i += 256) {
        uint32_t m = Bm[i];
        if (!m) continue;
        const int yy = i / bw, w = i - yy * bw;
        const uint32_t* br = Bm + yy * bw;
        int pos = rowc[yy];
        for (int w2 = 0; w2 < w; ++w2) pos += __popc(br[w2]);
        const uint32_t ly = (uint32_t)(ry0 + yy) << 12;
        while (m) {
            const int xx = 32 * w + __builtin_ctz(m);
            m &= m - 1;
            const uint32_t sc = (uint32_t)(Sp[yy * dwp + xx] - 1);
            out[pos++] = (sc << 24) | ly | (uint32_t)(rx0 + xx);
        }
    }
    __syncthreads();  // smem is reused by the caller
#if KR_TIMING
    // phases: 0 stage + zero, 1 compass + strength, 2 NMS, 3 row scan + output; [4] = cells,
    // [5] = detection pixels, [6] = corners kept
    if (tid == 0) {
        atomicAdd(&g_krtime[level][0], krt1 - krt0);
        atomicAdd(&g_krtime[level][1], krt2 - krt1);
        atomicAdd(&g_krtime[level][2], krt3 - krt2);
        atomicAdd(&g_krtime[level][3], __builtin_amdgcn_s_memrealtime() - krt3);
        atomicAdd(&g_krtime[level][4], 1ull);
        atomicAdd(&g_krtime[level][5], (unsigned long long)(dw * dh));
        atomicAdd(&g_krtime[level][6], (unsigned long long)totalK);
    }
#endif
    return totalK;
}

// The FAST(7) re-runs of every (frame, level), at every batch size, before k_select<.., false>
// (the in-k_select re-run path, k_select<.., true>, is no longer launched): NWG workgroups per
// (frame, level), workgroup (b * NWG + gw, l)
// re-running the level's fallback cells gw, gw + NWG, ... (in cell order), so one frame's
// re-runs — serial inside k_select's single workgroup per level — spread over many CUs.  A
// cell re-runs where the reference's does: not skipped, and min(count, cap) <= 3 with 0 for a
// cell with no detection area.  The new count is stored with RERUN_FLAG set, so a workgroup
// deciding later still counts the cell among the fallback cells (the ordinal -> workgroup
// assignment is the same everywhere, and so is the decision of every wave of a workgroup).
#ifndef KR_NWG_MIN  // least k_rerun workgroups per (frame, level): at B = 512, 1 / 2 / 3 / 4 measured
#define KR_NWG_MIN 3  // re-runs + selection 640x480 0.146 / 0.117 / 0.116 / 0.132 ms, 1241x376
#endif                // 0.463 / 0.380 / 0.357 / 0.406, 1280x720 0.814 / 0.809 / 0.765 / 0.910
#define RERUN_FLAG 0x40000000
#define COUNT_MASK 0x3FFFFFFF
#ifndef KR_WAVES
#define KR_WAVES 4  // waves per SIMD k_rerun's register allocation targets; re-runs + selection at
                    // B = 512 with 2 / 3 / 5 / 6 / 8: 1241x376 0.406 / 0.404 / 0.434 / 0.437 /
                    // 0.453 ms vs 0.357, 1280x720 0.90-1.17 vs 0.765
#endif
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(KR_WAVES))) k_rerun(const uint8_t* __restrict__ pyr, uint32_t* __restrict__ cand,
                                               int* __restrict__ cellCount, Geom g,
                                               const CellGeom* __restrict__ cells, int NWG) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int b = blockIdx.x / NWG, gw = blockIdx.x - b * NWG, l = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63;
    const LevelGeom& lg = g.lv[l];
    const int nC = lg.rows * lg.cols;
    const CellGeom* lc = cells + lg.cell0;
    uint32_t* fcand = cand + (long long)b * g.candPerFrame;
    int* fcount = cellCount + (long long)b * g.nCells + lg.cell0;
    int ord = 0;
    for (int c0 = 0; c0 < nC; c0 += 64) {
        const int c = c0 + lane;
        bool fb = false;
        if (c < nC) {
            const CellGeom& cg = lc[c];
            const int cnt = fcount[c];
            const int n = (cg.hx <= 6 || cg.hy <= 6) ? 0 : min(cnt & COUNT_MASK, cg.cap);
            fb = (cnt & RERUN_FLAG) || (!cg.skipped && n <= 3);
        }
        uint64_t m = __ballot(fb);
        while (m) {
            const int cc = c0 + __builtin_ctzll(m);
            m &= m - 1;
            if (ord++ % NWG != gw) continue;
            const CellGeom cg = lc[cc];
            const int dw = cg.hx - 6, dh = cg.hy - 6;
            int n = 0;
            if (dw > 0 && dh > 0) {
                const uint8_t* det = pyr + lg.base + (long long)b * lg.fstride +
                                     (long long)(EDGE + cg.y0 + 3) * lg.pitch + EDGE + cg.x0 + 3;
                n = cell_fast_rerun(det, lg.pitch, dw, dh, cg.x0 + 3, cg.y0 + 3, 7, smem, fcand + cg.candOff, tid, l);
            }
            if (tid == 0) fcount[cc] = n | RERUN_FLAG;
        }
    }
}

// ---- selection (retainBest replay) -------------------------------------------------------
struct ScoreGreater {  // KeypointResponseGreater on the packed FAST score
    ORB_HD bool operator()(uint32_t a, uint32_t b) const { return (a >> 24) > (b >> 24); }
};

// One workgroup per (level, frame).  In: each cell's NMS survivors at fastTh from k_fast, in
// arrival order, and their count.  (1) cells with <= 3 survivors are re-run at t = 7 (RERUN;
// otherwise k_rerun did it); (2) each
// cell's survivors are put in raster order — the order cv::FAST returns them, which
// retainBest's nth_element depends on; (3) nToRetain / redistribution (ORBextractor.cc:622-670);
// (4) retainBest per cell, concatenation in cell order, retainBest to the level quota
// (ORBextractor.cc:680-701) — exact libstdc++ nth_element replays.  Lists live in LDS when the
// level's survivors fit (Geom::selCap), otherwise in the frame's scratch area `cand2`.
// survivors per level held in LDS (beyond: the global-scratch path, same result), per frame
// size: (W*H / 200) rounded down to 512 in [1024, 3072] -- 1536 at 640x480 (6 -> 10 work-groups
// per CU: 0.177 -> 0.146 ms with 3072), 2048 at 1241x376 (0.499 -> 0.474), 3072 at 1280x720
// (2048 there: 0.84 -> 1.14, most levels past LDS)
inline int select_cap(int w, int h) {
    return std::min(3072, std::max(1024, (int)(((long long)w * h / 200) & ~511ll)));
}
// KeypointResponseGreater on HARRIS_SCORE elements: float response in the high word, the
// packed FAST record (identity) in the low word.
struct HarrisGreater {
    __device__ bool operator()(uint64_t a, uint64_t b) const {
        return __uint_as_float((uint32_t)(a >> 32)) > __uint_as_float((uint32_t)(b >> 32));
    }
};

// HarrisResponses (ORBextractor.cc:79-120) at level pixel (x, y), blockSize 7, k = 0.04:
// cellImage is a view into the level, so the 7x7 block starts at (x-3, y-3) of the level.
// g++ -O3 -march=native contracts the response to fma(-(k*s), s, fma(A, B, -(C*C))) (oracle
// harris_responses, DESIGN.md §FP policy).
__device__ __forceinline__ float harris_response(const uint8_t* roi, int pitch, int x, int y, float scale4) {
    const uint8_t* p0 = roi + (long long)(y - 3) * pitch + (x - 3);
    int a = 0, b = 0, c = 0;
    for (int i = 0; i < 7; ++i)
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            const uint8_t* ptr = p0 + (long long)i * pitch + j;
            const int Ix = (ptr[1] - ptr[-1]) * 2 + (ptr[-pitch + 1] - ptr[-pitch - 1]) + (ptr[pitch + 1] - ptr[pitch - 1]);
            const int Iy = (ptr[pitch] - ptr[-pitch]) * 2 + (ptr[pitch - 1] - ptr[-pitch - 1]) + (ptr[pitch + 1] - ptr[-pitch + 1]);
            a += Ix * Ix;
            b += Iy * Iy;
            c += Ix * Iy;
        }
    const float fa = (float)a, fb = (float)b, fc = (float)c;
    const float s = fa + fb;
    const float t3 = 0.04f * s;
    const float u = __builtin_fmaf(fa, fb, -(fc * fc));
    const float rsp = __builtin_fmaf(-t3, s, u);
    return rsp * scale4;
}

// Exclusive prefix of src[0..n) into dst[0..n], total into dst[n], on one wave (n <= 256).
__device__ __forceinline__ void wave_prefix(int* dst, const int* src, int n, int lane) {
    int carry = 0;
    for (int c0 = 0; c0 < n; c0 += 64) {
        const int c = c0 + lane;
        const int v = c < n ? src[c] : 0;
        const int incl = wave_incl_scan(v);
        if (c < n) dst[c] = carry + incl - v;
        carry += __builtin_amdgcn_readlane(incl, 63);
    }
    if (lane == 0) dst[n] = carry;
}

__device__ __forceinline__ int wave_sum(int v) { return wave_total(v); }

// Cell of list element i: the last c in [0, n) with off[c] <= i (off ascending, off[0] = 0).
__device__ __forceinline__ int cell_of(const int* off, int n, int i) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

#ifndef KR_TAIL_BATCH
#define KR_TAIL_BATCH 256  // batches below this resize every level with its own launch
#endif
#ifndef KS_WAVES
#define KS_WAVES 2  // waves per SIMD the register allocation targets
#endif

// The last of a frame's L k_select workgroups to finish writes the frame's per-level (first output
// slot, count) pairs and total (what k_lvl_prefix did in a launch of its own): each workgroup's
// thread 0 publishes its level count with an agent-scope atomic store (past its XCD's L2: the
// frame's workgroups run on different XCDs), waits for it, then counts itself in selDone[b];
// the one that brings it to L reads the L counts with agent-scope atomic loads and resets
// selDone[b] for the next launch.  Ordering: the only data handed over (lvlCount) is written and
// read with agent-scope atomics, which bypass the XCD's L2, and the writer waits for its store to
// complete (vmcnt(0)) before it counts itself; the last workgroup then takes an agent-scope
// acquire (one L1 / L2 invalidate, on that workgroup only) before its loads.  (A __threadfence()
// release on every workgroup writes back the L2 of each: +60 us per c3 step.)
__device__ __forceinline__ void select_frame_done(int b, int L, int l, int keep, int* __restrict__ lvlCount,
                                                  int* __restrict__ selDone, int2* __restrict__ lvlInfo,
                                                  int* __restrict__ counts) {
    __hip_atomic_store(&lvlCount[(long long)b * L + l], keep, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (__hip_atomic_fetch_add(&selDone[b], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != L - 1) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    int c[ORB_MAX_LEVELS];
#pragma unroll
    for (int l = 0; l < ORB_MAX_LEVELS; ++l)
        c[l] = __hip_atomic_load(&lvlCount[(long long)b * L + min(l, L - 1)], __ATOMIC_RELAXED,  // (in bounds:
                                 __HIP_MEMORY_SCOPE_AGENT);                                      // all issued at once)
    int before = 0;
#pragma unroll
    for (int l = 0; l < ORB_MAX_LEVELS; ++l)
        if (l < L) {
            lvlInfo[(long long)b * ORB_MAX_LEVELS + l] = make_int2(before, c[l]);
            before += c[l];
        }
    counts[b] = before;
    __hip_atomic_store(&selDone[b], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// RERUN: only <.., false> is instantiated (k_rerun runs first at every batch size).  The parameter
// and its path are still here because the <.., false> kernels keep s_fb and one store to it from
// that path: without the path their static LDS goes 6448 -> 5408 B and 14 instructions go, a change
// of the kernel to be measured on its own.
template <bool HARRIS, bool RERUN>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(KS_WAVES))) k_select(const uint8_t* __restrict__ pyr, uint32_t* __restrict__ cand,
                                                uint32_t* __restrict__ cand2, int* __restrict__ cellCount, Geom g,
                                                const CellGeom* __restrict__ cells, uint32_t* __restrict__ lvlOut,
                                                int* __restrict__ lvlCount, uint64_t* __restrict__ candH,
                                                float* __restrict__ lvlResp, float harrisScale4, int* __restrict__ selDone,
                                                int2* __restrict__ lvlInfo, int* __restrict__ counts) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    __shared__ int s_cnt[ORB_MAX_CELLS_PER_LEVEL];
    __shared__ int s_ret[ORB_MAX_CELLS_PER_LEVEL];
    __shared__ int s_off[ORB_MAX_CELLS_PER_LEVEL + 1];
    __shared__ int s_koff[ORB_MAX_CELLS_PER_LEVEL + 1];
    __shared__ uint8_t s_skip[ORB_MAX_CELLS_PER_LEVEL];
    __shared__ int s_fb[ORB_MAX_CELLS_PER_LEVEL + 1];  // cells to re-run at t = 7, count last
    __shared__ int s_coff[ORB_MAX_CELLS_PER_LEVEL];    // candOff of every cell
    // grid (frame, level): workgroup i runs on XCD i % 8, so every XCD gets every level (with
    // (level, frame) all the heavy level-0 lists landed on one XCD), heaviest level first
    const int b = blockIdx.x, l = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    KS_T(0);
    const LevelGeom& lg = g.lv[l];
    const int nC = lg.rows * lg.cols;
    const CellGeom* lc = cells + lg.cell0;
    uint32_t* fcand = cand + (long long)b * g.candPerFrame;
    int* fcount = cellCount + (long long)b * g.nCells + lg.cell0;
    if (wave == 0) {  // counts, skip flags, and the list of cells to re-run (ascending, RERUN)
        constexpr int CPL = ORB_MAX_CELLS_PER_LEVEL / 64;
        int cnt[CPL], cap[CPL], skip[CPL], hx[CPL], hy[CPL], coff[CPL];
#pragma unroll
        for (int j = 0; j < CPL; ++j) {  // every load of the wave in flight at once
            const int c = 64 * j + lane;
            if (c < nC) {
                cnt[j] = fcount[c];
                cap[j] = lc[c].cap;
                skip[j] = lc[c].skipped;
                hx[j] = lc[c].hx;
                hy[j] = lc[c].hy;
                coff[j] = lc[c].candOff;
            }
        }
        int nfb = 0;
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            const int c = 64 * j + lane;
            bool fb = false;
            if (c < nC) {
                // (k_rerun's counts carry RERUN_FLAG; such a cell has been re-run: not again)
                const int n = (skip[j] || hx[j] <= 6 || hy[j] <= 6) ? 0 : min(cnt[j] & COUNT_MASK, cap[j]);
                s_cnt[c] = n;
                s_skip[c] = (uint8_t)skip[j];
                s_coff[c] = coff[j];
                fb = RERUN && !skip[j] && n <= 3;
            }
            const uint64_t m = __ballot(fb);
            if (fb) s_fb[nfb + __popcll(m & ((lane == 0) ? 0ull : (~0ull >> (64 - lane))))] = c;
            nfb += __popcll(m);
        }
        if (lane == 0) s_fb[ORB_MAX_CELLS_PER_LEVEL] = nfb;
    }
    __syncthreads();
    // (1) FAST(cellImage, keys, 7, true) where a cell kept <= 3 (a skipped cell is `continue`d)
    {
        const int nfb = s_fb[ORB_MAX_CELLS_PER_LEVEL];
        for (int f = 0; f < (RERUN ? nfb : 0); ++f) {
            const int c = s_fb[f];
            const CellGeom cg = lc[c];
            const int dw = cg.hx - 6, dh = cg.hy - 6;
            int n = 0;
            if (dw > 0 && dh > 0) {
                const uint8_t* det = pyr + lg.base + (long long)b * lg.fstride +
                                     (long long)(EDGE + cg.y0 + 3) * lg.pitch + EDGE + cg.x0 + 3;
                n = cell_fast_rerun(det, lg.pitch, dw, dh, cg.x0 + 3, cg.y0 + 3, 7, smem, fcand + cg.candOff, tid, l);
            }
            if (tid == 0) {
                s_cnt[c] = n;
                fcount[c] = n;
            }
            __syncthreads();
        }
    }
    KS_T(1);
    if (wave == 0) {
        wave_prefix(s_off, s_cnt, nC, lane);
        // (3) nToRetain / nToDistribute / bNoMore bookkeeping (ORBextractor.cc:622-670), one
        // lane per cell: within a pass every cell's update reads only the pass constants, and
        // the pass totals are integer sums, so the lanes reproduce the sequential loop exactly.
        // A skipped cell keeps 0 and is not bNoMore after the first pass (the reference
        // `continue`s past it), then takes the tot = 0 branch of the redistribution.
        constexpr int CPL = ORB_MAX_CELLS_PER_LEVEL / 64;
        const int nfc = lg.nfc;
        int ret[CPL], tot[CPL];
        bool more[CPL];  // live and not bNoMore
        int dist = 0, nm = 0;
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            const int c = 64 * j + lane;
            more[j] = false;
            ret[j] = 0;
            tot[j] = 0;
            if (c < nC) {
                const bool sk = s_skip[c] != 0;
                tot[j] = sk ? 0 : s_cnt[c];
                if (sk) {
                    more[j] = true;
                } else if (tot[j] > nfc) {
                    ret[j] = nfc;
                    more[j] = true;
                } else {
                    ret[j] = tot[j];
                    dist += nfc - tot[j];
                    nm++;
                }
            }
        }
        int nToDistribute = wave_sum(dist), nNoMore = wave_sum(nm);
        while (nToDistribute > 0 && nNoMore < nC) {
            const int nNew = nfc + (int)ceilf((float)nToDistribute / (nC - nNoMore));
            dist = 0;
            nm = 0;
#pragma unroll
            for (int j = 0; j < CPL; ++j) {
                if (!more[j]) continue;
                if (tot[j] > nNew) {
                    ret[j] = nNew;
                } else {
                    ret[j] = tot[j];
                    dist += nNew - tot[j];
                    more[j] = false;
                    nm++;
                }
            }
            nToDistribute = wave_sum(dist);
            nNoMore += wave_sum(nm);
        }
#pragma unroll
        for (int j = 0; j < CPL; ++j)
            if (64 * j + lane < nC) s_ret[64 * j + lane] = ret[j];
    }
    __syncthreads();
    KS_T(2);
    const int M = s_off[nC];
    const int selCap = g.selCap;
    const bool inLds = M <= selCap;
    uint32_t* raw = (uint32_t*)smem;                                      // arrival order
    uint32_t* srt = inLds ? raw + selCap : cand2 + (long long)b * g.candPerFrame;  // raster order
    const uint32_t* srcOf = inLds ? raw : fcand;
    if (inLds) {  // the level's survivors, cell after cell, one element per thread (4 loads in flight)
        for (int i0 = tid; i0 < M; i0 += 1024) {
            uint32_t v[4];
            int dsti[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int i = i0 + 256 * u;
                dsti[u] = -1;
                if (i < M) {
                    const int c = cell_of(s_off, nC, i);
                    v[u] = fcand[s_coff[c] + (i - s_off[c])];
                    dsti[u] = i;
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (dsti[u] >= 0) raw[dsti[u]] = v[u];
        }
        __syncthreads();
        // (2) rank sort of each cell by position (positions are unique), one element per thread
        for (int i = tid; i < M; i += 256) {
            const int c = cell_of(s_off, nC, i);
            const int o = s_off[c], n = s_cnt[c];
            const uint32_t e = raw[i], key = e & 0xFFFFFFu;
            int r = 0;
            for (int j2 = 0; j2 < n; ++j2) r += (raw[o + j2] & 0xFFFFFFu) < key;
            srt[o + r] = e;
        }
    } else {
        // (2) as above on the frame's scratch area, one wave per cell
        for (int c = wave; c < nC; c += 4) {
            const int n = s_cnt[c];
            const uint32_t* seg = srcOf + lc[c].candOff;
            uint32_t* dst = srt + lc[c].candOff;
            for (int i = lane; i < n; i += 64) {
                const uint32_t e = seg[i], key = e & 0xFFFFFFu;
                int r = 0;
                for (int j2 = 0; j2 < n; ++j2) r += (seg[j2] & 0xFFFFFFu) < key;
                dst[r] = e;
            }
        }
    }
    __syncthreads();
    if constexpr (HARRIS) {
        // HarrisResponses on every cell keypoint (ORBextractor.cc:616-620), then the same
        // retention on (response, record) pairs
        uint64_t* hs = inLds ? (uint64_t*)(smem + (size_t)8 * selCap) : candH + (long long)b * g.candPerFrame;
        const uint8_t* roi = pyr + lg.base + (long long)b * lg.fstride + (long long)EDGE * lg.pitch + EDGE;
        for (int c = wave; c < nC; c += 4) {
            const int o = inLds ? s_off[c] : lc[c].candOff;
            for (int i = lane; i < s_cnt[c]; i += 64) {
                const uint32_t e = srt[o + i];
                const float r = harris_response(roi, lg.pitch, e & 0xFFF, (e >> 12) & 0xFFF, harrisScale4);
                hs[o + i] = ((uint64_t)__float_as_uint(r) << 32) | e;
            }
        }
        __syncthreads();
        HarrisGreater hcomp;
        for (int c = lane * 4 + wave; c < nC; c += 256) {  // cell c on wave c % 4
            uint64_t* seg = hs + (inLds ? s_off[c] : lc[c].candOff);
            s_cnt[c] = orbsel::retain_best(seg, s_cnt[c], s_ret[c], hcomp);
        }
        __syncthreads();
        if (wave == 0) wave_prefix(s_koff, s_cnt, nC, lane);
        __syncthreads();
        const int K = s_koff[nC];
        uint64_t* list;
        if (inLds) {  // kept prefixes of hs -> the raw + srt region (disjoint)
            list = (uint64_t*)smem;
            for (int c = wave; c < nC; c += 4)
                for (int k = lane; k < s_cnt[c]; k += 64) list[s_koff[c] + k] = hs[s_off[c] + k];
        } else {
            list = hs + lc[0].candOff;
            if (tid == 0)
                for (int c = 0; c < nC; ++c) {
                    const uint64_t* src = hs + lc[c].candOff;
                    for (int k = 0; k < s_cnt[c]; ++k) list[s_koff[c] + k] = src[k];
                }
        }
        __syncthreads();
        int keep = K;
        if (K > lg.nDesired) {
            keep = lg.nDesired;
            if (tid == 0) orbsel::retain_best(list, K, lg.nDesired, hcomp);
        }
        __syncthreads();
        const long long ob = (long long)b * g.kpCap + lg.kpBase;
        for (int k = tid; k < keep; k += 256) {
            const uint64_t v = list[k];
            lvlOut[ob + k] = (uint32_t)v;
            lvlResp[ob + k] = __uint_as_float((uint32_t)(v >> 32));
        }
        if (tid == 0) {
            select_frame_done(b, g.L, l, keep, lvlCount, selDone, lvlInfo, counts);
        }
        return;
    }
    // (4) retainBest per cell, then the level list in cell order, then retainBest to the quota
    KS_T(3);
    ScoreGreater comp;
    // cells dealt round-robin over the four waves (cell c on wave c % 4): a level's few dozen
    // serial replays run on four SIMDs instead of one wave's lanes
    // (measured and dropped, round 4: cells of > 32 / 64 / 128 survivors retained by a whole wave
    // with the ballot partitions: k_select 71 -> 83-88 us c3, 105 -> 113-122 us c4)
    for (int c = lane * 4 + wave; c < nC; c += 256) {
        uint32_t* seg = srt + (inLds ? s_off[c] : lc[c].candOff);
        s_cnt[c] = orbsel::retain_best(seg, s_cnt[c], s_ret[c], comp);
    }
    __syncthreads();
    KS_T(4);
    if (wave == 0) wave_prefix(s_koff, s_cnt, nC, lane);
    __syncthreads();
    const int K = s_koff[nC];
    uint32_t* list;
    if (inLds) {  // kept prefixes of srt -> raw (disjoint regions), one element per thread
        for (int i = tid; i < K; i += 256) {
            const int c = cell_of(s_koff, nC, i);
            raw[i] = srt[s_off[c] + (i - s_koff[c])];
        }
        list = raw;
    } else {  // sequential in-place compaction (dest <= src, ascending) in cand2's level area
        list = srt + lc[0].candOff;
        if (tid == 0)
            for (int c = 0; c < nC; ++c) {
                const uint32_t* src = srt + lc[c].candOff;
                for (int k = 0; k < s_cnt[c]; ++k) list[s_koff[c] + k] = src[k];
            }
    }
    __syncthreads();
    int keep = K;
    if (K > lg.nDesired) {
        keep = lg.nDesired;
        if (inLds) {  // one wave, partitions by ballot (nth_select.h); scratch = the free srt region
            uint16_t* Lp = (uint16_t*)srt;
            if (wave == 0)
                orbsel::retain_best_wave(list, K, lg.nDesired, comp, Lp, Lp + K, lane);
        } else if (tid == 0) {
            orbsel::retain_best(list, K, lg.nDesired, comp);
        }
    }
    __syncthreads();
    KS_T(5);
    uint32_t* out = lvlOut + (long long)b * g.kpCap + lg.kpBase;
    for (int k = tid; k < keep; k += 256) out[k] = list[k];
    if (tid == 0) {
        select_frame_done(b, g.L, l, keep, lvlCount, selDone, lvlInfo, counts);
    }
#if KS_TIMING
    // phases: 0 counts + re-runs, 1 bookkeeping, 2 load + raster sort, 3 per-cell retainBest,
    // 4 level list + level retainBest, 5 output; [6] = survivors M, [7] = workgroups
    if (tid == 0) {
        atomicAdd(&g_kstime[l][0], kst1 - kst0);
        atomicAdd(&g_kstime[l][1], kst2 - kst1);
        atomicAdd(&g_kstime[l][2], kst3 - kst2);
        atomicAdd(&g_kstime[l][3], kst4 - kst3);
        atomicAdd(&g_kstime[l][4], kst5 - kst4);
        atomicAdd(&g_kstime[l][5], __builtin_amdgcn_s_memrealtime() - kst5);
        atomicAdd(&g_kstime[l][6], (unsigned long long)M);
        atomicAdd(&g_kstime[l][7], 1ull);
    }
#endif
}

// ---- orientation + descriptor -------------------------------------------------------------
// One wave per keypoint slot.  Two memory round trips per wave: (1) the slot's packed record
// and the frame's per-level counts; (2) the raw 43x43 window around the keypoint (rows y-21 ..
// y+21, 16-byte loads into the wave's own LDS: 64 B per row from the 16-aligned column
// (x-5) & ~15 of the padded level).  From the window:
//   * IC_Angle (ORBextractor.cc:124-151) on its raw 31x31 disc;
//   * the descriptor image the reference reads after GaussianBlur(level ROI, 7x7, sigma 2)
//     in place (ORBextractor.cc:760), only where rBRIEF samples it: the row pass of the
//     fixed-point kernel (18, 34, 49, 55, 49, 34, 18) over the window's rows on the matrix
//     cores (three v_mfma_i32_16x16x64_i8 M-tiles x four N-tiles against a banded tap matrix),
//     stored as u16 sums in LDS, rows interleaved in pairs; then per sample the column pass by
//     four v_dot2 over row pairs, OpenCV's rounding for that column (SSE2 columns
//     x < 4*floor(w/4) half-to-even, the scalar tail half-up), or the raw
//     border byte where the sample lies outside the ROI (in-place ROI blur: the padding stays
//     un-blurred).  Exact integers throughout (T <= 257 * 65535 < 2^24).
// OD_WAVES keypoint slots per workgroup.  A wave's window and sums are its own (LDS is in order
// per wave); the two workgroup barriers only hand the IC moments to wave 0, which computes the
// slots' angle / sin / cos once, and hand those back.
#define OD_WR 21   // window reach: rBRIEF |offset| <= 18 + the blur's 3
#ifndef OD_WP
#define OD_WP 64   // LDS row pitch of the raw window (bytes).  80 (row blocks 4 rows apart on
                   // different banks: the row pass's 7-way conflicts become 2-way) measured
                   // slower: 640x480 0.607 vs 0.597 ms, 1241x376 1.183 vs 1.172
#endif
#define OD_HC 40   // row-pass columns: x-18 .. x+21 (10 groups of 4)
#define OD_HPR 22  // row pairs of the row-pass sums (window rows 0 .. 43)
#define OD_HN 56   // row-pass sum columns per pair row (window columns n = 0 .. 55 >= o0 + 39; hc = n - o0)
#define OD_BUF (OD_HPR * OD_HN * 4)  // per-wave LDS: the 44-row window, then (overlaid) the sums
static_assert(48 * OD_WP <= OD_BUF, "window rows 0 .. 47 inside the wave's buffer");
typedef int i32x4v __attribute__((ext_vector_type(4)));
// first window row of the three row-pass M-tiles (rows 28 .. 31 computed twice, identically)
__device__ constexpr int kOdRow[3] = {0, 16, 28};
// column-pass taps over row pairs (low half = the even row): rows r0-3 .. r0+4 when r0 is even
#define GP_E0 (18u | (34u << 16))
#define GP_E1 (49u | (55u << 16))
#define GP_E2 (49u | (34u << 16))
#define GP_E3 (18u | (0u << 16))
// ... and rows r0-4 .. r0+3 when r0 is odd (the even row of the first pair is r0-1, tap 0)
#define GP_O0 (0u | (18u << 16))
#define GP_O1 (34u | (49u << 16))
#define GP_O2 (55u | (49u << 16))
#define GP_O3 (34u | (18u << 16))

typedef unsigned short u16x2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t dot2u(uint32_t a, uint32_t b, uint32_t c) {
    return __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2v, a), __builtin_bit_cast(u16x2v, b), c, false);
}

// cvRound-equivalent of T / 65536: half to even (SSE2 columns) or half up (scalar tail), then
// the saturating cast.
__device__ __forceinline__ uint32_t blur_round(uint32_t T, bool tail) {
    const uint32_t bias = tail ? 1u : ((T >> 16) & 1u);
    return min((T + 0x7FFFu + bias) >> 16, 255u);
}

#ifndef OD_WAVES
#define OD_WAVES 4  // keypoint slots (waves) per workgroup (8 / 2 measured slower: 0.521 / 0.474 vs 0.468 ms c3;
                    // two slots per wave, lanes 0-31 / 32-63, 2 or 4 waves per workgroup: 0.531 / 0.567 vs
                    // 0.428 ms c3, 1.018 / 1.093 vs 0.818 c4 -- half the waves per CU, longer chains)
#endif
__global__ void __launch_bounds__(64 * OD_WAVES) k_orient_desc(const uint8_t* __restrict__ pyr, Geom g,
                                                     const uint32_t* __restrict__ lvlOut,
                                                     const uint8_t* __restrict__ slotLvl,
                                                     const int2* __restrict__ lvlInfo, orb_keypoint_t* __restrict__ kps,
                                                     uint8_t* __restrict__ desc, const float* __restrict__ lvlResp) {
    // per wave: the raw window, then (overlaid) the row-pass sums
    __shared__ __attribute__((aligned(16))) uint8_t s_buf[OD_WAVES][OD_BUF];
    __shared__ int2 s_mom[OD_WAVES];     // the waves' IC moments (m01, m10)
    __shared__ float4 s_trig[OD_WAVES];  // angle, sin, cos of the waves' keypoints
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    // XCD-aware block order: workgroup i runs on XCD i % 8, so give each XCD a contiguous run
    // of keypoints (neighbouring keypoints share window rows: L2 hits instead of HBM re-reads)
    int bid = blockIdx.y * gridDim.x + blockIdx.x;
    const int full = (gridDim.x * gridDim.y) & ~7;
    if (bid < full) bid = (bid & 7) * (full >> 3) + (bid >> 3);
    const int b = (int)__umulhi((uint32_t)bid, g.odDivMagic);  // bid / gridDim.x (exact: bid * gridDim.x < 2^32)
    const int k = (bid - b * gridDim.x) * OD_WAVES + wave;  // slot: level l owns [kpBase_l, kpBase_l + nDesired_l)
    // wave-uniform record: x, y and the window base live in SGPRs (its load first: the window's
    // address depends on it)
    const int kc = min(k, g.kpCap - 1);
    // (32-bit element offsets into the per-slot arrays: the host checks B * kpCap * 32 < 2^32)
    const uint32_t fslot = (uint32_t)b * (uint32_t)g.kpCap;
    const uint32_t e = (uint32_t)__builtin_amdgcn_readfirstlane((int)lvlOut[fslot + (uint32_t)kc]);
    // the slot's level: one byte of the host-built slot -> level table (a scalar load beside the
    // record's), then the frame's (first output slot, count) of that level (select_frame_done)
    const uint32_t lw = *(const uint32_t*)(slotLvl + (kc & ~3));
    const int l = (int)((lw >> (8 * (kc & 3))) & 0xFFu);
    const int2 linfo = lvlInfo[(uint32_t)b * ORB_MAX_LEVELS + (uint32_t)l];
    const LevelGeom& lg = g.lv[l];
    const int idx = k - lg.kpBase;
    // raw window: padded rows y-5 .. y+37 (level rows y-21 .. y+21), padded columns xa .. xa+63
    // (keypoints lie in 16 <= x <= w-7 and y likewise, App. B / DESIGN §4; the clamp only keeps
    // an empty slot's stale record inside the level; the last row's over-read stays inside the
    // pyramid's tail slack).  Loaded before the slot is known to be filled: the per-level counts
    // are scalar loads of their own
    const int x = min(max((int)(e & 0xFFF), 16), lg.w - 7), y = min(max((int)((e >> 12) & 0xFFF), 16), lg.h - 7);
    const int score = e >> 24;
    const int xa = (x - 5) & ~15;
    const uint4* src = (const uint4*)(pyr + lg.base + (long long)b * lg.fstride +
                                      (long long)(y + EDGE - OD_WR) * lg.pitch + xa);
    const uint32_t pu = (uint32_t)lg.pitch >> 4;
    uint8_t* W = s_buf[wave];
    uint32_t* Hs = (uint32_t*)s_buf[wave];
    uint32_t ico[5], ic10[5], ic01[5];  // IC_Angle: the lane's patch dwords and their coefficients
    i32x4v Bf[4];  // the row pass's B fragments (constant; in flight with the window loads)
    // (PC-relative addresses per table load: routing the tables through one opaque SGPR base
    // saved ~30 SALU per wave but let the loads sink below the window's, 0.420 -> 0.440 ms c3)
#pragma unroll
    for (int t = 0; t < 4; ++t) Bf[t] = __builtin_bit_cast(i32x4v, c_rowB[t * 64 + lane]);
    constexpr int NU = (2 * OD_WR + 1) * 4;  // 172 16-byte units
    uint4 v[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int i = lane + 64 * j, r = i >> 2, c = i & 3;
        v[j] = src[i < NU ? __umul24((uint32_t)r, pu) + c : 0u];
    }
    // the IC tables of this alignment (dword loads), in flight with the window
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const int sh320 = 320 * ((x + 1 - xa) & 3);
        ico[j] = c_icoff[lane + 64 * j];
        ic10[j] = c_ic10[sh320 + lane + 64 * j];
        ic01[j] = c_ic01[sh320 + lane + 64 * j];
    }
    {
        // the window as i8 p - 128 (p ^ 0x80): the row pass's MFMA operand as it is, and IC_Angle's
        // sums unchanged (the disc is symmetric in u and v: sum u = sum v = 0 over it).  All 192
        // units stored (units >= 172 repeat unit 0 into the buffer's unused tail, before the
        // row-pass sums are written): no masked store
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int i = lane + 64 * j;
            const uint4 w = make_uint4(v[j].x ^ 0x80808080u, v[j].y ^ 0x80808080u, v[j].z ^ 0x80808080u,
                                       v[j].w ^ 0x80808080u);
            ((uint4*)W)[(i >> 2) * (OD_WP / 16) + (i & 3)] = w;
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // LDS is in order per wave; compiler fence
    // IC_Angle (ORBextractor.cc:124-151): the disc sums m10 = sum u*I, m01 = sum v*I over
    // |u| <= umax[|v|], one patch dword per lane and step (patch row v = window row v + 21,
    // patch dword c = window dword pd0 + c): two v_dot4_i32_i8 of the window dword (p - 128)
    // with the dword's coefficient bytes (0 outside the disc).  sum u (p - 128) = sum u p since
    // sum u = 0 over the symmetric disc (likewise v): exact integer sums, any order.
    int m01 = 0, m10 = 0;
    {
        const int pc = x + 1 - xa;  // window column of patch column u = -15
        const uint8_t* P0 = W + (OD_WR - HALF_PATCH) * OD_WP + 4 * (pc >> 2);  // the patch's first dword
        // five full 64-lane steps: dwords n >= 279 (patch rows 31 .. 35, still inside the
        // 43-row window) carry zero coefficients, so no lane is masked off
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const int pm = *(const int*)(P0 + ico[j]);
            m10 = __builtin_amdgcn_sdot4(pm, (int)ic10[j], m10, false);
            m01 = __builtin_amdgcn_sdot4(pm, (int)ic01[j], m01, false);
        }
    }
    // output position: level-major order (ORBextractor.cc:749-778)
    const int before = linfo.x, cntL = linfo.y;
    // an empty slot's wave does no work but stays for the workgroup's two barriers
    const bool active = k < g.kpCap && idx < cntL;  // wave-uniform
    // IC_Angle's sums, then the angle arithmetic (fastAtan2, glibc sincosf: ~100 VALU, a fifth of a
    // keypoint's) once per workgroup: wave 0's lanes 0 .. 3 for the four slots, between the
    // two barriers, while the other waves run their row passes
    m01 = wave_total(m01);
    m10 = wave_total(m10);
    typedef float f32x2v __attribute__((ext_vector_type(2)));
    // The rBRIEF pattern: points 8 lane .. 8 lane + 7 (tests 4 lane .. 4 lane + 3), pair q =
    // (x, y) of point 8 lane + q.  The rule of DESIGN §6.1, as code: eight fully coalesced
    // dwordx2 rows of the pair-major table (each instruction reads 512 contiguous bytes, four
    // cache lines no other pattern load touches; the float4 form read all 32 lines of the table
    // with each of its four instructions, 64-B lane stride, and returned wrong data), issued by
    // one asm statement and waited by another before the first sample (the registers are outputs
    // of the first and in-out operands of the second: the compiler can neither move the loads nor
    // read the registers early).  Issued by the active waves once their own row pass is done, in
    // flight across the second barrier.
    f32x2v pat[8];
    auto issue_pattern = [&]() {
        const uint32_t poff = 8u * (uint32_t)lane;
        asm volatile(
            "global_load_dwordx2 %0, %8, %9\n\t"
            "global_load_dwordx2 %1, %8, %9 offset:512\n\t"
            "global_load_dwordx2 %2, %8, %9 offset:1024\n\t"
            "global_load_dwordx2 %3, %8, %9 offset:1536\n\t"
            "global_load_dwordx2 %4, %8, %9 offset:2048\n\t"
            "global_load_dwordx2 %5, %8, %9 offset:2560\n\t"
            "global_load_dwordx2 %6, %8, %9 offset:3072\n\t"
            "global_load_dwordx2 %7, %8, %9 offset:3584"
            : "=&v"(pat[0]), "=&v"(pat[1]), "=&v"(pat[2]), "=&v"(pat[3]), "=&v"(pat[4]), "=&v"(pat[5]),
              "=&v"(pat[6]), "=&v"(pat[7])
            : "v"(poff), "s"((const float*)c_patternf)
            : "memory");
    };
    if (lane == 0) s_mom[wave] = make_int2(m01, m10);
    lds_barrier();
    if (wave == 0 && lane < OD_WAVES) {
        const int2 mm = s_mom[lane];
        const float ang = fast_atan2((float)mm.x, (float)mm.y);
        // computeOrbDescriptor (ORBextractor.cc:155-194)
        const float factorPI = (float)(3.14159265358979323846 / 180.f);
        float sa, ca;
        glibc_sincosf(ang * factorPI, &sa, &ca);
        s_trig[lane] = make_float4(ang, sa, ca, 0.f);
    }
    // row pass on the matrix cores: for M-tile m (window rows kOdRow[m] .. +15) and N-tile t
    // (output columns n = 16t .. 16t+15 of the window), H = A x B with A = the window bytes as
    // i8 (p ^ 0x80 = p - 128) and B = the banded tap matrix B[k][n] = tap[k - n] (c_rowB), one
    // v_mfma_i32_16x16x64_i8 over all 64 window columns.  Columns 61 .. 63 (never inside a
    // needed band: sum column hc reads window columns o0 + hc .. o0 + hc + 6 <= 60) carry
    // (127, 127, 11) in A and (127, 127, 58) in B: + 32896 = 128 * 257 restores the unsigned
    // sum, so H = sum tap * p exactly (0 .. 65535).  Lane l holds H of column 16t + (l & 15),
    // rows kOdRow[m] + 4(l >> 4) .. +3: two row-pair dwords Hs[pair][n] (56 columns per pair
    // row, so 8 work-groups fit a CU; the column pass adds o0).  All window reads are issued before the first write (LDS
    // is in order per wave), so the sums overlay the window.
    if (active) {
        const int r16 = lane & 15, h4 = lane >> 4;
        const uint4* W4 = (const uint4*)W;
        uint4 A[3];
#pragma unroll
        for (int m = 0; m < 3; ++m) A[m] = W4[(kOdRow[m] + r16) * (OD_WP / 16) + h4];
        const uint32_t keep = h4 == 3 ? 0x000000FFu : 0xFFFFFFFFu;
        const uint32_t bias = h4 == 3 ? 0x0B7F7F00u : 0u;
        const i32x4v zero = {0, 0, 0, 0};
        {
        uint32_t* q3 = Hs + 2 * h4 * OD_HN + r16 + (r16 >= 8 ? 32 : 48);
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            i32x4v a;
            a.x = (int)A[m].x;  // the window is stored as p ^ 0x80
            a.y = (int)A[m].y;
            a.z = (int)A[m].z;
            a.w = (int)((A[m].w & keep) | bias);
            i32x4v c[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) c[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, Bf[t], zero, 0, 0, 0);
            uint32_t* q = Hs + (kOdRow[m] / 2 + 2 * h4) * OD_HN + r16;
            // N-tile 3 first: its columns 56 .. 63 (beyond the 56-column pair rows) go to the
            // lane's own tile-2 slots, which tile 2 then overwrites (same lane, program order)
            q3[0] = (uint32_t)c[3].x | ((uint32_t)c[3].y << 16);
            q3[OD_HN] = (uint32_t)c[3].z | ((uint32_t)c[3].w << 16);
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                q[16 * t] = (uint32_t)c[t].x | ((uint32_t)c[t].y << 16);
                q[16 * t + OD_HN] = (uint32_t)c[t].z | ((uint32_t)c[t].w << 16);
            }
            q3 += (kOdRow[m + (m < 2)] - kOdRow[m]) / 2 * OD_HN;
        }
        }
    }
    if (active) issue_pattern();
    lds_barrier();  // s_trig is written (and the row-pass sums: LDS)
    if (!active) return;
    const float4 trig = s_trig[wave];
    const float angle = trig.x, a = trig.z, bsin = trig.y;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the row-pass sums are in LDS
    // wave-uniform: can any sample leave the ROI (raw border bytes) or reach the scalar tail?
    const bool edge = x - 18 < 0 || x + 18 >= lg.w || y - 18 < 0 || y + 18 >= lg.h;
    const bool tailAny = x + 18 >= lg.xsimd_blur;
    const int o0 = x - 5 - xa;  // window column of sum column hc = 0 (level column x - 18)
    // Sample offsets: dy = cvRound(fma(px, b, py * a)), dx = cvRound(fma(px, a, -(py * b)))
    // (ORBextractor.cc:168-169 as g++ contracts them) on packed f32 pairs; cvRound = round half
    // to even of the float, taken as the low bits of v + (1.5 * 2^23 + 18) (one more RNE
    // rounding, exact for |v| < 2^22; the even addend keeps the tie parity), so the bits are
    // kMagic + dy + 18 = kMagic + r0 (window row of the first tap) and kMagic + dx + 18.
    constexpr uint32_t kMagic = 0x4B400000u;
    const f32x2v rA = {a, -bsin}, rB = {bsin, a};
    // tap words of the column pass for even / odd r0, opaque so they stay in VGPRs
    uint32_t tE0 = GP_E0, tE1 = GP_E1, tE2 = GP_E2, tE3 = GP_E3;
    uint32_t tO0 = GP_O0, tO1 = GP_O1, tO2 = GP_O2, tO3 = GP_O3;
    asm volatile("" : "+v"(tE0), "+v"(tE1), "+v"(tE2), "+v"(tE3), "+v"(tO0), "+v"(tO1), "+v"(tO2), "+v"(tO3));
    // sum (pair p, column dx + 18 + o0) = hbase[56 p + bits_x] (32-bit LDS addresses wrap); the
    // pair index p = r0 >> 1 comes from v_mul_u32_u24 of by >> 1, whose low 24 bits are
    // ((kMagic >> 1) & 0xFFFFFF) + p: that constant is taken off the base
    const uint32_t* hbase = Hs + (o0 - (int)kMagic) - (int)(OD_HN * ((kMagic >> 1) & 0xFFFFFFu));
    const uint32_t hb = (uint32_t)((const uint8_t*)hbase - s_buf[0]);  // as a byte offset from s_buf
    // tail columns (scalar-tail rounding): x + dx >= xsimd_blur <=> bits_x >= thr
    const uint32_t thr = kMagic + 18u + (uint32_t)(lg.xsimd_blur - x);
    uint32_t bxs[8], bys[8];
    int vals[8];
    asm volatile("s_waitcnt vmcnt(0)"
                 : "+v"(pat[0]), "+v"(pat[1]), "+v"(pat[2]), "+v"(pat[3]), "+v"(pat[4]), "+v"(pat[5]), "+v"(pat[6]),
                   "+v"(pat[7])::"memory");
    // one copy of the loop per wave-uniform tail case (no per-sample tail test when none)
    auto samples = [&](auto tailC) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        // R = (fma(px, b, py * a), fma(px, a, py * -b)) with px / py splat from the loaded pair
        // by op_sel (no copies): v_pk_mul_f32 takes py (the high half) for both lanes, v_pk_fma_f32
        // px (the low half) for both
        f32x2v R;
        asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,0] op_sel_hi:[1,1]\n\t"
            "v_pk_fma_f32 %0, %1, %3, %0 op_sel:[0,0,0] op_sel_hi:[0,1,1]"
            : "=&v"(R)
            : "v"(pat[q]), "v"(rA), "v"(rB));
        // (the magic add per element: this compiler turns a <2 x float> add of a splat literal
        // into the low lane's sum copied to both lanes)
        const uint32_t by = __builtin_bit_cast(uint32_t, R.x + 12582930.0f);
        const uint32_t bx = __builtin_bit_cast(uint32_t, R.y + 12582930.0f);
        bxs[q] = bx;
        bys[q] = by;
        // byte offset (by >> 1) * 224 + 4 bx: v_lshl_add_u32 + v_mad_u32_u24 (the compiler's
        // mul / shift / add3 was one more)
        uint32_t hoff;
        asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(hoff) : "v"(by >> 1), "v"(4u * OD_HN), "v"((bx << 2) + hb));
        const uint32_t* hq = (const uint32_t*)(s_buf[0] + hoff);
        // odd r0: the first pair starts one row early (taps shifted by one u16 lane)
        const uint32_t om = (uint32_t)__builtin_amdgcn_sbfe((int)by, 0, 1);
        const uint32_t t0 = bfi(om, tO0, tE0), t1 = bfi(om, tO1, tE1);
        const uint32_t t2 = bfi(om, tO2, tE2), t3 = bfi(om, tO3, tE3);
        const uint32_t T = dot2u(hq[3 * OD_HN], t3, dot2u(hq[2 * OD_HN], t2, dot2u(hq[OD_HN], t1, dot2u(hq[0], t0, 0u))));
        vals[q] = (int)blur_round(T, decltype(tailC)::value && bx >= thr);
    }
    };
    if (tailAny)
        samples(std::true_type{});
    else
        samples(std::false_type{});
    if (edge) {  // samples outside the ROI read the padded level itself (the window is overlaid)
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int X = x + (int)(bxs[q] - kMagic) - 18, Y = y + (int)(bys[q] - kMagic) - 18;
            if (X < 0 || X >= lg.w || Y < 0 || Y >= lg.h)
                vals[q] = pyr[lg.base + (long long)b * lg.fstride + (long long)(Y + EDGE) * lg.pitch + (X + EDGE)];
        }
    }
    int nib = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) nib |= (vals[2 * q] < vals[2 * q + 1]) << q;
    const int other = lane_xor1(nib);
    const uint32_t kslot = fslot + (uint32_t)(before + idx);
    if ((lane & 1) == 0) desc[kslot * 32u + (uint32_t)(lane >> 1)] = (uint8_t)(nib | (other << 4));
    if (lane == 0) {
        orb_keypoint_t kp;
        kp.x = l == 0 ? (float)x : (float)x * lg.scale;
        kp.y = l == 0 ? (float)y : (float)y * lg.scale;
        kp.size = lg.size;
        kp.angle = angle;
        kp.response = lvlResp ? lvlResp[fslot + (uint32_t)k] : (float)score;
        kp.octave = l;
        kp.class_id = -1;
        kps[kslot] = kp;
    }
}

// The descriptor image of one level (blurred ROI + raw border), over level coordinates
// [-3, ringX1) x [-3, ringY1), by the same row / column passes and rounding as k_orient_desc:
// test hook behind orb_debug_blur_image (not on the product path).  One thread per pixel.
__global__ void __launch_bounds__(256) k_debug_desc_image(const uint8_t* __restrict__ pyr, LevelGeom lg, int b,
                                                          uint8_t* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int W = lg.w + 2 * EDGE;
    const int X = i % W - EDGE, Y = i / W - EDGE;
    if (Y + EDGE >= lg.h + 2 * EDGE) return;
    const uint8_t* P = pyr + lg.base + (long long)b * lg.fstride;
    uint32_t v = P[(long long)(Y + EDGE) * lg.pitch + X + EDGE];
    if (X >= 0 && X < lg.w && Y >= 0 && Y < lg.h) {
        uint32_t T = 0;
        const int kk[7] = {18, 34, 49, 55, 49, 34, 18};
        for (int j = 0; j < 7; ++j) {
            uint32_t H = 0;
            for (int q = 0; q < 7; ++q) H += kk[q] * P[(long long)(Y + j - 3 + EDGE) * lg.pitch + X + q - 3 + EDGE];
            T += kk[j] * H;
        }
        v = blur_round(T, X >= lg.xsimd_blur);
    }
    out[i] = (uint8_t)v;
}

// ======================================================================================
// host side
// ======================================================================================
namespace {

inline int cvRoundH(double v) { return (int)lrint(v); }
inline short satS16(int v) { return (short)std::min(std::max(v, -32768), 32767); }

// OpenCV 2.4 getGaussianKernel(7, 2, CV_32F) -> convertTo(CV_32S, 256).
void gaussian_taps7(int* k7) {
    double scale2X = -0.5 / (2.0 * 2.0), sum = 0;
    float cf[7];
    for (int i = 0; i < 7; ++i) {
        double x = i - 3.0;
        cf[i] = (float)std::exp(scale2X * x * x);
        sum += cf[i];
    }
    sum = 1. / sum;
    for (int i = 0; i < 7; ++i) cf[i] = (float)(cf[i] * sum);
    for (int i = 0; i < 7; ++i) k7[i] = cvRoundH(cf[i] * 256.0f);
}

}  // namespace

struct orb_extractor {
    int nfeatures = 0;
    double scaleFactor = 1.2;  // double member, as in the reference (ORBextractor.h:62)
    int nlevels = 0, scoreType = 1, fastTh = 20, device = 0, maxBatch = 1;
    std::vector<float> mvScaleFactor, mvInvScaleFactor;
    std::vector<int> nDesired;
    int umax[16] = {};
    int kpCap = 0;
    hipStream_t stream = nullptr;      // the handle's own stream (host-buffer entry points)
    hipStream_t lastStream = nullptr;  // stream of the last launch on this handle's workspace
    bool lastValid = false;            // lastStream names a stream that ran a launch
    hipEvent_t evOrder = nullptr;      // orders a launch after the previous one on another stream
    int pyrBatch = 0;                  // frames whose pyramid phase 1 left in the workspace
    // geometry of the current frame size
    int W = 0, H = 0;
    Geom g{};
    int fastCl = FT_CL;  // orb_debug_set_fast_corner_list
    std::vector<CellGeom> cells;
    std::vector<int> rtab;
    size_t listLds = 0;  // k_select: the survivor lists
    size_t cellLds = 0;  // k_rerun: a FAST(7) re-run's LDS (largest cell)
    size_t resizeLds[ORB_MAX_LEVELS] = {}, resizeLdsS[ORB_MAX_LEVELS] = {};
    int resizeTail = 0;           // first level of k_pyr_resize_tail (nlevels: none)
    int tailBufA = 0, tailBufB = 0;
    size_t tailLds = 0;
    // k_pyr_stream plan (build_stream_plan); streamOk false: per-level launches only
    bool streamOk = false;
    StreamGeom sgeom{};
    size_t streamLds = 0;
    int streamK0 = 0;
    std::vector<StreamLevel> streamLv;  // host copy of d_slv (orb_debug_pyramid_plan_levels)
    std::vector<int> streamCap;         // ring rows of levels 0 .. L-2
    uint32_t* d_scol = nullptr;
    uint4* d_srows = nullptr;
    StreamLevel* d_slv = nullptr;
    uint32_t* d_srounds = nullptr;
    // device workspace
    uint8_t* d_pyr = nullptr;
    size_t pyrAlloc = 0;  // bytes of d_pyr (orb_debug_fill_pyramid)
    FastTile* d_tiles = nullptr;
    int nTiles = 0;
    uint32_t* d_cand = nullptr;
    int* d_cellCount = nullptr;
    uint32_t* d_cand2 = nullptr;  // k_select scratch when a level's survivors exceed its LDS
    uint32_t* d_lvl = nullptr;
    int* d_lvlCount = nullptr;
    int2* d_lvlInfo = nullptr;     // [frame][ORB_MAX_LEVELS] (first output slot, count): k_select's last WG
    int* d_selDone = nullptr;      // [frame] k_select workgroups done (self-resetting, zero between launches)
    uint8_t* d_slotLvl = nullptr;  // keypoint slot -> level (kpCap bytes, padded to a dword)
    uint64_t* d_candH = nullptr;  // HARRIS_SCORE: (response, record) scratch when a level exceeds LDS
    float* d_lvlResp = nullptr;   // HARRIS_SCORE: response of every kept keypoint
    float harrisScale4 = 0.f;
    int* d_rtab = nullptr;
    CellGeom* d_cells = nullptr;
    // per-stage HIP-event timing (orb_profile_*): stage k brackets its kernel(s) on the launch stream
    static constexpr int kStages = 5;
    // phases run by orb_extract_batch_device (the other entry points always run both):
    // bit 0 = pyramid (stages 0-1), bit 1 = detection, selection and descriptors (stages 2-4,
    // reading the pyramid bit 0 left in the workspace)
    unsigned phaseMask = 3u;
    bool pyrLegacy = false;        // orb_debug_set_pyramid_path(1): per-level launches at every batch size
    bool pyrStreamAlways = false;  // orb_debug_set_pyramid_path(2): k_pyr_stream at every batch size
    bool prof = false;
    unsigned profMask = 0;           // stages that record events (bit k = stage k)
    std::vector<hipEvent_t> evPool;  // 2 per stage per launch, recycled after each read
    std::vector<std::pair<int, int>> evPending;  // (stage, index of the start event)
    double stageMs[kStages] = {};
    long long stageLaunches[kStages] = {};
    int evNext = 0;
    // staging for host-buffer entry points
    uint8_t* d_img = nullptr;
    uint8_t* d_imgColor = nullptr;  // orb_extract_color's interleaved frame
    size_t imgColorCap = 0;
    // one device block: counts (maxBatch, padded to 256 B) | keypoints | descriptors, so a
    // single-frame download of the count and frame 0's keypoints is one contiguous copy
    uint8_t* d_out = nullptr;
    orb_keypoint_t* d_kps = nullptr;
    uint8_t* d_desc = nullptr;
    int* d_counts = nullptr;
    size_t countsPad = 0;
    // pinned host staging of the single-frame host entry points (orb_extract, orb_extract_color):
    // frame (W x H x up to 4 channels) | count + keypoints | descriptors, mirroring d_out, so the
    // uploads and downloads are DMA from page-locked memory and nothing is allocated per call
    uint8_t* h_pin = nullptr;
    size_t pinImg = 0;

    void free_events() {
        for (auto e : evPool) hipEventDestroy(e);
        evPool.clear();
        evPending.clear();
        evNext = 0;
    }

    void free_ws() {
        hipFree(d_pyr);
        hipFree(d_tiles);
        hipFree(d_cand);
        hipFree(d_cellCount);
        hipFree(d_cand2);
        hipFree(d_lvl);
        hipFree(d_lvlCount);
        hipFree(d_lvlInfo);
        hipFree(d_selDone);
        hipFree(d_slotLvl);
        hipFree(d_candH);
        hipFree(d_lvlResp);
        hipFree(d_rtab);
        hipFree(d_cells);
        hipFree(d_img);
        hipFree(d_imgColor);
        hipFree(d_out);
        hipFree(d_scol);
        hipFree(d_srows);
        hipFree(d_slv);
        hipFree(d_srounds);
        if (h_pin) (void)hipHostFree(h_pin);
        d_scol = nullptr;
        d_srows = nullptr;
        d_slv = nullptr;
        d_srounds = nullptr;
        streamOk = false;
        d_pyr = nullptr;
        pyrAlloc = 0;
        d_tiles = nullptr;
        nTiles = 0;
        d_cand = nullptr;
        d_cellCount = nullptr;
        d_cand2 = nullptr;
        d_lvl = nullptr;
        d_lvlCount = nullptr;
        d_lvlInfo = nullptr;
        d_selDone = nullptr;
        d_slotLvl = nullptr;
        d_candH = nullptr;
        d_lvlResp = nullptr;
        d_rtab = nullptr;
        d_cells = nullptr;
        d_img = nullptr;
        d_imgColor = nullptr;
        imgColorCap = 0;
        d_out = nullptr;
        d_kps = nullptr;
        d_desc = nullptr;
        d_counts = nullptr;
        h_pin = nullptr;
        pinImg = 0;
        W = H = 0;
        pyrBatch = 0;
    }

    // ORBextractor ctor arithmetic (ORBextractor.cc:462-510)
    void init_params() {
        mvScaleFactor.assign(nlevels, 1.f);
        for (int i = 1; i < nlevels; ++i) mvScaleFactor[i] = (float)(mvScaleFactor[i - 1] * scaleFactor);
        float invScaleFactor = (float)(1.0f / scaleFactor);
        mvInvScaleFactor.assign(nlevels, 1.f);
        for (int i = 1; i < nlevels; ++i) mvInvScaleFactor[i] = mvInvScaleFactor[i - 1] * invScaleFactor;
        nDesired.assign(nlevels, 0);
        float factor = (float)(1.0 / scaleFactor);
        float nd = nfeatures * (1 - factor) / (1 - (float)std::pow((double)factor, (double)nlevels));
        int sum = 0;
        for (int l = 0; l < nlevels - 1; ++l) {
            nDesired[l] = cvRoundH(nd);
            sum += nDesired[l];
            nd *= factor;
        }
        nDesired[nlevels - 1] = std::max(nfeatures - sum, 0);
        kpCap = 0;
        for (int n : nDesired) kpCap += n;
        int vmax = (int)std::floor(15 * std::sqrt(2.f) / 2 + 1), vmin = (int)std::ceil(15 * std::sqrt(2.f) / 2);
        for (int v = 0; v <= vmax; ++v) umax[v] = cvRoundH(std::sqrt(225.0 - v * v));
        for (int v = 15, v0 = 0; v >= vmin; --v) {
            while (umax[v0] == umax[v0 + 1]) ++v0;
            umax[v] = v0;
            ++v0;
        }
    }

    // Per-frame-size geometry: level sizes, cell grids, resize tables, workspace.
    int build_geometry(int w0, int h0) {
        free_ws();
        Geom G{};
        G.L = nlevels;
        G.fastTh = std::min(std::max(fastTh, 0), 255);
        G.fastCl = fastCl;
        G.scoreType = scoreType;
        int k7[7];
        gaussian_taps7(k7);
        for (int i = 0; i < 4; ++i) G.taps[i] = k7[3 + i];
        if (G.taps[0] != 55 || G.taps[1] != 49 || G.taps[2] != 34 || G.taps[3] != 18)
            return orb_internal_set_error(ORB_EINVAL,
                                          "Gaussian taps differ from the kernel's constants (c_rowB, GP_*)");
        for (int v = 0; v < 16; ++v) G.umax[v] = umax[v];
        G.umaxNib = 0;
        for (int v = 0; v < 16; ++v) G.umaxNib |= (unsigned long long)umax[v] << (4 * v);
        std::vector<CellGeom> cl;
        cellLds = 0;
        std::vector<int> rt;
        long long pyrBytes = 0;
        int cand = 0, kpBase = 0;
        for (int l = 0; l < nlevels; ++l) {
            LevelGeom& lg = G.lv[l];
            float sc = mvInvScaleFactor[l];
            lg.w = cvRoundH((float)w0 * sc);
            lg.h = cvRoundH((float)h0 * sc);
            if (lg.w < 1 || lg.h < 1 || lg.w >= 4096 || lg.h >= 4096)
                return orb_internal_set_error(ORB_ENOTSUP, "level size out of the supported range [1, 4095]");
            lg.pitch = (lg.w + 2 * orbdev::EDGE + 15) & ~15;
            lg.ph = lg.h + 2 * orbdev::EDGE;
            lg.fstride = (long long)lg.pitch * lg.ph;
            lg.base = pyrBytes;
            pyrBytes += lg.fstride * maxBatch;
            lg.scale = mvScaleFactor[l];
            lg.size = (float)(int)(31 * mvScaleFactor[l]);
            lg.xsimd_blur = (lg.w / 4) * 4;
            lg.nDesired = nDesired[l];
            lg.kpBase = kpBase;
            kpBase += nDesired[l];
        }
        // cell grid (ORBextractor.cc:527-597)
        const float imageRatio = (float)G.lv[0].w / G.lv[0].h;
        for (int l = 0; l < nlevels; ++l) {
            LevelGeom& lg = G.lv[l];
            const int nD = nDesired[l];
            const int levelCols = (int)std::sqrt((float)nD / (5 * imageRatio));
            const int levelRows = (int)(imageRatio * levelCols);
            if (levelCols <= 0 || levelRows <= 0)
                return orb_internal_set_error(ORB_ENOTSUP,
                                              "level " + std::to_string(l) + " has an empty cell grid (the reference "
                                              "divides by zero here)");
            if (levelCols * levelRows > ORB_MAX_CELLS_PER_LEVEL)
                return orb_internal_set_error(ORB_ENOTSUP, "more than 256 cells per level");
            const int maxBX = lg.w - 16, maxBY = lg.h - 16;
            const int Wd = maxBX - 16, Hd = maxBY - 16;
            const int cellW = (int)std::ceil((float)Wd / levelCols);
            const int cellH = (int)std::ceil((float)Hd / levelRows);
            const int nCells = levelRows * levelCols;
            lg.rows = levelRows;
            lg.cols = levelCols;
            lg.nfc = (int)std::ceil((float)nD / nCells);
            lg.cellW = cellW;
            lg.cellH = cellH;
            // (a 1-px cell's reciprocal 2^32 does not fit: 2^32 - 1, which k_fast applies to n + 1)
            lg.cellWm = cellW == 1 ? -1 : (int)(uint32_t)((0x100000000ull + cellW - 1) / (uint64_t)cellW);
            lg.cellHm = cellH == 1 ? -1 : (int)(uint32_t)((0x100000000ull + cellH - 1) / (uint64_t)cellH);
            lg.detX1 = std::max(maxBX, levelCols > 1 ? 16 + (levelCols - 1) * cellW : 0);
            lg.detY1 = std::max(maxBY, levelRows > 1 ? 16 + (levelRows - 1) * cellH : 0);
            // keypoints of non-last cells can sit past maxBorder (ORBextractor.cc:560-597); the
            // descriptor image must hold every sample they reach (|offset| <= 18)
            lg.ringX1 = std::max(lg.w + 3, lg.detX1 + 18);
            lg.ringY1 = std::max(lg.h + 3, lg.detY1 + 18);
            if (lg.ringX1 > lg.w + 12 || lg.ringY1 > lg.h + 12)
                return orb_internal_set_error(ORB_ENOTSUP,
                                              "cell grid too dense: rBRIEF samples leave the 16-px padding");
            if (cellW <= 0 || cellH <= 0) return orb_internal_set_error(ORB_ENOTSUP, "empty cell size");
            lg.cell0 = (int)cl.size();
            std::vector<int> iniXCol(levelCols, 0);
            float hY = cellH + 6;
            for (int i = 0; i < levelRows; ++i) {
                const float iniY = 16 + i * cellH - 3;
                bool rowSkip = false;
                if (i == levelRows - 1) {
                    hY = maxBY + 3 - iniY;
                    if (hY <= 0) rowSkip = true;
                }
                float hX = cellW + 6;
                for (int j = 0; j < levelCols; ++j) {
                    CellGeom c{};
                    c.level = l;
                    float iniX;
                    if (rowSkip) {
                        c.skipped = 1;
                    } else {
                        if (i == 0) {
                            iniX = 16 + j * cellW - 3;
                            iniXCol[j] = (int)iniX;
                        } else {
                            iniX = iniXCol[j];
                        }
                        if (j == levelCols - 1) {
                            hX = maxBX + 3 - iniX;
                            if (hX <= 0) c.skipped = 1;
                        }
                        if (!c.skipped) {
                            c.x0 = (int)iniX;
                            c.y0 = (int)iniY;
                            c.hx = (int)(iniX + hX) - c.x0;
                            c.hy = (int)(iniY + hY) - c.y0;
                            if (c.x0 < 0 || c.y0 < 0 || c.x0 + c.hx > lg.w || c.y0 + c.hy > lg.h)
                                return orb_internal_set_error(ORB_ENOTSUP,
                                                              "cell ROI outside the level (the reference asserts)");
                            int dw = c.hx - 6, dh = c.hy - 6;
                            c.cap = (dw > 0 && dh > 0) ? ((dw + 1) / 2) * ((dh + 1) / 2) : 0;
                            if (dw > 0 && dh > 0) cellLds = std::max(cellLds, rerun_lds(dw, dh));
                        }
                    }
                    cl.push_back(c);
                }
            }
            // uniform slot stride per level (k_fast computes a cell's slots arithmetically)
            int capMax = 0;
            for (size_t i = lg.cell0; i < cl.size(); ++i) capMax = std::max(capMax, cl[i].cap);
            lg.candBase = cand;
            lg.capMax = capMax;
            for (size_t i = lg.cell0; i < cl.size(); ++i) cl[i].candOff = cand + (int)(i - lg.cell0) * capMax;
            cand += (int)(cl.size() - lg.cell0) * capMax;
        }
        G.selCap = select_cap(w0, h0);
        listLds = (size_t)(scoreType == ORB_HARRIS_SCORE ? 4 : 2) * G.selCap * 4;
        if (std::max(cellLds, listLds) > 150 * 1024)
            return orb_internal_set_error(ORB_ENOTSUP, "FAST cell larger than the LDS budget");
        // resize tables, l >= 1
        for (int l = 1; l < nlevels; ++l) {
            LevelGeom& lg = G.lv[l];
            const LevelGeom& ls = G.lv[l - 1];
            const int sw = ls.w, sh = ls.h, dw = lg.w, dh = lg.h;
            double inv_sx = (double)dw / sw, inv_sy = (double)dh / sh;
            double scale_x = 1. / inv_sx, scale_y = 1. / inv_sy;
            int isx = cvRoundH(scale_x), isy = cvRoundH(scale_y);
            if (std::abs(scale_x - isx) < 2.220446049250313e-16 && std::abs(scale_y - isy) < 2.220446049250313e-16 &&
                isx == 2 && isy == 2)
                return orb_internal_set_error(ORB_ENOTSUP, "exact 2x level step (OpenCV switches to INTER_AREA)");
            lg.rtab = (int)rt.size();
            std::vector<int> xofs(dw), alpha(dw), yofs(dh), beta(dh);
            int xmax = dw;
            for (int dx = 0; dx < dw; ++dx) {
                float fx = (float)((dx + 0.5) * scale_x - 0.5);
                int sx = (int)std::floor(fx);
                fx -= sx;
                if (sx < 0) fx = 0, sx = 0;
                if (sx + 1 >= sw) {
                    xmax = std::min(xmax, dx);
                    if (sx >= sw - 1) fx = 0, sx = sw - 1;
                }
                xofs[dx] = sx;
                short a0 = satS16(cvRoundH((1.f - fx) * 2048)), a1 = satS16(cvRoundH(fx * 2048));
                alpha[dx] = (int)(uint16_t)a0 | ((int)(uint16_t)a1 << 16);
            }
            for (int dy = 0; dy < dh; ++dy) {
                float fy = (float)((dy + 0.5) * scale_y - 0.5);
                int sy = (int)std::floor(fy);
                fy -= sy;
                yofs[dy] = sy;
                short b0 = satS16(cvRoundH((1.f - fy) * 2048)), b1 = satS16(cvRoundH(fy * 2048));
                beta[dy] = (int)(uint16_t)b0 | ((int)(uint16_t)b1 << 16);
            }
            for (int dx = 0; dx < dw; ++dx) {  // k_pyr_resize's no-saturation premise
                const int c0 = alpha[dx] & 0xFFFF, c1 = (alpha[dx] >> 16) & 0xFFFF;
                if ((short)c0 < 0 || (short)c1 < 0 || c0 + c1 > 2050)
                    return orb_internal_set_error(ORB_ENOTSUP, "resize coefficient outside [0, 2050]");
            }
            for (int dy = 0; dy < dh; ++dy) {
                const int c0 = beta[dy] & 0xFFFF, c1 = (beta[dy] >> 16) & 0xFFFF;
                if ((short)c0 < 0 || (short)c1 < 0 || c0 + c1 > 2050)
                    return orb_internal_set_error(ORB_ENOTSUP, "resize coefficient outside [0, 2050]");
            }
            int xs = 0;
            while (xs <= dw - 16) xs += 16;
            while (xs < dw - 4) xs += 4;
            lg.xs_resize = xs;
            lg.xmax = xmax;
            rt.insert(rt.end(), xofs.begin(), xofs.end());
            rt.insert(rt.end(), alpha.begin(), alpha.end());
            rt.insert(rt.end(), yofs.begin(), yofs.end());
            rt.insert(rt.end(), beta.begin(), beta.end());
            // source rectangle of every RZ_TW x TH tile of the padded level (k_pyr_resize), for
            // the two tile heights
            auto tiles = [&](int TH, int& off, size_t& ldsOut) {
                const int tx = (lg.pitch + RZ_TW - 1) / RZ_TW, ty = (lg.ph + TH - 1) / TH;
                off = (int)rt.size();
                size_t lds = 0;
                for (int y = 0; y < ty; ++y)
                    for (int x = 0; x < tx; ++x) {
                        int c0 = INT32_MAX, c1 = -1, r0 = INT32_MAX, r1 = -1;
                        for (int px = x * RZ_TW; px < std::min((x + 1) * RZ_TW, lg.pitch); ++px) {
                            const int lx = orbdev::reflect101(std::min(px, dw + 31) - 16, dw);
                            const int sx = xofs[lx];
                            const int sx1 = (lx < xmax && (alpha[lx] >> 16) != 0) ? sx + 1 : sx;
                            c0 = std::min(c0, sx);
                            c1 = std::max(c1, sx1);
                        }
                        for (int py = y * TH; py < std::min((y + 1) * TH, lg.ph); ++py) {
                            const int ly = orbdev::reflect101(py - 16, dh);
                            r0 = std::min(r0, std::min(std::max(yofs[ly], 0), sh - 1));
                            r1 = std::max(r1, std::min(std::max(yofs[ly] + 1, 0), sh - 1));
                        }
                        const int cs = c0 & ~15, units = ((c1 - cs) >> 4) + 1, nr = r1 - r0 + 1;
                        rt.push_back(cs);
                        rt.push_back(units);
                        rt.push_back(r0);
                        rt.push_back(nr);
                        lds = std::max(lds, (size_t)units * 16 * nr);
                    }
                ldsOut = lds;
            };
            tiles(RZ_TH, lg.rtile, resizeLds[l]);
            tiles(RZ_THS, lg.rtileS, resizeLdsS[l]);
            if (resizeLds[l] > 96 * 1024)
                return orb_internal_set_error(ORB_ENOTSUP, "scale factor too large for the resize tile");
        }
        // the fused small-level tail: the first level from which every later level's source
        // ROI (ping-pong A / B) plus the staged tables fit the CU's LDS
        resizeTail = nlevels;
        for (int l = 1; l + 1 < nlevels; ++l) {
            auto roi = [&](int k) { return k + 1 < nlevels ? (size_t)G.lv[k].w * G.lv[k].h : (size_t)0; };
            const size_t a = (roi(l) + 15) & ~(size_t)15, bsz = (roi(l + 1) + 15) & ~(size_t)15;
            const size_t need = a + bsz + (size_t)8 * (G.lv[l].w + G.lv[l].h);
            if (need <= (size_t)RT_LDS_MAX) {
                resizeTail = l;
                tailBufA = (int)a;
                tailBufB = (int)bsz;
                tailLds = need;
                break;
            }
        }
        G.nCells = (int)cl.size();
        G.candPerFrame = cand;
        G.kpCap = kpCap;
        {  // k_orient_desc's grid is ((kpCap + slots - 1) / slots, B): bid / gridDim.x by multiply-high
            const unsigned long long gx = (unsigned long long)(std::max(kpCap, 1) + OD_WAVES - 1) / OD_WAVES;
            // and its per-slot offsets are 32-bit: descriptor bytes of the whole batch < 2^32
            if ((unsigned long long)std::max(kpCap, 1) * (unsigned long long)maxBatch * 32ull >= (1ull << 32))
                return orb_internal_set_error(ORB_ENOTSUP,
                                              "max_batch x keypoint capacity too large (descriptor bytes >= 4 GiB)");
            G.odDivMagic = (uint32_t)(((1ull << 32) + gx - 1) / gx);
            if (gx * gx * (unsigned long long)maxBatch >= (1ull << 32))
                return orb_internal_set_error(ORB_ENOTSUP, "keypoint grid too large for k_orient_desc's block decode");
        }
        // workspace
        // + slack: k_orient_desc's 64-byte window rows and k_rerun's 16-B ROI units may over-read
        // the last row's pitch
        ORB_HIPCHK(hipMalloc(&d_pyr, (size_t)pyrBytes + 256));
        pyrAlloc = (size_t)pyrBytes + 256;
        // k_fast tiles over each level's detection region: the width split evenly into
        // ceil(width / 256) tiles of a multiple of 4 columns, as many rows as the LDS budgets
        // (staged tile, strength plane) and the 16-bit queue codes allow
        std::vector<FastTile> tl;
        auto rcp = [](int d) { return (uint32_t)((0x100000000ull + (uint64_t)d - 1) / (uint64_t)d); };
        for (int l = 0; l < nlevels; ++l) {
            const int detW = G.lv[l].detX1 - orbdev::EDGE;
            const int nx = (detW + FT_TW_MAX - 1) / FT_TW_MAX;
            int tw4 = std::max(2, ((detW + 3) / 4 + nx - 1) / nx);
            tw4 = (tw4 + 1) & ~1;  // tiles of a multiple of 8 columns: every x0 = 0 mod 8
            const int TW = 4 * tw4;
            for (int x0 = orbdev::EDGE; x0 < G.lv[l].detX1; x0 += TW) {
                // first staged byte at sx = 16 + (x0 mod 16) in {16, 24}: the compass groups' dword
                // pairs (sx - 8 + 8 kp) 8-B aligned, and 16 bytes left of the tile for the left pair
                const int sx = 16 + (x0 & 15);
                const int sp = (sx + TW + 8 + 15) & ~15, spw = TW + 8;
                const int thMax = std::min({FT_IN_BYTES / sp - 8, FT_S_BYTES / spw - 2, 126, 4095 / (tw4 + 2) - 2});
                if (thMax < 1 || sp > 288) return orb_internal_set_error(ORB_EINVAL, "k_fast tile geometry");
                for (int y0 = orbdev::EDGE; y0 < G.lv[l].detY1; y0 += thMax) {
                    const int th = std::min(thMax, G.lv[l].detY1 - y0);
                    tl.push_back(FastTile{l, x0, y0, tw4, th, sp, sx, rcp(tw4 + 2), rcp(tw4), rcp(sp >> 4)});
                }
            }
        }
        ORB_HIPCHK(hipMalloc(&d_tiles, tl.size() * sizeof(FastTile)));
        ORB_HIPCHK(hipMemcpy(d_tiles, tl.data(), tl.size() * sizeof(FastTile), hipMemcpyHostToDevice));
        nTiles = (int)tl.size();

        ORB_HIPCHK(hipMalloc(&d_cand, (size_t)std::max(cand, 1) * maxBatch * 4));
        ORB_HIPCHK(hipMalloc(&d_cellCount, (size_t)G.nCells * maxBatch * 4));
        ORB_HIPCHK(hipMalloc(&d_cand2, (size_t)std::max(cand, 1) * maxBatch * 4));
        ORB_HIPCHK(hipMalloc(&d_lvl, (size_t)std::max(kpCap, 1) * maxBatch * 4));
        ORB_HIPCHK(hipMalloc(&d_lvlCount, (size_t)nlevels * maxBatch * 4));
        ORB_HIPCHK(hipMalloc(&d_lvlInfo, (size_t)ORB_MAX_LEVELS * maxBatch * sizeof(int2)));
        ORB_HIPCHK(hipMalloc(&d_selDone, (size_t)maxBatch * sizeof(int)));
        ORB_HIPCHK(hipMemset(d_selDone, 0, (size_t)maxBatch * sizeof(int)));
        {
            std::vector<uint8_t> sl(((size_t)std::max(kpCap, 1) + 3) & ~(size_t)3, 0);
            for (int l = 0; l < nlevels; ++l)
                for (int k = 0; k < G.lv[l].nDesired; ++k) sl[(size_t)G.lv[l].kpBase + k] = (uint8_t)l;
            ORB_HIPCHK(hipMalloc(&d_slotLvl, sl.size()));
            ORB_HIPCHK(hipMemcpy(d_slotLvl, sl.data(), sl.size(), hipMemcpyHostToDevice));
        }
        if (scoreType == ORB_HARRIS_SCORE) {
            ORB_HIPCHK(hipMalloc(&d_candH, (size_t)std::max(cand, 1) * maxBatch * 8));
            ORB_HIPCHK(hipMalloc(&d_lvlResp, (size_t)std::max(kpCap, 1) * maxBatch * 4));
        }
        ORB_HIPCHK(hipMalloc(&d_rtab, std::max<size_t>(rt.size(), 1) * 4));
        ORB_HIPCHK(hipMalloc(&d_cells, cl.size() * sizeof(CellGeom)));
        if (!rt.empty()) ORB_HIPCHK(hipMemcpy(d_rtab, rt.data(), rt.size() * 4, hipMemcpyHostToDevice));
        ORB_HIPCHK(hipMemcpy(d_cells, cl.data(), cl.size() * sizeof(CellGeom), hipMemcpyHostToDevice));
        if (int r = build_stream_plan(G, rt)) return r;
        g = G;
        cells = std::move(cl);
        rtab = std::move(rt);
        W = w0;
        H = h0;
        return ORB_OK;
    }

    // k_pyr_stream's plan: the round schedule (greedy: level l computes every row whose source
    // rows of level l-1 are in its ring), the ring capacity of each level (max over rounds of
    // newest row written - oldest row read + 1), ring slots, per-row and per-quad tables.  K0
    // (level-0 rows per round) is the largest whose rings fit PS_LDS_TARGET.  Frames with a
    // level under 17 px (multiple reflections) or rings that never fit keep the per-level path.
    int build_stream_plan(const Geom& G, const std::vector<int>& rt) {
        streamOk = false;
        const int L = nlevels;
        if (L < 2) return ORB_OK;
        for (int l = 0; l < L; ++l)
            if (G.lv[l].w < 17 || G.lv[l].h < 17) return ORB_OK;
        const int u0 = (G.lv[0].w + 15) / 16;
        std::vector<std::vector<int>> s0(L), s1(L);
        for (int l = 1; l < L; ++l) {
            const LevelGeom& lg = G.lv[l];
            const int hs = G.lv[l - 1].h;
            const int* yofs = rt.data() + lg.rtab + 2 * lg.w;
            s0[l].resize(lg.h);
            s1[l].resize(lg.h);
            for (int dy = 0; dy < lg.h; ++dy) {
                s0[l][dy] = std::min(std::max(yofs[dy], 0), hs - 1);
                s1[l][dy] = std::min(std::max(yofs[dy] + 1, 0), hs - 1);
            }
        }
        auto ringPitch = [&](int l) { return (G.lv[l].w + 15) & ~15; };
        auto nqOf = [&](int l) { return l == 0 ? G.lv[0].pitch / 16 : G.lv[l].pitch / 4; };
        // column words (LDS-resident): one u32 per padded column of levels >= 1
        // sx | a1 << 12 | (a0 - 2047 + a1) << 24 | simd << 26 | live << 27
        std::vector<uint32_t> cw;
        std::vector<int> colQuad(L, 0);
        for (int l = 1; l < L; ++l) {
            const LevelGeom& lg = G.lv[l];
            const int* xofs = rt.data() + lg.rtab;
            const int* alpha = xofs + lg.w;
            colQuad[l] = (int)(cw.size() / 4);
            for (int px = 0; px < 4 * nqOf(l); ++px) {
                const int lx = orbdev::reflect101(std::min(px, lg.w + 2 * orbdev::EDGE - 1) - orbdev::EDGE, lg.w);
                const int sx = xofs[lx];
                const int a0 = lx < lg.xmax ? (alpha[lx] & 0xFFFF) : 2048;
                const int a1 = lx < lg.xmax ? ((alpha[lx] >> 16) & 0xFFFF) : 0;
                const int d = a0 - 2047 + a1;
                if (sx < 0 || sx > 0xFFF || a1 > 0xFFF || d < 0 || d > 3) return ORB_OK;  // not encodable
                uint32_t c = (uint32_t)sx | ((uint32_t)a1 << 12) | ((uint32_t)d << 24);
                if (lx < lg.xs_resize) c |= 1u << 26;
                if (px < lg.w + 2 * orbdev::EDGE) c |= 1u << 27;
                cw.push_back(c);
            }
        }
        const size_t colBytes = (cw.size() * 4 + 15) & ~(size_t)15;
        std::vector<uint32_t> rounds;
        std::vector<int> cap;
        std::vector<std::vector<int>> plan;  // per round: lo, cnt per level
        int K0 = 0, maxEnt = 0;
        size_t lds = 0;
        for (int k0 : {32, 24, 16, 12, 8, 6, 4, 2}) {
            if (k0 * u0 > PS_NPF * 64 * PS_LOADERS) continue;
            std::vector<int> next(L, 0), cp(L, 0);
            std::vector<std::vector<int>> pl;
            int me = 0;
            bool ok = true;
            for (int n = 0;; ++n) {
                bool done = true;
                for (int l = 0; l < L; ++l) done = done && next[l] >= G.lv[l].h;
                if (done) break;
                if (n > 65536) {
                    ok = false;
                    break;
                }
                std::vector<int> lo(L), cnt(L);
                lo[0] = next[0];
                cnt[0] = std::min(k0, G.lv[0].h - next[0]);
                const int avail0 = next[0] + cnt[0];
                for (int l = 1; l < L; ++l) {
                    const int srcAvail = l == 1 ? avail0 : next[l - 1];
                    int d = next[l];
                    while (d < G.lv[l].h && s1[l][d] < srcAvail) ++d;
                    lo[l] = next[l];
                    cnt[l] = d - next[l];
                }
                for (int l = 0; l + 1 < L; ++l) {
                    // level 0: the loaders store round n+1's rows during round n
                    const int newest = (l == 0 ? std::min(avail0 + k0, G.lv[0].h) : next[l] + cnt[l]) - 1;
                    int oldest = INT32_MAX;
                    if (l == 0 && cnt[0]) oldest = lo[0];
                    if (cnt[l + 1]) oldest = std::min(oldest, s0[l + 1][lo[l + 1]]);
                    if (oldest != INT32_MAX) cp[l] = std::max(cp[l], newest - oldest + 1);
                }
                std::vector<int> rec(2 * L);
                int ent = 0;
                for (int l = 0; l < L; ++l) {
                    rec[2 * l] = lo[l];
                    rec[2 * l + 1] = cnt[l];
                    ent += cnt[l];
                    next[l] += cnt[l];
                }
                me = std::max(me, ent);
                pl.push_back(std::move(rec));
            }
            if (!ok || me > PS_NPF * 64 * PS_LOADERS) continue;
            size_t bytes = 0;
            bool capOk = true;
            for (int l = 0; l + 1 < L; ++l) {
                cp[l] = std::min(std::max(cp[l], 1), G.lv[l].h);
                capOk = capOk && cp[l] <= 255;
                bytes += (size_t)cp[l] * ringPitch(l);
            }
            const int stride8 = (me + 1) & ~1;
            bytes += colBytes;
            if (capOk && bytes <= PS_LDS_TARGET) {
                K0 = k0;
                plan = std::move(pl);
                cap = std::move(cp);
                maxEnt = stride8;
                lds = bytes;
                break;
            }
        }
        if (!K0) return ORB_OK;
        std::vector<StreamLevel> lv(L);
        int ringOff = 0;
        for (int l = 0; l < L; ++l) {
            const LevelGeom& lg = G.lv[l];
            StreamLevel& s = lv[l];
            s.nq = nqOf(l);
            s.nqm = (uint32_t)((0x100000000ull + s.nq - 1) / (uint64_t)s.nq);
            s.ringPitch = ringPitch(l);
            s.ringOff = l + 1 < L ? ringOff : 0;
            if (l + 1 < L) ringOff += cap[l] * s.ringPitch;
            s.w = lg.w;
            s.h = lg.h;
            s.pitch = lg.pitch;
            s.base = lg.base;
            s.fstride = lg.fstride;
        }
        // waves per level: one each, then greedily to the level with the most work per wave
        // (level-0 units are copies: weighted 1/4), up to one wave per 64 column units
        if (L > PS_THREADS / 64 - PS_LOADERS) return ORB_OK;
        {
            std::vector<int> nw(L, 1);
            for (int left = PS_THREADS / 64 - PS_LOADERS - L; left > 0; --left) {
                int best = -1;
                double bw = 0;
                for (int l = 0; l < L; ++l) {
                    if (nw[l] * 64 >= lv[l].nq) continue;
                    const double wk = (double)lv[l].nq * G.lv[l].h * (l == 0 ? 0.25 : 1.0) / nw[l];
                    if (wk > bw) {
                        bw = wk;
                        best = l;
                    }
                }
                if (best < 0) break;
                ++nw[best];
            }
            int ws = PS_LOADERS;
            for (int l = 0; l < L; ++l) {
                lv[l].waveStart = ws;
                lv[l].nWaves = nw[l];
                ws += nw[l];
            }
        }
        const int colOff = ringOff;  // multiple of 16
        for (int l = 1; l < L; ++l) lv[l].colOff = colOff + 16 * colQuad[l];
        lv[0].colOff = 0;
        // rounds (L level words + the first entry) and the row entries in round order: per row
        // {source row 0, source row 1 (LDS addresses), b0 << 12, b1 << 12, own ring row (LDS
        //  address or ~0u), padded-row offset, top mirror offset, bottom mirror offset (~0u: none)}
        std::vector<uint32_t> ent;
        for (const auto& rec : plan) {
            int ne = 0;
            for (int l = 0; l < L; ++l) {
                if (rec[2 * l] > 0xFFF || rec[2 * l + 1] > 0x3F || ne > 0x3FFF) return ORB_OK;
                rounds.push_back((uint32_t)rec[2 * l] | ((uint32_t)rec[2 * l + 1] << 12) | ((uint32_t)ne << 18));
                ne += rec[2 * l + 1];
            }
            rounds.push_back((uint32_t)(ent.size() / 8));
            rounds.push_back((uint32_t)ne);
            for (int l = 0; l < L; ++l)
                for (int dy = rec[2 * l]; dy < rec[2 * l] + rec[2 * l + 1]; ++dy) {
                    const LevelGeom& lg = G.lv[l];
                    const uint32_t own =
                        l + 1 < L ? (uint32_t)(lv[l].ringOff + (dy % cap[l]) * lv[l].ringPitch) : 0xFFFFFFFFu;
                    const uint32_t main = (uint32_t)((dy + orbdev::EDGE) * lg.pitch);
                    const uint32_t top = dy >= 1 && dy <= orbdev::EDGE ? (uint32_t)((orbdev::EDGE - dy) * lg.pitch) : 0xFFFFFFFFu;
                    const uint32_t bot = dy >= lg.h - 17 && dy <= lg.h - 2 ? (uint32_t)((2 * lg.h + 14 - dy) * lg.pitch) : 0xFFFFFFFFu;
                    if (l == 0) {
                        ent.insert(ent.end(), {own, 0u, 0u, 0u, 0xFFFFFFFFu, main, top, bot});
                    } else {
                        const int cs = cap[l - 1];
                        const uint32_t beta = (uint32_t)rt[lg.rtab + 2 * lg.w + lg.h + dy];
                        const uint32_t a0 = (uint32_t)(lv[l - 1].ringOff + (s0[l][dy] % cs) * lv[l - 1].ringPitch);
                        const uint32_t a1 = (uint32_t)(lv[l - 1].ringOff + (s1[l][dy] % cs) * lv[l - 1].ringPitch);
                        ent.insert(ent.end(), {a0, a1, (beta & 0xFFFFu) << 12, (beta >> 16) << 12, own, main, top, bot});
                    }
                }
        }
        // the magic divisions are exact over every task index of every round
        for (int l = 0; l < L; ++l) {
            int maxCnt = 0;
            for (const auto& rec : plan) maxCnt = std::max(maxCnt, rec[2 * l + 1]);
            for (uint32_t i = 0; i < (uint32_t)(maxCnt * lv[l].nq); ++i)
                if ((uint32_t)(((uint64_t)i * lv[l].nqm) >> 32) != i / (uint32_t)lv[l].nq) return ORB_OK;
        }
        StreamGeom sg{};
        sg.L = L;
        sg.nRounds = (int)plan.size();
        sg.u0 = u0;
        sg.u0m = (uint32_t)((0x100000000ull + u0 - 1) / (uint64_t)u0);
        for (uint32_t i = 0; i < (uint32_t)(K0 * u0); ++i)
            if ((uint32_t)(((uint64_t)i * sg.u0m) >> 32) != i / (uint32_t)u0) return ORB_OK;
        sg.colWords = (int)cw.size();
        sg.colOff = colOff;
        sg.rowOff = colOff + (int)colBytes;
        sg.rowStride = maxEnt;
        sg.cap0 = cap[0];
        ORB_HIPCHK(hipMalloc(&d_scol, std::max<size_t>(cw.size(), 1) * 4));
        ORB_HIPCHK(hipMemcpy(d_scol, cw.data(), cw.size() * 4, hipMemcpyHostToDevice));
        ORB_HIPCHK(hipMalloc(&d_srows, ent.size() * 4));
        ORB_HIPCHK(hipMemcpy(d_srows, ent.data(), ent.size() * 4, hipMemcpyHostToDevice));
        ORB_HIPCHK(hipMalloc(&d_slv, L * sizeof(StreamLevel)));
        ORB_HIPCHK(hipMemcpy(d_slv, lv.data(), L * sizeof(StreamLevel), hipMemcpyHostToDevice));
        ORB_HIPCHK(hipMalloc(&d_srounds, rounds.size() * 4));
        ORB_HIPCHK(hipMemcpy(d_srounds, rounds.data(), rounds.size() * 4, hipMemcpyHostToDevice));
        sgeom = sg;
        streamLv = lv;
        streamCap = cap;
        streamLds = lds;
        streamK0 = K0;
        streamOk = true;
        return ORB_OK;
    }

    int ensure_staging() {
        if (d_img) return ORB_OK;
        ORB_HIPCHK(hipMalloc(&d_img, (size_t)W * H * maxBatch));
        const size_t cap = (size_t)std::max(kpCap, 1);
        countsPad = ((size_t)maxBatch * 4 + 255) & ~(size_t)255;
        const size_t kpsBytes = ((cap * maxBatch * sizeof(orb_keypoint_t)) + 255) & ~(size_t)255;
        ORB_HIPCHK(hipMalloc(&d_out, countsPad + kpsBytes + cap * maxBatch * 32));
        d_counts = (int*)d_out;
        d_kps = (orb_keypoint_t*)(d_out + countsPad);
        d_desc = d_out + countsPad + kpsBytes;
        return ORB_OK;
    }

    // single-frame pinned staging: [frame: pinImg][count + frame-0 keypoints: countsPad + kpCap*28][descriptors]
    int ensure_pinned(size_t frameBytes) {
        if (h_pin && frameBytes <= pinImg) return ORB_OK;
        if (h_pin) {
            ORB_HIPCHK(hipStreamSynchronize(stream));  // the previous call's copies are complete anyway
            (void)hipHostFree(h_pin);
            h_pin = nullptr;
            pinImg = 0;
        }
        const size_t img = (std::max(frameBytes, (size_t)W * H * 4) + 255) & ~(size_t)255;
        const size_t cap = (size_t)std::max(kpCap, 1);
        ORB_HIPCHK(hipHostMalloc((void**)&h_pin, img + countsPad + cap * (sizeof(orb_keypoint_t) + 32), 0));
        pinImg = img;
        return ORB_OK;
    }

    // host frame (rows at `stride`) -> pinned -> device at `dst` (tight rows of `row` bytes)
    int upload_frame(uint8_t* dst, const uint8_t* img, size_t row, int hgt, size_t stride) {
        if (int r = ensure_pinned(row * hgt)) return r;
        if (stride == row) {
            std::memcpy(h_pin, img, row * hgt);
        } else {
            for (int y = 0; y < hgt; ++y) std::memcpy(h_pin + row * y, img + stride * y, row);
        }
        ORB_HIPCHK(hipMemcpyAsync(dst, h_pin, row * hgt, hipMemcpyHostToDevice, stream));
        return ORB_OK;
    }

    // frame 0's count, keypoints and descriptors -> the caller's buffers (one stream sync)
    int download_frame0(orb_keypoint_t* kps_out, int kps_cap, uint8_t* desc_out, int* n_out) {
        const size_t cap = (size_t)std::max(kpCap, 1);
        uint8_t* pk = h_pin + pinImg;
        uint8_t* pd = pk + countsPad + cap * sizeof(orb_keypoint_t);
        ORB_HIPCHK(hipMemcpyAsync(pk, d_out, countsPad + cap * sizeof(orb_keypoint_t), hipMemcpyDeviceToHost, stream));
        ORB_HIPCHK(hipMemcpyAsync(pd, d_desc, cap * 32, hipMemcpyDeviceToHost, stream));
        ORB_HIPCHK(hipStreamSynchronize(stream));
        int n = 0;
        std::memcpy(&n, pk, 4);
        if (n > kps_cap) return orb_internal_set_error(ORB_ERANGE, "kps_cap smaller than the number of keypoints");
        std::memcpy(kps_out, pk + countsPad, (size_t)n * sizeof(orb_keypoint_t));
        std::memcpy(desc_out, pd, (size_t)n * 32);
        *n_out = n;
        return ORB_OK;
    }

    hipEvent_t next_event() {
        if (evNext == (int)evPool.size()) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) return nullptr;
            evPool.push_back(e);
        }
        return evPool[evNext++];
    }
    // stage_begin pushes one entry per bracketed stage; an entry whose events could not be
    // created is a sentinel (index -1) that stage_end and profile_collect skip
    void stage_begin(int stage, hipStream_t st) {
        if (!prof || !((profMask >> stage) & 1u)) return;
        int i = evNext;
        hipEvent_t a = next_event(), b = next_event();
        if (!a || !b || hipEventRecord(a, st) != hipSuccess) {
            evPending.push_back({stage, -1});
            return;
        }
        evPending.push_back({stage, i});
    }
    void stage_end(int stage, hipStream_t st) {
        if (!prof || !((profMask >> stage) & 1u) || evPending.empty()) return;
        const auto& pe = evPending.back();
        if (pe.first != stage || pe.second < 0) return;
        hipEventRecord(evPool[pe.second + 1], st);
    }
    int profile_collect() {
        for (auto& pe : evPending) {
            if (pe.second < 0) continue;
            ORB_HIPCHK(hipEventSynchronize(evPool[pe.second + 1]));
            float ms = 0.f;
            ORB_HIPCHK(hipEventElapsedTime(&ms, evPool[pe.second], evPool[pe.second + 1]));
            stageMs[pe.first] += ms;
            stageLaunches[pe.first] += 1;
        }
        evPending.clear();
        evNext = 0;
        return ORB_OK;
    }

    // Every launch on this handle's workspace is ordered after the previous one, whatever
    // stream either ran on: an event recorded on the previous stream is waited on by `st`
    // (device-side; the host never blocks).
    int order_after_last(hipStream_t st) {
        if (lastValid && lastStream != st) {
            ORB_HIPCHK(hipEventRecord(evOrder, lastStream));
            ORB_HIPCHK(hipStreamWaitEvent(st, evOrder, 0));
        }
        lastStream = st;
        lastValid = true;
        return ORB_OK;
    }
    // The workspace is about to be re-allocated: drain every stream that may still use it.
    int drain() {
        ORB_HIPCHK(hipStreamSynchronize(stream));
        if (lastValid) ORB_HIPCHK(hipStreamSynchronize(lastStream));
        return ORB_OK;
    }

    int launch(int B, const uint8_t* d_imgs, int stride, long long fpitch, orb_keypoint_t* kps, uint8_t* desc,
               int* counts, hipStream_t st, int cn = 1, int rgb = 0, unsigned phases = 3u) {
        if (!(phases & 1u) && B > pyrBatch)
            return orb_internal_set_error(ORB_EINVAL,
                                          "phase 2 without a phase-1 pyramid of this geometry for these frames");
        if (int r = order_after_last(st)) return r;
        if (prof && evNext > 4096) {  // bound the pool between reads
            int r = profile_collect();
            if (r) return r;
        }
        bool countsZeroed = false;  // k_pyr_stream zeroed k_fast's cell counters
        if ((phases & 1u) && cn == 1 && streamOk && (B >= KR_STREAM_BATCH || pyrStreamAlways) && !pyrLegacy) {
            // the whole pyramid in one streaming pass per frame (stage 0; stage 1 is empty)
            stage_begin(0, st);
            StreamGeom sg = sgeom;
            const uintptr_t al = (uintptr_t)d_imgs | (uintptr_t)stride | (uintptr_t)fpitch;
            sg.align = (al & 15u) == 0 ? 16 : (al & 3u) == 0 ? 4 : 1;
            orb_ilp_pyr_stream(B, streamLds, st, d_imgs, stride, fpitch, d_pyr, (const uint32_t*)d_scol,
                               (const uint4*)d_srows, (const StreamLevel*)d_slv, (const uint32_t*)d_srounds, sg,
                               (phases & 2u) ? d_cellCount : (int*)nullptr, g.nCells);
            countsZeroed = (phases & 2u) != 0;
            stage_end(0, st);
            pyrBatch = B;
        } else if (phases & 1u) {
        stage_begin(0, st);
        {
            const LevelGeom& lg = g.lv[0];
            dim3 grid((lg.pitch / 4 + 63) / 64, (lg.ph + 3) / 4, B);
            if (cn == 1)
                hipLaunchKernelGGL(k_pyr0, dim3(((lg.pitch >> 4) * lg.ph + 255) / 256, B), dim3(256), 0, st, d_imgs,
                                   stride, fpitch, d_pyr, g);
            else  // R2Y on the red channel, B2Y on the blue one
                hipLaunchKernelGGL(k_pyr0_color, grid, dim3(64, 4), 0, st, d_imgs, stride, fpitch, cn,
                                   rgb ? 4899 : 1868, rgb ? 1868 : 4899, d_pyr, g);
        }
        stage_end(0, st);
        stage_begin(1, st);
        // a few frames: one multi-workgroup launch per level (the tail kernel's one workgroup
        // per frame walks its levels serially, the latency floor of a single frame)
        const int tail = B < KR_TAIL_BATCH ? nlevels : resizeTail;
        for (int l = 1; l < tail; ++l) {
            const LevelGeom& lg = g.lv[l];
            if (B < KR_SHORT_BATCH) {
                dim3 grid((lg.pitch + RZ_TW - 1) / RZ_TW, (lg.ph + RZ_THS - 1) / RZ_THS, B);
                hipLaunchKernelGGL(k_pyr_resize<RZ_THS>, grid, dim3(256), resizeLdsS[l], st, d_pyr, d_rtab, g.lv[l],
                                   g.lv[l - 1]);
            } else {
                dim3 grid((lg.pitch + RZ_TW - 1) / RZ_TW, (lg.ph + RZ_TH - 1) / RZ_TH, B);
                hipLaunchKernelGGL(k_pyr_resize<RZ_TH>, grid, dim3(256), resizeLds[l], st, d_pyr, d_rtab, g.lv[l],
                                   g.lv[l - 1]);
            }
        }
        if (tail < nlevels)
            hipLaunchKernelGGL(k_pyr_resize_tail, dim3(B), dim3(RT_THREADS), tailLds, st, d_pyr, d_rtab, g, resizeTail,
                               tailBufA, tailBufB);
        stage_end(1, st);
        pyrBatch = B;
        }
        if (!(phases & 2u)) {
            ORB_HIPCHK(hipGetLastError());
            return ORB_OK;
        }
        stage_begin(2, st);
        if (!countsZeroed) ORB_HIPCHK(hipMemsetAsync(d_cellCount, 0, (size_t)g.nCells * B * 4, st));
        orb_ilp_fast(nTiles, B, st, d_pyr, g, d_tiles, d_cand, d_cellCount);
        stage_end(2, st);
        stage_begin(3, st);
        // FAST(7) re-runs: spread over NWG workgroups per level (k_rerun), ahead of k_select's one
        // workgroup per level and frame.  Measured against re-running inside k_select (removed
        // after f2fe5e8) at B = 512, re-run + select: 640x480 0.190 vs 0.239 ms inside; 1241x376
        // 0.497 vs 0.696; 1280x720 0.864 vs 1.421.  (cellLds > 0: the first cell of every level
        // has a detection area, build_geometry.)
        {
            const int NWG = std::min(32, std::max(KR_NWG_MIN, 512 / (B * nlevels)));
            hipLaunchKernelGGL(k_rerun, dim3(B * NWG, nlevels), dim3(256), cellLds, st, d_pyr, d_cand, d_cellCount, g,
                               d_cells, NWG);
        }
        const dim3 sg(B, nlevels);
        if (scoreType == ORB_HARRIS_SCORE)
            hipLaunchKernelGGL((k_select<true, false>), sg, dim3(256), listLds, st, d_pyr, d_cand, d_cand2, d_cellCount,
                               g, d_cells, d_lvl, d_lvlCount, d_candH, d_lvlResp, harrisScale4, d_selDone, d_lvlInfo,
                               counts);
        else
            hipLaunchKernelGGL((k_select<false, false>), sg, dim3(256), listLds, st, d_pyr, d_cand, d_cand2, d_cellCount,
                               g, d_cells, d_lvl, d_lvlCount, (uint64_t*)nullptr, (float*)nullptr, 0.f, d_selDone,
                               d_lvlInfo, counts);
        // (the frames' per-level output offsets and totals: written by each frame's last k_select
        // workgroup, select_frame_done)
        if (hipError_t e = hipGetLastError(); e != hipSuccess) {
            // a k_select launch that did not run to completion leaves selDone[b] counting: clear it,
            // or the next extraction on this handle would take its frames' counts from stale levels
            (void)hipMemsetAsync(d_selDone, 0, (size_t)maxBatch * sizeof(int), st);
            return orb_internal_set_error(ORB_EDEVICE, std::string("k_select launch: ") + hipGetErrorString(e));
        }
        stage_end(3, st);
        stage_begin(4, st);
        dim3 gd((std::max(kpCap, 1) + OD_WAVES - 1) / OD_WAVES, B);
        hipLaunchKernelGGL(k_orient_desc, gd, dim3(64 * OD_WAVES), 0, st, d_pyr, g, d_lvl, d_slotLvl, d_lvlInfo, kps,
                           desc, (const float*)d_lvlResp);
        stage_end(4, st);
        ORB_HIPCHK(hipGetLastError());
        return ORB_OK;
    }
};

static int upload_pattern(int device) {
    static bool uploaded[64] = {};
    static std::mutex mu;
    std::lock_guard<std::mutex> lock(mu);
    if (device >= 0 && device < 64 && uploaded[device]) return ORB_OK;
    float pf[1024];  // pair-major: point 8 l + q at pair 64 q + l (c_patternf)
    for (int l = 0; l < 64; ++l)
        for (int q = 0; q < 8; ++q)
            for (int c = 0; c < 2; ++c) pf[2 * (64 * q + l) + c] = (float)kOrbPattern31[2 * (8 * l + q) + c];
    ORB_HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(c_patternf), pf, sizeof(pf)));
    {  // IC disc masks per alignment (umax of ORBextractor.cc:495-510, HALF_PATCH_SIZE 15)
        int um[16];
        const int vmax = (int)std::floor(15 * std::sqrt(2.f) / 2 + 1), vmin = (int)std::ceil(15 * std::sqrt(2.f) / 2);
        for (int v = 0; v <= vmax; ++v) um[v] = (int)lrint(std::sqrt(225.0 - v * v));
        for (int v = 15, v0 = 0; v >= vmin; --v) {
            while (um[v0] == um[v0 + 1]) ++v0;
            um[v] = v0;
            ++v0;
        }
        uint32_t off[320], c10[4 * 320] = {}, c01[4 * 320] = {};
        for (int n = 0; n < 320; ++n) off[n] = (uint32_t)(OD_WP * (n / 9) + 4 * (n % 9));
        for (int sh = 0; sh < 4; ++sh)
            for (int n = 0; n < 31 * 9; ++n) {
                const int r = n / 9, c = n % 9, v = std::abs(r - 15);
                uint32_t w10 = 0, w01 = 0;
                for (int i = 0; i < 4; ++i) {
                    const int u = 4 * c + i - sh - 15;
                    if (std::abs(u) <= um[v]) {
                        w10 |= (uint32_t)(uint8_t)(int8_t)u << (8 * i);
                        w01 |= (uint32_t)(uint8_t)(int8_t)(r - 15) << (8 * i);
                    }
                }
                c10[320 * sh + n] = w10;
                c01[320 * sh + n] = w01;
            }
        ORB_HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(c_icoff), off, sizeof(off)));
        ORB_HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(c_ic10), c10, sizeof(c10)));
        ORB_HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(c_ic01), c01, sizeof(c01)));
    }
    {  // banded 7-tap row-pass matrix (GaussianBlur 7x7 sigma 2 fixed-point taps) + the bias rows
        static const int8_t tap[7] = {18, 34, 49, 55, 49, 34, 18};
        uint8_t bf[4 * 64 * 16];
        for (int t = 0; t < 4; ++t)
            for (int l = 0; l < 64; ++l)
                for (int j = 0; j < 16; ++j) {
                    const int k = 16 * (l >> 4) + j, n = 16 * t + (l & 15);
                    int8_t v = (k - n >= 0 && k - n <= 6) ? tap[k - n] : 0;
                    if (k >= 61) v = k == 63 ? 58 : 127;  // 127*127 + 127*127 + 11*58 = 128 * 257
                    bf[(t * 64 + l) * 16 + j] = (uint8_t)v;
                }
        ORB_HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(c_rowB), bf, sizeof(bf)));
    }
    if (device >= 0 && device < 64) uploaded[device] = true;
    return ORB_OK;
}

// ======================================================================================
// C ABI
// ======================================================================================
extern "C" {

const char* orb_last_error(void) { return g_last_error.c_str(); }

const char* orb_version(void) { return "orb_hip gfx950 " __DATE__; }

int orb_extractor_create(int nfeatures, float scale_factor, int nlevels, int score_type, int fast_th, int device,
                         int max_batch, orb_extractor_t** out) {
    if (!out) return orb_internal_set_error(ORB_EINVAL, "out is NULL");
    *out = nullptr;
    if (nfeatures <= 0 || nlevels <= 0 || nlevels > ORB_MAX_LEVELS || !(scale_factor > 1.0f) || max_batch <= 0)
        return orb_internal_set_error(ORB_EINVAL, "invalid extractor parameters");
    if (score_type != ORB_FAST_SCORE && score_type != ORB_HARRIS_SCORE)
        return orb_internal_set_error(ORB_EINVAL, "score_type must be HARRIS_SCORE(0) or FAST_SCORE(1)");
    int ndev = 0;
    ORB_HIPCHK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return orb_internal_set_error(ORB_EINVAL, "device ordinal out of range");
    ORB_HIPCHK(hipSetDevice(device));
    int st = upload_pattern(device);
    if (st) return st;
    // k_select<true> (HARRIS_SCORE) stages (response, record) pairs: up to 96 KB of LDS
    hipFuncSetAttribute((const void*)k_select<true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
    hipFuncSetAttribute((const void*)k_select<false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
    hipFuncSetAttribute((const void*)k_rerun, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
    hipFuncSetAttribute((const void*)k_pyr_resize_tail, hipFuncAttributeMaxDynamicSharedMemorySize, RT_LDS_MAX);
    orb_ilp_init();
    orb_extractor* h = new orb_extractor();
    h->nfeatures = nfeatures;
    h->scaleFactor = scale_factor;
    h->nlevels = nlevels;
    h->scoreType = score_type;
    h->fastTh = fast_th;
    {  // HarrisResponses' scale (ORBextractor.cc:89-91), blockSize 7, in the reference's float steps
        float scale = (1 << 2) * 7 * 255.0f;
        scale = 1.0f / scale;
        h->harrisScale4 = scale * scale * scale * scale;
    }
    h->device = device;
    h->maxBatch = max_batch;
    h->init_params();
    hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->evOrder, hipEventDisableTiming);
    if (e != hipSuccess) {
        if (h->stream) (void)hipStreamDestroy(h->stream);
        delete h;
        return orb_internal_set_error(ORB_EDEVICE, std::string("hipStreamCreate: ") + hipGetErrorString(e));
    }
    *out = h;
    return ORB_OK;
}

int orb_extractor_destroy(orb_extractor_t* h) {
    if (!h) return ORB_OK;
    hipSetDevice(h->device);
    (void)h->drain();
    h->free_ws();
    h->free_events();
    hipEventDestroy(h->evOrder);
    hipStreamDestroy(h->stream);
    delete h;
    return ORB_OK;
}

int orb_get_levels(const orb_extractor_t* h) { return h ? h->nlevels : ORB_EINVAL; }

float orb_get_scale_factor(const orb_extractor_t* h) { return h ? (float)h->scaleFactor : 0.f; }

int orb_get_max_keypoints(const orb_extractor_t* h) { return h ? h->kpCap : ORB_EINVAL; }

int orb_get_level_info(const orb_extractor_t* h, int* fpl, float* sf) {
    if (!h) return ORB_EINVAL;
    for (int l = 0; l < h->nlevels; ++l) {
        if (fpl) fpl[l] = h->nDesired[l];
        if (sf) sf[l] = h->mvScaleFactor[l];
    }
    return ORB_OK;
}

int orb_extract_batch_device(orb_extractor_t* h, int B, const uint8_t* d_imgs, int w, int hgt, int stride,
                             int64_t frame_pitch, orb_keypoint_t* d_kps, uint8_t* d_desc, int32_t* d_counts,
                             void* stream) {
    if (!h || B <= 0 || !d_imgs || !d_kps || !d_desc || !d_counts)
        return orb_internal_set_error(ORB_EINVAL, "bad arguments");
    if (B > h->maxBatch) return orb_internal_set_error(ORB_EINVAL, "B exceeds max_batch");
    if (w <= 0 || hgt <= 0 || stride < w || frame_pitch < (int64_t)stride * hgt)
        return orb_internal_set_error(ORB_EINVAL, "bad image geometry");
    ORB_HIPCHK(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;  // NULL = the null stream, as everywhere in HIP
    if (w != h->W || hgt != h->H) {
        // the workspace is re-allocated: drain every stream that may still be using it
        if (int r = h->drain()) return r;
        int r = h->build_geometry(w, hgt);
        if (r) return r;
    }
    return h->launch(B, d_imgs, stride, frame_pitch, d_kps, d_desc, d_counts, st, 1, 0, h->phaseMask);
}

int orb_extract_batch(orb_extractor_t* h, int B, const uint8_t* imgs, int w, int hgt, int stride, int64_t frame_pitch,
                      orb_keypoint_t* kps_out, uint8_t* desc_out, int32_t* n_out) {
    if (!h || B <= 0 || !imgs || !kps_out || !desc_out || !n_out)
        return orb_internal_set_error(ORB_EINVAL, "bad arguments");
    if (B > h->maxBatch) return orb_internal_set_error(ORB_EINVAL, "B exceeds max_batch");
    if (w <= 0 || hgt <= 0 || stride < w || frame_pitch < (int64_t)stride * hgt)
        return orb_internal_set_error(ORB_EINVAL, "bad image geometry");
    ORB_HIPCHK(hipSetDevice(h->device));
    if (w != h->W || hgt != h->H) {
        if (int r = h->drain()) return r;
        int st = h->build_geometry(w, hgt);
        if (st) return st;
    }
    // the copies below overwrite the staging a launch on another stream may still read
    if (int r = h->order_after_last(h->stream)) return r;
    int st = h->ensure_staging();
    if (st) return st;
    if (stride == w && frame_pitch == (int64_t)w * hgt) {  // tight frames: one linear copy
        ORB_HIPCHK(hipMemcpyAsync(h->d_img, imgs, (size_t)B * w * hgt, hipMemcpyHostToDevice, h->stream));
    } else {
        for (int k = 0; k < B; ++k)
            ORB_HIPCHK(hipMemcpy2DAsync(h->d_img + (size_t)k * w * hgt, w, imgs + (size_t)k * frame_pitch, stride, w,
                                     (size_t)hgt, hipMemcpyHostToDevice, h->stream));
    }
    st = h->launch(B, h->d_img, w, (long long)w * hgt, h->d_kps, h->d_desc, h->d_counts, h->stream);
    if (st) return st;
    ORB_HIPCHK(hipMemcpyAsync(n_out, h->d_counts, (size_t)B * 4, hipMemcpyDeviceToHost, h->stream));
    ORB_HIPCHK(hipMemcpyAsync(kps_out, h->d_kps, (size_t)B * h->kpCap * sizeof(orb_keypoint_t), hipMemcpyDeviceToHost,
                           h->stream));
    ORB_HIPCHK(hipMemcpyAsync(desc_out, h->d_desc, (size_t)B * h->kpCap * 32, hipMemcpyDeviceToHost, h->stream));
    ORB_HIPCHK(hipStreamSynchronize(h->stream));
    return ORB_OK;
}

int orb_extract(orb_extractor_t* h, const uint8_t* img, int w, int hgt, int stride, orb_keypoint_t* kps_out,
                int kps_cap, uint8_t* desc_out, int* n_out) {
    if (!h || !n_out) return orb_internal_set_error(ORB_EINVAL, "bad arguments");
    if (w <= 0 || hgt <= 0) {  // _image.empty(): return, outputs untouched (ORBextractor.cc:721-722)
        *n_out = 0;
        return ORB_OK;
    }
    if (!img || !kps_out || !desc_out) return orb_internal_set_error(ORB_EINVAL, "bad arguments");
    if (stride < w) return orb_internal_set_error(ORB_EINVAL, "bad image geometry");
    ORB_HIPCHK(hipSetDevice(h->device));
    if (w != h->W || hgt != h->H) {
        if (int r = h->drain()) return r;
        if (int r = h->build_geometry(w, hgt)) return r;
    }
    // the upload overwrites the staging a launch on another stream may still read
    if (int r = h->order_after_last(h->stream)) return r;
    if (int r = h->ensure_staging()) return r;
    if (int r = h->upload_frame(h->d_img, img, (size_t)w, hgt, (size_t)stride)) return r;
    if (int r = h->launch(1, h->d_img, w, (long long)w * hgt, h->d_kps, h->d_desc, h->d_counts, h->stream)) {
        (void)hipStreamSynchronize(h->stream);
        return r;
    }
    return h->download_frame0(kps_out, kps_cap, desc_out, n_out);
}

int orb_extract_batch_device_color(orb_extractor_t* h, int B, const uint8_t* d_imgs, int w, int hgt, int stride,
                                   int64_t frame_pitch, int channels, int rgb, orb_keypoint_t* d_kps, uint8_t* d_desc,
                                   int32_t* d_counts, void* stream) {
    if (!h || B <= 0 || !d_imgs || !d_kps || !d_desc || !d_counts)
        return orb_internal_set_error(ORB_EINVAL, "bad arguments");
    if (channels != 3 && channels != 4) return orb_internal_set_error(ORB_EINVAL, "channels must be 3 or 4");
    if (B > h->maxBatch) return orb_internal_set_error(ORB_EINVAL, "B exceeds max_batch");
    if (w <= 0 || hgt <= 0 || stride < w * channels || frame_pitch < (int64_t)stride * hgt)
        return orb_internal_set_error(ORB_EINVAL, "bad image geometry");
    ORB_HIPCHK(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    if (w != h->W || hgt != h->H) {
        if (int r = h->drain()) return r;
        int r = h->build_geometry(w, hgt);
        if (r) return r;
    }
    return h->launch(B, d_imgs, stride, frame_pitch, d_kps, d_desc, d_counts, st, channels, rgb);
}

int orb_extract_color(orb_extractor_t* h, const uint8_t* img, int w, int hgt, int stride, int channels, int rgb,
                      orb_keypoint_t* kps_out, int kps_cap, uint8_t* desc_out, int* n_out) {
    if (!h || !n_out) return orb_internal_set_error(ORB_EINVAL, "bad arguments");
    if (w <= 0 || hgt <= 0) {  // _image.empty(): return, outputs untouched (ORBextractor.cc:721-722)
        *n_out = 0;
        return ORB_OK;
    }
    if (!img || !kps_out || !desc_out) return orb_internal_set_error(ORB_EINVAL, "bad arguments");
    if (channels != 3 && channels != 4) return orb_internal_set_error(ORB_EINVAL, "channels must be 3 or 4");
    if (stride < w * channels) return orb_internal_set_error(ORB_EINVAL, "bad image geometry");
    ORB_HIPCHK(hipSetDevice(h->device));
    if (w != h->W || hgt != h->H) {
        if (int r = h->drain()) return r;
        int r = h->build_geometry(w, hgt);
        if (r) return r;
    }
    if (int r = h->order_after_last(h->stream)) return r;
    int st = h->ensure_staging();
    if (st) return st;
    const size_t row = (size_t)w * channels;
    if (row * hgt > h->imgColorCap) {  // handle-owned, grow-only (the stream is ordered after every user)
        ORB_HIPCHK(hipStreamSynchronize(h->stream));
        (void)hipFree(h->d_imgColor);
        h->d_imgColor = nullptr;
        h->imgColorCap = 0;
        ORB_HIPCHK(hipMalloc(&h->d_imgColor, row * hgt));
        h->imgColorCap = row * hgt;
    }
    if (int r = h->upload_frame(h->d_imgColor, img, row, hgt, (size_t)stride)) return r;
    st = h->launch(1, h->d_imgColor, (int)row, (long long)(row * hgt), h->d_kps, h->d_desc, h->d_counts, h->stream,
                   channels, rgb);
    if (st) {
        (void)hipStreamSynchronize(h->stream);
        return st;
    }
    return h->download_frame0(kps_out, kps_cap, desc_out, n_out);
}

int orb_descriptor_distance(const uint8_t* a, const uint8_t* b) {
    int dist = 0;
    for (int i = 0; i < 8; ++i) {
        uint32_t pa, pb;
        std::memcpy(&pa, a + 4 * i, 4);
        std::memcpy(&pb, b + 4 * i, 4);
        dist += __builtin_popcount(pa ^ pb);
    }
    return dist;
}


// A stream with every CU in its mask: the runtime gives a CU-masked stream a hardware queue of
// its own instead of sharing one of its GPU_MAX_HW_QUEUES round-robin (include/orb_abi.h).
int orb_stream_create_dedicated(void** out_stream) {
    if (!out_stream) return orb_internal_set_error(ORB_EINVAL, "bad arguments");
    int dev = 0;
    ORB_HIPCHK(hipGetDevice(&dev));
    int ncu = 0;
    ORB_HIPCHK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
    std::vector<uint32_t> mask((size_t)(ncu + 31) / 32, 0xFFFFFFFFu);
    if (ncu % 32) mask.back() = (1u << (ncu % 32)) - 1u;
    hipStream_t st = nullptr;
    ORB_HIPCHK(hipExtStreamCreateWithCUMask(&st, (uint32_t)mask.size(), mask.data()));
    *out_stream = (void*)st;
    return ORB_OK;
}

int orb_stream_destroy(void* stream) {
    if (!stream) return orb_internal_set_error(ORB_EINVAL, "bad arguments");
    orb_match_release_stream_scratch(stream);
    ORB_HIPCHK(hipStreamDestroy((hipStream_t)stream));
    return ORB_OK;
}

static const char* kStageNames[] = {"k_pyr0", "k_pyr_resize", "k_fast", "k_select", "k_orient_desc"};

int orb_profile_enable(orb_extractor_t* h, int enable) {
    return orb_profile_enable_stages(h, enable ? (1u << orb_extractor::kStages) - 1u : 0u);
}

int orb_debug_set_pyramid_path(orb_extractor_t* h, int mode) {
    if (!h || mode < 0 || mode > 2) return orb_internal_set_error(ORB_EINVAL, "mode must be 0, 1 or 2");
    h->pyrLegacy = mode == 1;
    h->pyrStreamAlways = mode == 2;
    return ORB_OK;
}

int orb_debug_set_fast_corner_list(orb_extractor_t* h, int cap) {
    if (!h || cap < 0 || cap > FT_CL) return orb_internal_set_error(ORB_EINVAL, "cap must be in [0, 256]");
    h->fastCl = cap;
    h->g.fastCl = cap;
    return ORB_OK;
}

int orb_debug_pyramid_plan(const orb_extractor_t* h, int* rows_per_round, int* rounds, int* lds_bytes) {
    if (!h) return orb_internal_set_error(ORB_EINVAL, "bad handle");
    if (!h->streamOk) return 0;
    if (rows_per_round) *rows_per_round = h->streamK0;
    if (rounds) *rounds = h->sgeom.nRounds;
    if (lds_bytes) *lds_bytes = (int)h->streamLds;
    return 1;
}

int orb_debug_pyramid_plan_levels(const orb_extractor_t* h, int* nq, int* n_waves, int* ring_rows, int cap) {
    if (!h || cap < 0) return orb_internal_set_error(ORB_EINVAL, "bad arguments");
    if (!h->streamOk) return 0;
    const int L = (int)h->streamLv.size();
    for (int l = 0; l < L && l < cap; ++l) {
        if (nq) nq[l] = h->streamLv[l].nq;
        if (n_waves) n_waves[l] = h->streamLv[l].nWaves;
        if (ring_rows) ring_rows[l] = l + 1 < L ? h->streamCap[l] : 0;
    }
    return L;
}

int orb_debug_fill_pyramid(orb_extractor_t* h, int value) {
    if (!h || !h->d_pyr || value < 0 || value > 255) return orb_internal_set_error(ORB_EINVAL, "bad arguments");
    ORB_HIPCHK(hipSetDevice(h->device));
    // ordered like a launch: after the handle's last one, and before its next on any stream
    if (int r = h->order_after_last(h->stream)) return r;
    ORB_HIPCHK(hipMemsetAsync(h->d_pyr, value, h->pyrAlloc, h->stream));
    h->pyrBatch = 0;
    return ORB_OK;
}

int orb_extract_set_phases(orb_extractor_t* h, unsigned phase_mask) {
    if (!h) return orb_internal_set_error(ORB_EINVAL, "bad handle");
    if (phase_mask == 0u || (phase_mask & ~3u))
        return orb_internal_set_error(ORB_EINVAL, "phase_mask must be 1, 2 or 3");
    h->phaseMask = phase_mask;
    return ORB_OK;
}

int orb_profile_enable_stages(orb_extractor_t* h, unsigned stage_mask) {
    if (!h) return orb_internal_set_error(ORB_EINVAL, "bad handle");
    ORB_HIPCHK(hipSetDevice(h->device));
    int r = h->profile_collect();
    if (r) return r;
    h->profMask = stage_mask & ((1u << orb_extractor::kStages) - 1u);
    h->prof = h->profMask != 0;
    for (int k = 0; k < orb_extractor::kStages; ++k) {
        h->stageMs[k] = 0;
        h->stageLaunches[k] = 0;
    }
    return ORB_OK;
}

int orb_profile_read(orb_extractor_t* h, double* stage_ms, int64_t* stage_launches, int nstages) {
    if (!h || nstages < 0) return orb_internal_set_error(ORB_EINVAL, "bad arguments");
    ORB_HIPCHK(hipSetDevice(h->device));
    int r = h->profile_collect();
    if (r) return r;
    for (int k = 0; k < nstages && k < orb_extractor::kStages; ++k) {
        if (stage_ms) stage_ms[k] = h->stageMs[k];
        if (stage_launches) stage_launches[k] = h->stageLaunches[k];
    }
    return orb_extractor::kStages;
}

const char* orb_profile_stage_name(int i) {
    return (i >= 0 && i < orb_extractor::kStages) ? kStageNames[i] : "";
}

// ---- debug / test hooks (no device work) ------------------------------------------------
// Host instantiation of the device nth_element replay, for CPU unit tests.
int orb_debug_nth_element_u32(uint32_t* a, int n, int nth) {
    ScoreGreater comp;
    orbsel::nth_element(a, nth, n, comp);
    return ORB_OK;
}

}  // extern "C"

__global__ void __launch_bounds__(64) k_debug_nth_wave(uint32_t* a, int n, int nth) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_a[];
    uint16_t* Lp = (uint16_t*)(s_a + n);
    for (int i = threadIdx.x; i < n; i += 64) s_a[i] = a[i];
    __syncthreads();
    ScoreGreater comp;
    orbsel::nth_element_wave(s_a, nth, n, comp, Lp, Lp + n, (int)threadIdx.x);
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += 64) a[i] = s_a[i];
}

extern "C" {

int orb_debug_nth_element_wave_u32(uint32_t* a, int n, int nth, int device) {
    if (!a || n < 0 || n > 8192 || nth < 0 || nth > n) return orb_internal_set_error(ORB_EINVAL, "bad arguments");
    if (n == 0) return ORB_OK;
    ORB_HIPCHK(hipSetDevice(device));
    uint32_t* d = nullptr;
    ORB_HIPCHK(hipMalloc(&d, (size_t)n * 4));
    hipError_t e = hipMemcpy(d, a, (size_t)n * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        (void)hipFuncSetAttribute((const void*)k_debug_nth_wave, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
        hipLaunchKernelGGL(k_debug_nth_wave, dim3(1), dim3(64), (size_t)n * 8, 0, d, n, nth);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(a, d, (size_t)n * 4, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess)
        return orb_internal_set_error(ORB_EDEVICE, std::string("nth_element_wave: ") + hipGetErrorString(e));
    return ORB_OK;
}

// Download a padded pyramid level of frame `b` (after the last batch) into `out`
// ((w+32) x (h+32) bytes, tightly packed).  Synchronises the handle's stream.
int orb_debug_level_image(orb_extractor_t* h, int b, int l, uint8_t* out, int* w, int* hgt) {
    if (!h || l < 0 || l >= h->nlevels || !h->d_pyr) return orb_internal_set_error(ORB_EINVAL, "bad arguments");
    const LevelGeom& lg = h->g.lv[l];
    if (w) *w = lg.w;
    if (hgt) *hgt = lg.h;
    if (!out) return ORB_OK;
    ORB_HIPCHK(hipSetDevice(h->device));
    ORB_HIPCHK(hipDeviceSynchronize());
    ORB_HIPCHK(hipMemcpy2D(out, lg.w + 32, h->d_pyr + lg.base + (long long)b * lg.fstride, lg.pitch, lg.w + 32, lg.ph,
                        hipMemcpyDeviceToHost));
    return ORB_OK;
}

// The bytes of the same level's rows between the padded image and the row pitch: (h+32) rows of
// pitch - (w+32) bytes (the return value, 0 .. 15), tightly packed.  Every builder writes zeros there.
int orb_debug_level_row_slack(orb_extractor_t* h, int b, int l, uint8_t* out) {
    if (!h || b < 0 || b >= h->maxBatch || l < 0 || l >= h->nlevels || !h->d_pyr)
        return orb_internal_set_error(ORB_EINVAL, "bad arguments");
    const LevelGeom& lg = h->g.lv[l];
    const int slack = lg.pitch - (lg.w + 32);
    if (!out || slack == 0) return slack;
    ORB_HIPCHK(hipSetDevice(h->device));
    ORB_HIPCHK(hipDeviceSynchronize());
    ORB_HIPCHK(hipMemcpy2D(out, slack, h->d_pyr + lg.base + (long long)b * lg.fstride + lg.w + 32, lg.pitch, slack,
                           lg.ph, hipMemcpyDeviceToHost));
    return slack;
}

// Descriptor image of level l, frame b (blurred ROI + raw padding), padded layout, computed by
// k_debug_desc_image with k_orient_desc's rounding (the product never materialises it).
int orb_debug_blur_image(orb_extractor_t* h, int b, int l, uint8_t* out) {
    if (!h || l < 0 || l >= h->nlevels || !h->d_pyr || !out) return orb_internal_set_error(ORB_EINVAL, "bad arguments");
    const LevelGeom& lg = h->g.lv[l];
    ORB_HIPCHK(hipSetDevice(h->device));
    ORB_HIPCHK(hipDeviceSynchronize());
    const size_t n = (size_t)(lg.w + 32) * (lg.h + 32);
    uint8_t* d = nullptr;
    ORB_HIPCHK(hipMalloc(&d, n));
    hipLaunchKernelGGL(k_debug_desc_image, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, h->d_pyr, lg, b, d);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpy(out, d, n, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess)
        return orb_internal_set_error(ORB_EDEVICE, std::string("debug descriptor image: ") + hipGetErrorString(e));
    return ORB_OK;
}

#if KR_TIMING
// experiment builds: k_rerun's per-level phase sums, [level][8] (see cell_fast_rerun)
int orb_debug_kr_timing(unsigned long long* out) {
    ORB_HIPCHK(hipDeviceSynchronize());
    ORB_HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_krtime), sizeof(g_krtime)));
    static unsigned long long z[ORB_MAX_LEVELS][8] = {};
    ORB_HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_krtime), z, sizeof(z)));
    return ORB_OK;
}
#endif
#if KS_TIMING
// experiment builds: k_select's per-level phase sums, [level][8] (see the kernel)
int orb_debug_ks_timing(unsigned long long* out) {
    ORB_HIPCHK(hipDeviceSynchronize());
    ORB_HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_kstime), sizeof(g_kstime)));
    static unsigned long long z[ORB_MAX_LEVELS][8] = {};
    ORB_HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_kstime), z, sizeof(z)));
    return ORB_OK;
}
#endif
// Per-cell FAST counts (after fallback) of frame `b`, level `l`, row-major cells.
int orb_debug_cell_counts(orb_extractor_t* h, int b, int l, int* counts, int cap) {
    if (!h || l < 0 || l >= h->nlevels || !h->d_cellCount) return orb_internal_set_error(ORB_EINVAL, "bad arguments");
    const LevelGeom& lg = h->g.lv[l];
    int n = lg.rows * lg.cols;
    if (n > cap) return ORB_ERANGE;
    ORB_HIPCHK(hipSetDevice(h->device));
    ORB_HIPCHK(hipDeviceSynchronize());
    ORB_HIPCHK(hipMemcpy(counts, h->d_cellCount + (long long)b * h->g.nCells + lg.cell0, (size_t)n * 4,
                      hipMemcpyDeviceToHost));
    return n;
}

}  // extern "C"
