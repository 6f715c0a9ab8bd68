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
// (k_match_init) is orb_sfi.hip.  What a frame size decides (level and cell geometry, resize
// tables, k_fast's tiles, k_pyr_stream's schedule, every refusal) is the HIP-free planner
// orb_extract_plan.h; the handle below allocates and uploads from its plan.  The thread's last
// error (orb_last_error, orb_internal_set_error) is orb_runtime.hip.
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
#include "orb_extract_plan.h"
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
// The SSE2 path's (h * b) >> 16 is then mulhi(h, b << 16).  (RZ_TW, RZ_TH, RZ_THS: orb_extract_plan.h,
// whose planner builds the tile tables.)
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
#define RT_THREADS 1024  // (its LDS bound RT_LDS_MAX: orb_extract_plan.h)
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

// k_pyr_stream (orb_ilp.hip): when the host uses it (the LDS its plan aims for, PS_LDS_TARGET:
// orb_extract_plan.h)
#ifndef KR_STREAM_BATCH  // smallest batch that uses k_pyr_stream (one workgroup per frame)
#define KR_STREAM_BATCH 256
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
// rerun_lds() bytes (orb_extract_plan.h, with RR_Q).  Output: each survivor sets its bit in its row's mask
// and counts into its row; after the row prefix one thread per mask word writes that word's
// survivors at the row's offset + the set bits of the row's earlier words (no per-row scan of
// the cell, no list, no returning atomics in the NMS).

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
// level's survivors fit (Geom::selCap = select_cap(), orb_extract_plan.h), otherwise in the frame's scratch area `cand2`.
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
using orbplan::ExtractParams;
using orbplan::ExtractPlan;

// The handle's buffers of the current frame size.  Value-initialised: none.  A device buffer is
// named here and where orb_extractor::alloc / upload allocates it, which registers it for
// free_ws; the pinned host block is ensure_pinned's.
struct ExtractWorkspace {
    uint8_t* d_pyr = nullptr;
    size_t pyrAlloc = 0;  // bytes of d_pyr (orb_debug_fill_pyramid)
    FastTile* d_tiles = nullptr;
    uint32_t* d_cand = nullptr;
    int* d_cellCount = nullptr;
    uint32_t* d_cand2 = nullptr;  // k_select scratch when a level's survivors exceed its LDS
    uint32_t* d_lvl = nullptr;
    int* d_lvlCount = nullptr;
    int2* d_lvlInfo = nullptr;     // [frame][ORB_MAX_LEVELS] (first output slot, count): k_select's last WG
    int* d_selDone = nullptr;      // [frame] k_select workgroups done (self-resetting, zero between launches)
    uint8_t* d_slotLvl = nullptr;  // keypoint slot -> level (ExtractPlan::slotLvl)
    uint64_t* d_candH = nullptr;   // HARRIS_SCORE: (response, record) scratch when a level exceeds LDS
    float* d_lvlResp = nullptr;    // HARRIS_SCORE: response of every kept keypoint
    int* d_rtab = nullptr;
    CellGeom* d_cells = nullptr;
    // k_pyr_stream's tables (plan.streamOk)
    uint32_t* d_scol = nullptr;
    uint32_t* d_srows = nullptr;
    StreamLevel* d_slv = nullptr;
    uint32_t* d_srounds = nullptr;
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
};

struct orb_extractor : ExtractWorkspace {
    ExtractParams prm;  // the constructor's arithmetic (orb_extract_plan.h)
    int device = 0, maxBatch = 1;
    float harrisScale4 = 0.f;
    hipStream_t stream = nullptr;      // the handle's own stream (host-buffer entry points)
    hipStream_t lastStream = nullptr;  // stream of the last launch on this handle's workspace
    bool lastValid = false;            // lastStream names a stream that ran a launch
    hipEvent_t evOrder = nullptr;      // orders a launch after the previous one on another stream
    int pyrBatch = 0;                  // frames whose pyramid phase 1 left in the workspace
    // the current frame size's plan (plan.W = plan.H = 0: none, no workspace either)
    ExtractPlan plan;
    int fastCl = FT_CL;        // orb_debug_set_fast_corner_list
    std::vector<void*> owned;  // every device buffer of the workspace, for free_ws
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

    void free_events() {
        for (auto e : evPool) hipEventDestroy(e);
        evPool.clear();
        evPending.clear();
        evNext = 0;
    }

    // one hipMalloc per workspace buffer, registered for free_ws
    template <class T>
    int alloc(T*& p, size_t bytes) {
        ORB_HIPCHK(hipMalloc(&p, bytes));
        owned.push_back(p);
        return ORB_OK;
    }
    // a buffer holding a table of the plan (one element at least, as an empty table has no size to ask for)
    template <class T>
    int upload(T*& p, const std::vector<T>& v) {
        if (int r = alloc(p, std::max<size_t>(v.size(), 1) * sizeof(T))) return r;
        if (!v.empty()) ORB_HIPCHK(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
        return ORB_OK;
    }
    void release(void* p) {
        owned.erase(std::remove(owned.begin(), owned.end(), p), owned.end());
        (void)hipFree(p);
    }

    void free_ws() {
        for (void* p : owned) (void)hipFree(p);
        owned.clear();
        if (h_pin) (void)hipHostFree(h_pin);
        static_cast<ExtractWorkspace&>(*this) = ExtractWorkspace{};
        plan = ExtractPlan{};
        pyrBatch = 0;
    }

    // The workspace of one frame size: the old one dropped, the size planned (every refusal
    // happens here, before anything is allocated), the buffers allocated and the plan's tables
    // uploaded.  The plan is kept only when all of that succeeded.
    int build_geometry(int w0, int h0) {
        free_ws();
        ExtractPlan P;
        std::string err;
        if (int r = orbplan::plan_extract(prm, w0, h0, maxBatch, fastCl, P, err)) return orb_internal_set_error(r, err);
        const Geom& G = P.g;
        const size_t cand = (size_t)std::max(G.candPerFrame, 1), kps = (size_t)std::max(prm.kpCap, 1);
        // + slack: k_orient_desc's 64-byte window rows and k_rerun's 16-B ROI units may over-read
        // the last row's pitch
        pyrAlloc = (size_t)P.pyrBytes + 256;
        if (int r = alloc(d_pyr, pyrAlloc)) return r;
        if (int r = upload(d_tiles, P.tiles)) return r;
        if (int r = alloc(d_cand, cand * maxBatch * 4)) return r;
        if (int r = alloc(d_cellCount, (size_t)G.nCells * maxBatch * 4)) return r;
        if (int r = alloc(d_cand2, cand * maxBatch * 4)) return r;
        if (int r = alloc(d_lvl, kps * maxBatch * 4)) return r;
        if (int r = alloc(d_lvlCount, (size_t)G.L * maxBatch * 4)) return r;
        if (int r = alloc(d_lvlInfo, (size_t)ORB_MAX_LEVELS * maxBatch * sizeof(int2))) return r;
        if (int r = alloc(d_selDone, (size_t)maxBatch * sizeof(int))) return r;
        ORB_HIPCHK(hipMemset(d_selDone, 0, (size_t)maxBatch * sizeof(int)));
        if (int r = upload(d_slotLvl, P.slotLvl)) return r;
        if (prm.scoreType == ORB_HARRIS_SCORE) {
            if (int r = alloc(d_candH, cand * maxBatch * 8)) return r;
            if (int r = alloc(d_lvlResp, kps * maxBatch * 4)) return r;
        }
        if (int r = upload(d_rtab, P.rtab)) return r;
        if (int r = upload(d_cells, P.cells)) return r;
        if (P.streamOk) {
            if (int r = upload(d_scol, P.streamCol)) return r;
            if (int r = upload(d_srows, P.streamRows)) return r;
            if (int r = upload(d_slv, P.streamLv)) return r;
            if (int r = upload(d_srounds, P.streamRounds)) return r;
        }
        plan = std::move(P);
        return ORB_OK;
    }

    // The workspace of frame size w x h: the current one, or a new one once every stream that
    // may still use the current one has drained.
    int ensure_geometry(int w, int h) {
        if (w == plan.W && h == plan.H) return ORB_OK;
        if (int r = drain()) return r;
        return build_geometry(w, h);
    }


    int ensure_staging() {
        if (d_img) return ORB_OK;
        if (int r = alloc(d_img, (size_t)plan.W * plan.H * maxBatch)) return r;
        const size_t cap = (size_t)std::max(prm.kpCap, 1);
        countsPad = ((size_t)maxBatch * 4 + 255) & ~(size_t)255;
        const size_t kpsBytes = ((cap * maxBatch * sizeof(orb_keypoint_t)) + 255) & ~(size_t)255;
        if (int r = alloc(d_out, countsPad + kpsBytes + cap * maxBatch * 32)) return r;
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
        const size_t img = (std::max(frameBytes, (size_t)plan.W * plan.H * 4) + 255) & ~(size_t)255;
        const size_t cap = (size_t)std::max(prm.kpCap, 1);
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
        const size_t cap = (size_t)std::max(prm.kpCap, 1);
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

    // The pyramid phase (stages 0 and 1) of B frames.  Returns whether k_pyr_stream zeroed
    // k_fast's cell counters on its way (`zeroCounts` asks it to).
    bool launch_pyramid(int B, const uint8_t* d_imgs, int stride, long long fpitch, hipStream_t st, int cn, int rgb,
                        bool zeroCounts) {
        const Geom& g = plan.g;
        pyrBatch = B;
        if (cn == 1 && plan.streamOk && (B >= KR_STREAM_BATCH || pyrStreamAlways) && !pyrLegacy) {
            // the whole pyramid in one streaming pass per frame (stage 0; stage 1 is empty)
            stage_begin(0, st);
            StreamGeom sg = plan.sgeom;
            const uintptr_t al = (uintptr_t)d_imgs | (uintptr_t)stride | (uintptr_t)fpitch;
            sg.align = (al & 15u) == 0 ? 16 : (al & 3u) == 0 ? 4 : 1;
            orb_ilp_pyr_stream(B, plan.streamLds, st, d_imgs, stride, fpitch, d_pyr, d_scol, (const uint4*)d_srows, d_slv,
                               d_srounds, sg, zeroCounts ? d_cellCount : (int*)nullptr, g.nCells);
            stage_end(0, st);
            return zeroCounts;
        }
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
        const int tail = B < KR_TAIL_BATCH ? g.L : plan.resizeTail;
        for (int l = 1; l < tail; ++l) {
            const LevelGeom& lg = g.lv[l];
            if (B < KR_SHORT_BATCH) {
                dim3 grid((lg.pitch + RZ_TW - 1) / RZ_TW, (lg.ph + RZ_THS - 1) / RZ_THS, B);
                hipLaunchKernelGGL(k_pyr_resize<RZ_THS>, grid, dim3(256), plan.resizeLdsS[l], st, d_pyr, d_rtab,
                                   g.lv[l], g.lv[l - 1]);
            } else {
                dim3 grid((lg.pitch + RZ_TW - 1) / RZ_TW, (lg.ph + RZ_TH - 1) / RZ_TH, B);
                hipLaunchKernelGGL(k_pyr_resize<RZ_TH>, grid, dim3(256), plan.resizeLds[l], st, d_pyr, d_rtab, g.lv[l],
                                   g.lv[l - 1]);
            }
        }
        if (tail < g.L)
            hipLaunchKernelGGL(k_pyr_resize_tail, dim3(B), dim3(RT_THREADS), plan.tailLds, st, d_pyr, d_rtab, g,
                               plan.resizeTail, plan.tailBufA, plan.tailBufB);
        stage_end(1, st);
        return false;
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
        const Geom& g = plan.g;
        const size_t cellLds = plan.cellLds, listLds = plan.listLds;
        bool countsZeroed = false;  // k_pyr_stream zeroed k_fast's cell counters
        if (phases & 1u) countsZeroed = launch_pyramid(B, d_imgs, stride, fpitch, st, cn, rgb, (phases & 2u) != 0);
        if (!(phases & 2u)) {
            ORB_HIPCHK(hipGetLastError());
            return ORB_OK;
        }
        stage_begin(2, st);
        if (!countsZeroed) ORB_HIPCHK(hipMemsetAsync(d_cellCount, 0, (size_t)g.nCells * B * 4, st));
        orb_ilp_fast((int)plan.tiles.size(), B, st, d_pyr, g, d_tiles, d_cand, d_cellCount);
        stage_end(2, st);
        stage_begin(3, st);
        // FAST(7) re-runs: spread over NWG workgroups per level (k_rerun), ahead of k_select's one
        // workgroup per level and frame.  Measured against re-running inside k_select (removed
        // after f2fe5e8) at B = 512, re-run + select: 640x480 0.190 vs 0.239 ms inside; 1241x376
        // 0.497 vs 0.696; 1280x720 0.864 vs 1.421.  (cellLds > 0: the first cell of every level
        // has a detection area, build_geometry.)
        {
            const int NWG = std::min(32, std::max(KR_NWG_MIN, 512 / (B * prm.nlevels)));
            hipLaunchKernelGGL(k_rerun, dim3(B * NWG, prm.nlevels), dim3(256), cellLds, st, d_pyr, d_cand, d_cellCount, g,
                               d_cells, NWG);
        }
        const dim3 sg(B, prm.nlevels);
        if (prm.scoreType == ORB_HARRIS_SCORE)
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
        dim3 gd((std::max(prm.kpCap, 1) + OD_WAVES - 1) / OD_WAVES, B);
        hipLaunchKernelGGL(k_orient_desc, gd, dim3(64 * OD_WAVES), 0, st, d_pyr, g, d_lvl, d_slotLvl, d_lvlInfo, kps,
                           desc, (const float*)d_lvlResp);
        stage_end(4, st);
        ORB_HIPCHK(hipGetLastError());
        return ORB_OK;
    }
};

static int upload_pattern(int device, const int* um) {  // um: ExtractParams::umax
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
    ExtractParams prm = orbplan::extract_params(nfeatures, scale_factor, nlevels, score_type, fast_th);
    int st = upload_pattern(device, prm.umax);
    if (st) return st;
    // k_select<true> (HARRIS_SCORE) stages (response, record) pairs: up to 96 KB of LDS
    hipFuncSetAttribute((const void*)k_select<true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
    hipFuncSetAttribute((const void*)k_select<false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
    hipFuncSetAttribute((const void*)k_rerun, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
    hipFuncSetAttribute((const void*)k_pyr_resize_tail, hipFuncAttributeMaxDynamicSharedMemorySize, RT_LDS_MAX);
    orb_ilp_init();
    orb_extractor* h = new orb_extractor();
    h->prm = std::move(prm);
    {  // HarrisResponses' scale (ORBextractor.cc:89-91), blockSize 7, in the reference's float steps
        float scale = (1 << 2) * 7 * 255.0f;
        scale = 1.0f / scale;
        h->harrisScale4 = scale * scale * scale * scale;
    }
    h->device = device;
    h->maxBatch = max_batch;
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

int orb_get_levels(const orb_extractor_t* h) { return h ? h->prm.nlevels : ORB_EINVAL; }

float orb_get_scale_factor(const orb_extractor_t* h) { return h ? (float)h->prm.scaleFactor : 0.f; }

int orb_get_max_keypoints(const orb_extractor_t* h) { return h ? h->prm.kpCap : ORB_EINVAL; }

int orb_get_level_info(const orb_extractor_t* h, int* fpl, float* sf) {
    if (!h) return ORB_EINVAL;
    for (int l = 0; l < h->prm.nlevels; ++l) {
        if (fpl) fpl[l] = h->prm.nDesired[l];
        if (sf) sf[l] = h->prm.mvScaleFactor[l];
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
    if (int r = h->ensure_geometry(w, hgt)) return r;
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
    if (int r = h->ensure_geometry(w, hgt)) return r;
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
    ORB_HIPCHK(hipMemcpyAsync(kps_out, h->d_kps, (size_t)B * h->prm.kpCap * sizeof(orb_keypoint_t), hipMemcpyDeviceToHost,
                           h->stream));
    ORB_HIPCHK(hipMemcpyAsync(desc_out, h->d_desc, (size_t)B * h->prm.kpCap * 32, hipMemcpyDeviceToHost, h->stream));
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
    if (int r = h->ensure_geometry(w, hgt)) return r;
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
    if (int r = h->ensure_geometry(w, hgt)) return r;
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
    if (int r = h->ensure_geometry(w, hgt)) return r;
    if (int r = h->order_after_last(h->stream)) return r;
    int st = h->ensure_staging();
    if (st) return st;
    const size_t row = (size_t)w * channels;
    if (row * hgt > h->imgColorCap) {  // handle-owned, grow-only (the stream is ordered after every user)
        ORB_HIPCHK(hipStreamSynchronize(h->stream));
        h->release(h->d_imgColor);
        h->d_imgColor = nullptr;
        h->imgColorCap = 0;
        if (int r = h->alloc(h->d_imgColor, row * hgt)) return r;
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
    h->plan.g.fastCl = cap;
    return ORB_OK;
}

int orb_debug_pyramid_plan(const orb_extractor_t* h, int* rows_per_round, int* rounds, int* lds_bytes) {
    if (!h) return orb_internal_set_error(ORB_EINVAL, "bad handle");
    if (!h->plan.streamOk) return 0;
    if (rows_per_round) *rows_per_round = h->plan.streamK0;
    if (rounds) *rounds = h->plan.sgeom.nRounds;
    if (lds_bytes) *lds_bytes = (int)h->plan.streamLds;
    return 1;
}

int orb_debug_pyramid_plan_levels(const orb_extractor_t* h, int* nq, int* n_waves, int* ring_rows, int cap) {
    if (!h || cap < 0) return orb_internal_set_error(ORB_EINVAL, "bad arguments");
    if (!h->plan.streamOk) return 0;
    const int L = (int)h->plan.streamLv.size();
    for (int l = 0; l < L && l < cap; ++l) {
        if (nq) nq[l] = h->plan.streamLv[l].nq;
        if (n_waves) n_waves[l] = h->plan.streamLv[l].nWaves;
        if (ring_rows) ring_rows[l] = l + 1 < L ? h->plan.streamCap[l] : 0;
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
    if (!h || l < 0 || l >= h->prm.nlevels || !h->d_pyr) return orb_internal_set_error(ORB_EINVAL, "bad arguments");
    const LevelGeom& lg = h->plan.g.lv[l];
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
    if (!h || b < 0 || b >= h->maxBatch || l < 0 || l >= h->prm.nlevels || !h->d_pyr)
        return orb_internal_set_error(ORB_EINVAL, "bad arguments");
    const LevelGeom& lg = h->plan.g.lv[l];
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
    if (!h || l < 0 || l >= h->prm.nlevels || !h->d_pyr || !out) return orb_internal_set_error(ORB_EINVAL, "bad arguments");
    const LevelGeom& lg = h->plan.g.lv[l];
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
    if (!h || l < 0 || l >= h->prm.nlevels || !h->d_cellCount) return orb_internal_set_error(ORB_EINVAL, "bad arguments");
    const LevelGeom& lg = h->plan.g.lv[l];
    int n = lg.rows * lg.cols;
    if (n > cap) return ORB_ERANGE;
    ORB_HIPCHK(hipSetDevice(h->device));
    ORB_HIPCHK(hipDeviceSynchronize());
    ORB_HIPCHK(hipMemcpy(counts, h->d_cellCount + (long long)b * h->plan.g.nCells + lg.cell0, (size_t)n * 4,
                      hipMemcpyDeviceToHost));
    return n;
}

}  // extern "C"
