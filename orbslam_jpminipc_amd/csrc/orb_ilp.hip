// orb_ilp.hip — k_pyr_stream and k_fast, compiled with the machine scheduler's max-ILP strategy
// (`-mllvm -amdgpu-sched-strategy=max-ilp`: __graft_entry__.ILP_FLAGS, this unit only) and
// launched by orb_hip.hip through the three orb_ilp_* functions at the end (orb_extract.h).
//
// Both kernels' occupancy is set by LDS (k_fast: five workgroups per CU) or by their own
// waves-per-EU target (k_pyr_stream: two workgroups per CU), so the default scheduler's
// occupancy-first schedule gains nothing from the registers it saves, and both kernels' time is
// their instruction issue: k_fast 442.5 -> 437.5 us per c3 step on one box, k_pyr_stream
// unchanged (289.4 / 289.9 us; both orders, two copies each: profiles/r06/r06_ilp3_summary.txt,
// HISTORY.md round 6).  The rest of
// the library keeps the default: k_orient_desc under max-ILP takes 112 VGPRs (occupancy 8 -> 4,
// 0.43 -> 0.58 ms) and spills when held to eight waves; k_select measured 10 % slower.
//
// The two kernels' timing probes (-DPS_TIMING=1 / -DKF_TIMING=1 experiment builds) and their
// readers live here too, so a timing build probes the kernels under the same scheduler flags.
#include <hip/hip_runtime.h>

#include "../../include/orb_debug.h"
#include "orb_internal.h"
#include "orb_device.h"
#include "orb_extract.h"

using namespace orbdev;

// ---- the whole pyramid of a frame in one streaming pass (large batches) ------------------
// k_pyr0 + k_pyr_resize x (L-1) read every level l-1 back from HBM to build level l.  Here one
// 1024-thread workgroup per frame walks down the frame once: each round loads the next K0
// level-0 rows into an LDS ring (prefetched into registers during the previous round), and
// every level l >= 1 computes the rows whose two source rows of level l-1 are already in that
// level's ring, writing them to the padded pyramid and (for the next level) to its own ring.
// Level l works on rows its source finished in an earlier round (level 1 on the level-0 rows of
// this round), so all levels run in one task pool per round: two barriers per round, no
// intermediate level ever leaves the CU except as the pyramid itself.  HBM traffic = the input
// read once + every padded level written once.
// The task loop issues no global load: on CDNA the vector-memory counter also counts stores, so
// a table load after a row's stores would wait for them.  The per-column taps live in LDS
// for the whole kernel, and the row entries of round n+1 are staged with the level-0 prefetch.
// The round schedule, ring capacities (the oldest row any round still reads to the newest one
// written by then), ring slots of every row and the per-column resize taps are host-built
// (build_stream_plan); the arithmetic per padded pixel is k_pyr0's / k_pyr_resize's exactly.
// Every ROI row r of a level goes to padded row r + 16 and to its reflect-101 mirrors 16 - r
// (1 <= r <= 16) and 2h + 14 - r (h - 17 <= r <= h - 2); the host requires h, w >= 17.
// One 16-B unit of a level-0 input row (nvalid >= 1 bytes of it inside the row; bytes past the
// row come back 0).  Aligned input: one 16-B load.  Otherwise (a 1241-px KITTI frame, a pitched
// view, a row's partial last unit): the one or two 16-B-aligned blocks holding the unit's valid
// bytes and a funnel shift — 16 byte loads per unit before, KITTI k_pyr_stream 0.799 -> 0.568 ms
// per 512 frames.  Only blocks holding a valid byte are read (the second is block 0 again when
// not needed, and its bytes are then never used), so no load leaves the pages of the input.
__device__ __forceinline__ uint4 load_unit16(const uint8_t* p, int nvalid, int align) {
    if (nvalid >= 16 && align == 16) return *(const uint4*)p;
    const int sh = (int)((uintptr_t)p & 15u), need = min(nvalid, 16);
    const uint4* blk = (const uint4*)(p - sh);  // pointer arithmetic on p: global, not flat, loads
    const uint4 lo = blk[0];
    const uint4 hi = blk[sh + need > 16 ? 1 : 0];
    // dwords w[d .. d + 4] of the 32-B pair, d = sh >> 2, selected without indexing
    const int d = sh >> 2;
    const uint32_t w0 = lo.x, w1 = lo.y, w2 = lo.z, w3 = lo.w, w4 = hi.x, w5 = hi.y, w6 = hi.z, w7 = hi.w;
    auto pick = [&](int j) {  // w[d + j], 0 <= j <= 4
        const int i = d + j;
        return i == 0 ? w0 : i == 1 ? w1 : i == 2 ? w2 : i == 3 ? w3 : i == 4 ? w4 : i == 5 ? w5 : i == 6 ? w6 : w7;
    };
    const uint32_t s0 = pick(0), s1 = pick(1), s2 = pick(2), s3 = pick(3), s4 = pick(4);
    const uint32_t bs = (uint32_t)(sh & 3);
    uint32_t o[4] = {__builtin_amdgcn_alignbyte(s1, s0, bs), __builtin_amdgcn_alignbyte(s2, s1, bs),
                     __builtin_amdgcn_alignbyte(s3, s2, bs), __builtin_amdgcn_alignbyte(s4, s3, bs)};
    if (need < 16) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int nb = min(max(need - 4 * q, 0), 4);
            o[q] &= nb == 4 ? 0xFFFFFFFFu : ((1u << (8 * nb)) - 1u);
        }
    }
    return make_uint4(o[0], o[1], o[2], o[3]);
}

typedef unsigned short ps_u16x2 __attribute__((ext_vector_type(2)));
// high 32 bits of the 48-bit product of two 24-bit operands (v_mul_hi_u32_u24)
__device__ __forceinline__ uint32_t mulhi24(uint32_t a, uint32_t b) {
    return (uint32_t)(((uint64_t)(a & 0xFFFFFFu) * (uint64_t)(b & 0xFFFFFFu)) >> 32);
}

#ifndef PS_TIMING  // 1: per-phase s_memtime sums of k_pyr_stream's waves (experiment builds only)
#define PS_TIMING 0
#endif
#if PS_TIMING
__device__ unsigned long long g_pstime[32];
#define PS_T(v) const unsigned long long v = __builtin_amdgcn_s_memtime()
#else
#define PS_T(v)
#endif
// rounds[n]: per level lo | cnt << 12 | (first stage entry) << 18 (L words), then the round's
// first row entry in rowEntries and the round's entry count
#ifndef PS_WAVES
#define PS_WAVES 8  // waves per SIMD the register allocation targets (two workgroups per CU)
#endif
#define PS_LB 4  // level-0 units per loader lane in flight at once
__global__ void __launch_bounds__(PS_THREADS) __attribute__((amdgpu_waves_per_eu(PS_WAVES)))
k_pyr_stream(const uint8_t* __restrict__ imgs, int stride, long long fpitch, uint8_t* __restrict__ pyr,
             const uint32_t* __restrict__ colWords, const uint4* __restrict__ rowEntries,
             const StreamLevel* __restrict__ slv, const uint32_t* __restrict__ rounds, StreamGeom sg,
             int* __restrict__ cellCount, int nCells) {
    extern __shared__ __attribute__((aligned(16))) uint8_t s_ring[];
    const int b = blockIdx.x, tid = threadIdx.x;
    // the frame's per-cell FAST counters for k_fast (when this launch is followed by the rest of
    // the extraction: one memset launch fewer)
    if (cellCount)
        for (int i = tid; i < nCells; i += PS_THREADS) cellCount[(long long)b * nCells + i] = 0;
    const int rw = sg.L + 2;  // words per round record
    for (int i = tid; i < sg.colWords; i += PS_THREADS) ((uint32_t*)(s_ring + sg.colOff))[i] = colWords[i];
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    // The first PS_LOADERS waves are loaders: during round n they bring the level-0 rows and
    // the row entries of round n+1 into the ring (whose capacity covers one round ahead) and
    // the other stage, while every other wave builds its level's rows of round n; one barrier
    // per round hands both over.  Builder waves hold no prefetch registers.
    if (wave < PS_LOADERS) {
        const uint8_t* img = imgs + (long long)b * fpitch;
        const int w0 = slv[0].w, r0Off = slv[0].ringOff, r0Pitch = slv[0].ringPitch;
        for (int n = 0; n <= sg.nRounds; ++n) {
            if (n < sg.nRounds) {
                const uint32_t e = rounds[n * rw];
                const int lo = e & 0xFFF, units = (int)((e >> 12) & 0x3F) * sg.u0;
                for (int i0 = tid; i0 < units; i0 += PS_LB * 64 * PS_LOADERS) {
                    uint4 pf[PS_LB];
#pragma unroll
                    for (int k = 0; k < PS_LB; ++k) {
                        const int i = i0 + k * 64 * PS_LOADERS;
                        if (i < units) {
                            const int r = (int)__umulhi((uint32_t)i, sg.u0m), u = i - r * sg.u0;
                            pf[k] = load_unit16(img + (long long)(lo + r) * stride + 16 * u, w0 - 16 * u, sg.align);
                        }
                    }
#pragma unroll
                    for (int k = 0; k < PS_LB; ++k) {
                        const int i = i0 + k * 64 * PS_LOADERS;
                        if (i < units) {
                            const int r = (int)__umulhi((uint32_t)i, sg.u0m), u = i - r * sg.u0;
                            *(uint4*)(s_ring + r0Off + ((lo + r) % sg.cap0) * r0Pitch + 16 * u) = pf[k];
                        }
                    }
                }
            }
            lds_barrier();  // round n's data is in LDS (n = 0: before the first round)
        }
        return;
    }
    // builder waves: this wave's level (host-assigned wave groups) and its column units
    int myL = 0;
    for (int l = 0; l < sg.L; ++l)
        if (wave >= slv[l].waveStart && wave < slv[l].waveStart + slv[l].nWaves) myL = l;
    const int ws = slv[myL].waveStart, nWaves = slv[myL].nWaves;
    const bool idle = wave < ws || wave >= ws + nWaves;  // a wave no level needed
    const int nq = slv[myL].nq, w = slv[myL].w, colOff = slv[myL].colOff;
    uint8_t* D = pyr + slv[myL].base + (long long)b * slv[myL].fstride;
    const int ql = (wave - ws) * 64 + lane, qs = 64 * nWaves;
    // a level >= 1 column quad: its four columns' source offsets, weights and flags
    struct QuadCols {
        int sx[4];
        uint32_t ap[4], live;  // ap = a0 | a1 << 16 (v_dot2 operand)
        uint32_t simd;
        bool allSimd;
        uint32_t hmask;
        uint32_t simdBytes;  // 0xFF in the byte of every SSE2 column (the others: the scalar tail)
    };
    auto decode_quad = [&](const uint4 cw) {
        // column words: sx | a1 << 12 | (a0 - 2047 + a1) << 24 | simd << 26 | live << 27
        QuadCols Q;
        const uint32_t cc[4] = {cw.x, cw.y, cw.z, cw.w};
        Q.live = 0;
        Q.simd = 0;
        Q.simdBytes = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            Q.sx[j] = (int)(cc[j] & 0xFFFu);
            const uint32_t a1 = (cc[j] >> 12) & 0xFFFu;
            Q.ap[j] = (2047u + ((cc[j] >> 24) & 3u) - a1) | (a1 << 16);
            if (cc[j] & (1u << 26)) Q.simd |= 1u << j, Q.simdBytes |= 0xFFu << (8 * j);
            if (cc[j] & (1u << 27)) Q.live |= 0xFFu << (8 * j);
        }
        Q.allSimd = Q.simd == 0xFu;
        Q.hmask = Q.allSimd ? 0xFFFFFFF0u : 0xFFFFFFFFu;  // (H >> 4) << 4 on all-SSE2 quads
        return Q;
    };
    auto build_quad = [&](const int q, const QuadCols& Q, const uint4* E, const int cnt) {
        const int* sx = Q.sx;
        const uint32_t* ap = Q.ap;
        const uint32_t live = Q.live, hmask = Q.hmask;
        const bool allSimd = Q.allSimd;
        // the level's scalar-tail columns (VResizeLinear's columns past the SSE2 body: one or two
        // quads per level) make their wave take the mixed path below for every row; the other
        // waves run the all-SSE2 formula alone (wave-uniform: no divergent path per row)
        const bool waveTail = __ballot(!allSimd) != 0ull;
        const uint32_t simdBytes = Q.simdBytes;
        // HResizeLinear of the source row at LDS address `ra`: H = S[sx] a0 + S[sx+1] a1
        // (a1 == 0 where OpenCV reads S[sx] only: the byte after it is multiplied by 0; it
        // lies in the ring row's slack or the next LDS row, never outside the allocation).
        // On all-SSE2 quads h keeps (H >> 4) << 4 = H & ~15 for the v_mul_hi_u32_u24 below.
        auto hrow = [&](uint32_t ra, uint32_t* hh) {
            const uint8_t* R = s_ring + ra;
            uint32_t lo8[4], hi8[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                lo8[j] = R[sx[j]];
                hi8[j] = R[sx[j] + 1];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t H = __builtin_amdgcn_udot2(__builtin_bit_cast(ps_u16x2, lo8[j] | (hi8[j] << 16)),
                                                          __builtin_bit_cast(ps_u16x2, ap[j]), 0u, false);
                hh[j] = H & hmask;
            }
        };
        const int cx = 4 * q - EDGE;
        const bool roi = cx >= 0 && cx < w;
        // one output row from its two source rows' horizontal sums hA (row s0) and hB (row s1)
        auto vrow = [&](const uint4 e0, const uint4 e1, const uint32_t* hA, const uint32_t* hB) {
            uint32_t word = 0;
            if (!waveTail) {
                // VResizeLinearVec_32s8u: ((H >> 4) * b) >> 16 per term = the high 32 bits of
                // (H & ~15) * (b << 12) (both < 2^24), + 2 >> 2
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    word |= ((mulhi24(hA[j], e0.z) + mulhi24(hB[j], e0.w) + 2u) >> 2) << (8 * j);
            } else {
                // both formulas for every column, the byte per column by one v_bfi (the branchy
                // per-column select cost the tail's wave both paths every row: k_pyr_stream 316 ->
                // 284 us c3 without it, timing-only ablation): SSE2 on H & ~15 (a tail quad's sums
                // are unmasked), the scalar VResizeLinear (H0 b0 + H1 b1 + 2^21) >> 22 on H
                const uint32_t b0 = e0.z >> 12, b1 = e0.w >> 12;
                uint32_t ws = 0, wc = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    ws |= ((mulhi24(hA[j] & ~15u, e0.z) + mulhi24(hB[j] & ~15u, e0.w) + 2u) >> 2) << (8 * j);
                    wc |= ((__umul24(hA[j], b0) + __umul24(hB[j], b1) + (1u << 21)) >> 22) << (8 * j);
                }
                word = bfi(simdBytes, ws, wc);
            }
            word &= live;
            // wave-uniform row base (SGPRs) + the lane's 32-bit offset: no 64-bit VALU address
            // add per store and row (nothing in this kernel reads the pyramid back)
            const uint32_t qo = 4u * (uint32_t)q;
            auto store_row = [&](uint32_t off) {
                asm volatile("global_store_dword %0, %1, %2" ::"v"(qo), "v"(word), "s"(D + off) : "memory");
            };
            store_row(e1.y);
            if (e1.z != 0xFFFFFFFFu) store_row(e1.z);
            if (e1.w != 0xFFFFFFFFu) store_row(e1.w);
            if (e1.x != 0xFFFFFFFFu && roi) *(uint32_t*)(s_ring + e1.x + cx) = word;
        };
        // Rows in pairs with the source roles alternating: even rows read (hP, hQ), odd rows
        // (hQ, hP).  A downscale step's next row starts at this row's second source row (held
        // in the set the next row reads first), so only the other set is recomputed, and no
        // row ever copies sums between register sets.  (tP / tQ: the rows they hold.)
        uint32_t tP = 0xFFFFFFFFu, tQ = 0xFFFFFFFFu;
        uint32_t hP[4] = {0u, 0u, 0u, 0u}, hQ[4] = {0u, 0u, 0u, 0u};
        for (int k = 0; k < cnt; k += 2) {
            {
                const uint4 e0 = E[2 * k], e1 = E[2 * k + 1];
                if (tP != e0.x) hrow(e0.x, hP), tP = e0.x;
                if (tQ != e0.y) hrow(e0.y, hQ), tQ = e0.y;
                vrow(e0, e1, hP, hQ);
            }
            if (k + 1 < cnt) {
                const uint4 e0 = E[2 * k + 2], e1 = E[2 * k + 3];
                if (tQ != e0.x) hrow(e0.x, hQ), tQ = e0.x;
                if (tP != e0.y) hrow(e0.y, hP), tP = e0.y;
                vrow(e0, e1, hQ, hP);
            }
        }
    };
    // a level whose quads fit one pass of its waves (every level of 640-px frames): each lane's
    // quad decoded once for the whole kernel instead of once per round
    const bool hoisted = myL > 0 && !idle && nq <= qs;
    lds_barrier();  // the column words are in LDS
    QuadCols col0{};
    if (hoisted) col0 = decode_quad(((const uint4*)(s_ring + colOff))[min(ql, nq - 1)]);
#if PS_TIMING
    unsigned long long acc[5] = {0, 0, 0, 0, 0};
#endif
    for (int n = 0; n < sg.nRounds; ++n) {
        PS_T(t1);
        const uint32_t e = idle ? 0u : rounds[n * rw + myL];
        const int cnt = (e >> 12) & 0x3F;
        // the level's row entries of this round (scalar loads: lgkmcnt, never behind stores):
        // {source row 0, source row 1 (LDS addresses), b0 << 12, b1 << 12, own ring row (LDS
        //  address, ~0u: none), padded-row offset, top mirror offset, bottom mirror offset (~0u: none)}
        const uint4* E = rowEntries + 2 * ((int)rounds[n * rw + sg.L] + (int)(e >> 18));
        if (cnt > 0 && myL == 0) {
            // padded level-0 rows from the ring (k_pyr0's copyMakeBorder), 16 B per unit
            for (int c = ql; c < nq; c += qs) {
                const int px = 16 * c;
                const bool inner = px >= EDGE && px <= w;
                for (int k = 0; k < cnt; ++k) {
                    const uint4 e0 = E[2 * k], e1 = E[2 * k + 1];
                    const uint8_t* R = s_ring + e0.x;
                    uint4 v;
                    if (inner) {
                        v = *(const uint4*)(R + px - EDGE);
                    } else if (px == 0) {
                        // left border: bytes R[16], R[15], .. R[1] (reflect-101 of -16 .. -1),
                        // the aligned dwords R[0..19] reversed by v_perm
                        const uint4 a = *(const uint4*)R;
                        const uint32_t a4 = *(const uint32_t*)(R + 16);
                        v = make_uint4(__builtin_amdgcn_perm(a4, a.w, 0x01020304u), __builtin_amdgcn_perm(a.w, a.z, 0x01020304u),
                                       __builtin_amdgcn_perm(a.z, a.y, 0x01020304u), __builtin_amdgcn_perm(a.y, a.x, 0x01020304u));
                    } else if ((w & 15) == 0 && px == w + EDGE) {
                        // right border of a 16-aligned row: R[w-2], R[w-3], .. R[w-17], from the
                        // aligned dwords R[w-32 .. w-1] (E0 .. E7) reversed by v_perm
                        const uint4 lo = *(const uint4*)(R + w - 32), hi = *(const uint4*)(R + w - 16);
                        v = make_uint4(__builtin_amdgcn_perm(hi.w, hi.z, 0x03040506u), __builtin_amdgcn_perm(hi.z, hi.y, 0x03040506u),
                                       __builtin_amdgcn_perm(hi.y, hi.x, 0x03040506u), __builtin_amdgcn_perm(hi.x, lo.w, 0x03040506u));
                    } else {  // a border unit: single-bounce reflect-101 (w >= 17); all 16
                              // reads unconditional (clamped), so they issue back to back.  (The
                              // compiler hoists the 16 indices out of the row loop for every unit;
                              // keeping them in this branch measured slower: the border lanes share
                              // the level-0 wave, which then ran them for every row, 0.394 vs
                              // 0.380 ms c3)
                        const int pxo = px;
                        uint32_t by[16];
#pragma unroll
                        for (int j = 0; j < 16; ++j) {
                            const int X = min(pxo + j - EDGE, w + EDGE - 1);
                            by[j] = R[X < 0 ? -X : (X >= w ? 2 * w - 2 - X : X)];
                        }
                        uint32_t w4[4];
#pragma unroll
                        for (int q4 = 0; q4 < 4; ++q4) {
                            uint32_t word = 0;
#pragma unroll
                            for (int j = 0; j < 4; ++j) word |= (pxo + 4 * q4 + j < w + 2 * EDGE ? by[4 * q4 + j] : 0u) << (8 * j);
                            w4[q4] = word;
                        }
                        v = make_uint4(w4[0], w4[1], w4[2], w4[3]);
                    }
                    *(uint4*)(D + e1.y + px) = v;
                    if (e1.z != 0xFFFFFFFFu) *(uint4*)(D + e1.z + px) = v;
                    if (e1.w != 0xFFFFFFFFu) *(uint4*)(D + e1.w + px) = v;
                }
            }
        } else if (cnt > 0) {
            // level myL from the ring of level myL-1: per column unit, the round's rows in order
            if (hoisted) {
                if (ql < nq) build_quad(ql, col0, E, cnt);
            } else {
                const uint4* C = (const uint4*)(s_ring + colOff);
                for (int q = ql; q < nq; q += qs) build_quad(q, decode_quad(C[q]), E, cnt);
            }
        }
        PS_T(t2);
        lds_barrier();
#if PS_TIMING
        PS_T(t3);
        acc[1] += t2 - t1;
        acc[2] += t3 - t2;
#endif
    }
#if PS_TIMING
    if (lane == 0) {
        for (int k = 0; k < 5; ++k) atomicAdd(&g_pstime[k], acc[k]);
        atomicAdd(&g_pstime[5], 1ull);
        if (!idle) {
            atomicAdd(&g_pstime[8 + myL], acc[1]);
            atomicAdd(&g_pstime[24 + myL], 1ull);
        }
    }
#endif
}

// ---- FAST on the levels: per-tile detection + the per-cell non-max suppression --------------
// ComputeKeyPoints runs cv::FAST(cellImage, keys, fastTh, true) on every cell ROI of every
// level (ORBextractor.cc:560-607).  A cell's FAST sees its ROI only: detection rows / cols
// [3, n-3) of the ROI = the cell's detection area, and NMS neighbours outside that area count
// as 0.  Corner-ness and score are properties of the pixel alone, so one pass
// over each level's detection region [16, detX1) x [16, detY1) (the union of the cells'
// areas) finds every cell's corners; the NMS then applies each cell's own boundary.
//
// k_fast: one 256-thread workgroup per detection tile of a level, per frame.  A tile is tw4
// dwords (TW = 4 tw4 <= 256 columns, x0 a multiple of 4) by th rows: the level's detection width
// is split evenly into ceil(width / 256) tiles, so few lanes fall outside the region, and th is
// sized so the staged tile and the strength plane fit their LDS budgets.  The tile with its 1-px
// strength ring is one flattened (plane row, dword) index space of (th + 2) x (tw4 + 2) dwords
// (ring rows -1 and th; ring dwords -1 and tw4 contribute their one adjacent pixel), dealt to
// the 4 waves 64 dwords at a time:
//   (1) stage rows y0-4 .. y0+th+3, columns from the 16-aligned column at or below x0-8 to
//       x0+TW+7, into LDS with 16-byte loads, all in flight before any LDS write;
//   (2) compass pre-filter of cv::FAST (a 9-arc always covers two cyclically adjacent points of
//       {0, 4, 8, 12}) on the lane's 4 pixels, packed 16-bit; dwords with a survivor inside the
//       level's detection region are queued per wave;
//   (3) the queue: expanded to one pixel per slot, the exact strength S (score = S - 1) in full
//       64-pixel passes, `S > fastTh ? S : 0` into an LDS strength plane (a pixel the compass
//       rejects is no corner at fastTh and keeps 0: the NMS only reads S > fastTh);
//   (4) after one barrier, the plane's interior corners (flattened again) and the per-cell 3x3
//       strict NMS; survivors are appended to their cell's candidate slots as
//       ((S-1) << 24) | (y << 12) | x (k_select restores raster order).
// The 7x7 blur of the descriptors is not materialised: k_orient_desc evaluates it at the
// rBRIEF sample points from a raw window (ORBextractor.cc:760).
#ifndef KF_TIMING  // 1: per-phase s_memtime sums of k_fast's waves (experiment builds only)
#define KF_TIMING 0
#endif
#if KF_TIMING
__device__ unsigned long long g_kftime[8];
#define KF_T(i) const unsigned long long kft##i = __builtin_amdgcn_s_memrealtime()
#else
#define KF_T(i)
#endif
#define KF_DPL 2  // adjacent dwords per lane and step of the compass loop (the groups' dword pairs are
                  // read as ds_read_b64)
__global__ void __launch_bounds__(256) k_fast(const uint8_t* __restrict__ pyr, Geom g,
                                                      const FastTile* __restrict__ tiles,
                                                      uint32_t* __restrict__ cand, int* __restrict__ cellCount) {
    __shared__ __attribute__((aligned(16))) uint8_t s_in[FT_IN_BYTES];
    __shared__ __attribute__((aligned(16))) uint8_t s_S[FT_S_BYTES];
    // per-wave lists; the last slot of each is a trash slot, so ballot-compacted appends store
    // unconditionally (no exec-mask branch per append)
    __shared__ uint16_t s_q[4][FT_Q + 2];
    __shared__ uint16_t s_px[4][FT_CQ + 2];  // a chunk's pixels, compacted in place to its corners
    __shared__ uint16_t s_cl[4][FT_CL + 2];  // the wave's interior corners (tile row << 9 | tile column)
    __shared__ int s_ovf;                    // a wave's corner list overflowed: scan the plane
    __shared__ uint8_t s_cm[FT_TW_MAX / 4 + 3 + KF_DPL];  // per flattened dword column: its detection
                                                           // pixels (0 past the ring; index
                                                           // dc + 1, 0 at dc = -1)
    KF_T(0);
    // (plain block order: an XCD-aware order, vertically adjacent tiles on one XCD so their halo
    // rows hit in its L2, measured slower -- 0.646 vs 0.574 ms c3: the halo is not what binds)
    FastTile t = tiles[blockIdx.x];
    const int b = blockIdx.y;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    // the level's geometry and the tile in SGPRs for the whole kernel (read through a reference
    // into the kernarg block, the compiler re-issued dependent s_loads inside the loops); the
    // empty asm makes the copies opaque, so they cannot be rematerialised
    LevelGeom lg = g.lv[t.level];
    asm volatile("" : "+s"(lg.w), "+s"(lg.h), "+s"(lg.pitch), "+s"(lg.ph), "+s"(lg.detX1), "+s"(lg.detY1),
                 "+s"(lg.rows), "+s"(lg.cols));
    asm volatile("" : "+s"(lg.cellW), "+s"(lg.cellH), "+s"(lg.cellWm), "+s"(lg.cellHm), "+s"(lg.cell0),
                 "+s"(lg.base), "+s"(lg.fstride), "+s"(lg.candBase), "+s"(lg.capMax));
    asm volatile("" : "+s"(t.x0), "+s"(t.y0), "+s"(t.tw4), "+s"(t.th), "+s"(t.sp), "+s"(t.sx), "+s"(t.rcpF),
                 "+s"(t.rcpI));
    const int fw = t.tw4 + 2;          // flattened row width (dwords): ring dword -1 .. tw4
    const int spw = 4 * t.tw4 + 8;     // strength-plane pitch: tile columns -4 .. TW+3
    {  // (1) stage: padded rows y0+12 .. (clipped to the buffer), t.sp bytes from the 16-aligned
       // padded column x0+16-sx (clipped to the row)
        const uint8_t* src = pyr + lg.base + (long long)b * lg.fstride;
        const int pr0 = t.y0 - 4 + EDGE, pc0 = t.x0 - t.sx + EDGE;
        const int upr = t.sp >> 4;
        const int rows = min(t.th + 8, lg.ph - pr0);
        const int units = min(upr, (lg.pitch - pc0) >> 4);
        const int nU = (t.th + 8) * upr;  // <= FT_IN_BYTES / 16
        const uint4* gs = (const uint4*)(src + (long long)pr0 * lg.pitch + pc0);
        const int gsu = lg.pitch >> 4;
        constexpr int NU = (FT_IN_BYTES / 16 + 255) / 256;
        uint4 v[NU];
#pragma unroll
        for (int k = 0; k < NU; ++k) {
            const int i = tid + 256 * k;
            const int r = (int)__umulhi((uint32_t)i, t.rcpU), u = i - r * upr;
            const bool ok = i < nU && r < rows && u < units;
            v[k] = gs[ok ? (long long)r * gsu + u : 0ll];  // every slot loads (no scratch spill)
            if (!ok) v[k] = make_uint4(0u, 0u, 0u, 0u);
        }
#pragma unroll
        for (int k = 0; k < NU; ++k) {
            const int i = tid + 256 * k;
            if (i < nU) ((uint4*)s_in)[i] = v[k];
        }
        // the strength plane zeroed with 16-B stores (FT_S_BYTES is a multiple of 16)
        const int nS = ((t.th + 2) * spw + 15) >> 4;
        for (int i = tid; i < nS; i += 256) ((uint4*)s_S)[i] = make_uint4(0u, 0u, 0u, 0u);
        if (tid == 0) s_ovf = 0;
        if (tid < fw + 3) {
            const int dc = tid - 1, X = t.x0 + 4 * (dc - 1);
            const int lo = max(dc == 0 ? 3 : 0, EDGE - X), hi = min(dc == fw - 1 ? 1 : 4, lg.detX1 - X);
            s_cm[tid] = (uint8_t)(dc >= 0 && dc < fw && lo < hi ? (((1u << hi) - 1u) & ~((1u << lo) - 1u)) : 0u);
        }
    }
    __syncthreads();
    KF_T(1);
    const int ft = g.fastTh;
    const uint32_t tt = (uint32_t)ft | ((uint32_t)ft << 16);
    uint16_t* pq = s_q[wave];
    uint16_t* px = s_px[wave];
    // pixel code = plane row << 9 | plane column (plane row = tile row + 1, plane column = tile
    // column + 1); staged byte of a pixel: row pr + 3, column sx + pc - 1
    int np = 0;
    int ncl = 0;  // the wave's corners so far (wave-uniform)
    uint16_t* cl = s_cl[wave];
    auto strength_pass = [&](int base, int n) {  // px[base .. base + n), n <= 64
        bool corner = false;
        uint16_t code = 0;
        if (lane < n) {
            const uint16_t c = px[base + lane];
            const int S = fast_strength_packed(s_in + ((c >> 9) + 3) * t.sp + t.sx + (c & 511) - 1, t.sp);
            s_S[(c >> 9) * spw + (c & 511) + 3] = (uint8_t)(S > ft ? S : 0);  // each pixel once
            // an NMS candidate: a corner inside the tile (plane rows 1 .. th, columns 1 .. TW)
            const int pr = c >> 9, pc = c & 511;
            corner = S > ft && pr >= 1 && pr <= t.th && pc >= 1 && pc <= 4 * t.tw4;
            code = (uint16_t)(((pr - 1) << 9) | (pc - 1));
        }
        const uint64_t m = __ballot(corner);
        if (corner) {
            const int ix = ncl + lanes_below(m);
            cl[ix < g.fastCl ? ix : FT_CL] = code;  // FT_CL: trash slot
        }
        ncl += __popcll(m);
    };
    // queue entry = flattened index f << 4 | mask (bit j: pixel j of dword f); f = pr * fw + dc,
    // dword dc - 1 of plane row pr, pixel j at plane column 4 dc + j - 3
    auto drain = [&](int qn) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        for (int i0 = 0; i0 < qn; i0 += 64) {
            const int i = i0 + lane;
            const uint32_t e = i < qn ? pq[i] : 0u;
            const int f = (int)(e >> 4);
            const int pr = (int)__umulhi((uint32_t)f, t.rcpF), dc = f - pr * fw;
            const uint32_t code = ((uint32_t)pr << 9) + 4u * (uint32_t)dc - 3u;
#pragma unroll
            for (int j = 0; j < 4; ++j) {  // expand the 64 entries into one pixel per slot
                const bool v = (e >> j) & 1u;
                const uint64_t m = __ballot(v);
                // every lane computes its slot, and the ballot itself selects it (one compare per bit)
                px[select_by_mask(m, FT_CQ, np + lanes_below(m))] = (uint16_t)(code + j);
                np += __popcll(m);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            // full passes from the top of the list (the next expansion overwrites what they read:
            // LDS accesses of one wave complete in issue order)
            while (np >= 64) {
                np -= 64;
                strength_pass(np, 64);
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    };
    // (2) compass pre-filter over the flattened tile + ring, 64 dwords per wave and step
#if KF_TIMING
    unsigned long long kft2 = 0;
#endif
    {
        // KF_DPL adjacent dwords (4 KF_DPL pixels) per lane and step: a group shares its left /
        // centre / right loads and the step bookkeeping (one dword per lane before: 484 -> 466 us
        // per 512 c3 frames with two, 700 -> 669 c4, 9.52 -> 8.95 ms per 4096 720p).  Group
        // index g = pr * fwg + k over the plane rows whose level row lies in the detection region
        // (only the two ring rows can fall outside, so the region test is the loop's row range);
        // group k covers dwords KF_DPL k .. KF_DPL k + KF_DPL - 1 (those past the ring, fw ..,
        // have no detection pixel: s_cm is 0 there)
        int qn = 0;
        // group kp = dwords dc = 2 kp - 1, 2 kp (kp = 0: dc = -1 is a dummy with no detection
        // pixel): with the tile's first staged byte sx = 16 or 24 (host: tile widths a multiple of
        // 8 columns) every group's pair is 8-B aligned, so its row (and the left / right
        // neighbours, up and down rows) are five ds_read_b64: a wave's 32-lane half reads 64
        // consecutive dwords, conflict-free (the dword reads at an 8-B lane stride were 2-way
        // bank conflicts: dword banks are (a / 4) mod 32, 64-bit reads' (a / 4) mod 64)
        const int iw2 = t.sp >> 3, fwg = (fw >> 1) + 1;
        const int prLo = max(0, EDGE + 1 - t.y0), prHi = min(t.th + 2, lg.detY1 + 1 - t.y0);  // wave-uniform
        const int nP = (prHi - prLo) * fwg;
        const int q256 = 256 / fwg, r256 = 256 - q256 * fwg;
        const int adStep = q256 * t.sp + 4 * KF_DPL * r256, adWrap = t.sp - 4 * KF_DPL * fwg;
        int g = wave * 64 + lane;
        int pr = g / fwg, kp = g - pr * fwg;
        pr += prLo;
        int ad = (pr + 3) * t.sp + t.sx + 8 * kp - 8;  // byte offset of the group's first dword (dc = 2 kp - 1)
        const int adSafe = 3 * t.sp + 16;
        for (int it = wave; it * 64 < nP; it = __builtin_amdgcn_readfirstlane(it + 4)) {  // wave-uniform
            const bool valid = g < nP;
            uint32_t h[KF_DPL + 2];  // dwords -1 .. KF_DPL of the group's row
            uint32_t upv[KF_DPL], dnv[KF_DPL];
            const uint2* row2 = (const uint2*)(s_in + (valid ? ad : adSafe));
            {
                const uint2 L = row2[-1], C = row2[0], R = row2[1], U = row2[-3 * iw2], D = row2[3 * iw2];
                h[0] = L.y;
                h[1] = C.x;
                h[2] = C.y;
                h[3] = R.x;
                upv[0] = U.x;
                upv[1] = U.y;
                dnv[0] = D.x;
                dnv[1] = D.y;
            }
            const int dc = valid ? 2 * kp : fw + 1;  // s_cm index of the group's first dword (0 past the ring)
            const int fq = pr * fw + 2 * kp - 1;
            // the row's dwords split once into even / odd byte lanes: a dword's q4 / q12 (pixels
            // x+3 / x-3) are the odd / even lanes of its neighbours, one v_alignbyte where they
            // straddle two dwords
            uint32_t he[KF_DPL + 2], ho[KF_DPL + 2];
#pragma unroll
            for (int j = 0; j < KF_DPL + 2; ++j) {
                he[j] = even_bytes(h[j]);
                ho[j] = odd_bytes(h[j]);
            }
            uint32_t m[KF_DPL];
#pragma unroll
            for (int j = 0; j < KF_DPL; ++j) {
                const uint32_t up = upv[j], dn = dnv[j];
                // even lanes (x, x+2): q4 = x+3, x+5 (odd bytes 3 / 1 of dwords 0 / +1), q12 = x-3, x-1
                const uint32_t pe = compass_half(he[j + 1], even_bytes(dn), __builtin_amdgcn_alignbyte(ho[j + 2], ho[j + 1], 2),
                                                 even_bytes(up), ho[j], tt);
                // odd lanes (x+1, x+3): q4 = x+4, x+6 (even bytes of +1), q12 = x-2, x (bytes 2 / 0 of -1 / 0)
                const uint32_t po = compass_half(ho[j + 1], odd_bytes(dn), he[j + 2], odd_bytes(up),
                                                 __builtin_amdgcn_alignbyte(he[j + 1], he[j], 2), tt);
                m[j] = compass_mask(pe, po) & s_cm[dc + j];
            }
            g += 256;
            kp += r256;
            pr += q256;
            ad += adStep;
            if (kp >= fwg) {
                kp -= fwg;
                pr += 1;
                ad += adWrap;
            }
            if (qn > FT_Q - 64 * KF_DPL) {
                drain(qn);
                qn = 0;
            }
#pragma unroll
            for (int j = 0; j < KF_DPL; ++j) {
                const bool v = m[j] != 0u;
                const uint64_t bm = __ballot(v);
                pq[select_by_mask(bm, FT_Q, qn + lanes_below(bm))] = (uint16_t)(((uint32_t)(fq + j) << 4) | m[j]);
                qn += (int)__popcll(bm);
            }
        }
#if KF_TIMING
        kft2 = __builtin_amdgcn_s_memrealtime();
#endif
        drain(qn);
        if (np) strength_pass(0, np);  // the remainder, < 64 pixels
    }
    if (ncl > g.fastCl && lane == 0) s_ovf = 1;
    KF_T(3);
    __syncthreads();
    KF_T(4);
    // (4) in-cell NMS.  Cell (i, j) has the detection area [16 + j*cellW, j == cols-1 ? w-16 :
    // 16 + (j+1)*cellW) in x (likewise in y), ORBextractor.cc:572-597; cell of a detection pixel:
    // ((y-16) / cellH, (x-16) / cellW) by exact reciprocal multiplies (host-checked).
    // (A 1-px cell -- a level 33 px high or wide has a 1-px detection area -- has no such
    // reciprocal: ceil(2^32 / 1) does not fit 32 bits.  The host sends 2^32 - 1 instead, and
    // umulhi(n + 1, 2^32 - 1) = n: the coordinate's origin moves by one, in an SGPR, at no VALU cost.)
    const int orgY = lg.cellHm == -1 ? EDGE - 1 : EDGE, orgX = lg.cellWm == -1 ? EDGE - 1 : EDGE;
    auto cell_row = [&](int y) { return (int)__umulhi((uint32_t)(y - orgY), (uint32_t)lg.cellHm); };
    auto cell_col = [&](int x) { return (int)__umulhi((uint32_t)(x - orgX), (uint32_t)lg.cellWm); };
    int* fcount = cellCount + (long long)b * g.nCells + lg.cell0;
    uint32_t* fcand = cand + (long long)b * g.candPerFrame + lg.candBase;
    // the tile's cells: rows ciT0 .. ciT1, columns cjT0 .. cjT0 + ncT - 1 (wave-uniform)
    const int ciT0 = cell_row(t.y0);
    const int ciT1 = cell_row(t.y0 + t.th - 1);
    const int cjT0 = cell_col(t.x0);
    const int cjT1 = cell_col(min(t.x0 + 4 * t.tw4, lg.detX1) - 1);
    const int ncT = cjT1 - cjT0 + 1, nT = (ciT1 - ciT0 + 1) * ncT;
    // The survivors' cell slots are taken per workgroup -- an LDS count per cell of the tile,
    // one global atomicAdd per cell, each survivor at the cell's base + its LDS rank -- instead of
    // one returning global atomic per survivor on the few counters of the tile's cells (their
    // same-address serialisation at L2 cost ~0.05 ms per c3 step: timing ablation `kf_noemit`,
    // profiles/r06/r06_w_summary.txt).  The counts and bases overlay s_px, the ranks s_in (both
    // free after the strength passes).
    int* s_cc = (int*)s_px[0];
    int* s_base = s_cc + 64;
    uint16_t* s_rk = (uint16_t*)s_in;
    static_assert(sizeof(s_px) >= 128 * sizeof(int) && FT_IN_BYTES >= 4 * FT_CL * 2, "the cell counts' and ranks' LDS overlays");
    auto nms_emit = [&](const uint16_t* list, int n, auto aggC) {  // list == pq, or a list disjoint from it
        constexpr bool AGG = decltype(aggC)::value;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        int sn = 0;
        for (int k0 = 0; k0 < n; k0 += 64) {
            const int k = k0 + lane;
            bool keep = false;
            uint16_t e = 0;
            if (k < n) {
                e = list[k];
                const int rt = e >> 9, ct = e & 511;
                const int X = t.x0 + ct, Y = t.y0 + rt;
                const int ci = cell_row(Y);
                const int cj = cell_col(X);
                if (ci < lg.rows && cj < lg.cols) {
                    const int xlo = EDGE + cj * lg.cellW, xhi = cj == lg.cols - 1 ? lg.w - EDGE : xlo + lg.cellW;
                    const int ylo = EDGE + ci * lg.cellH, yhi = ci == lg.rows - 1 ? lg.h - EDGE : ylo + lg.cellH;
                    // the plane holds the tile's 1-px ring, so all 9 reads are in bounds: issue
                    // them together (no per-neighbour branch), then mask the out-of-cell ones
                    const uint8_t* sp = s_S + (rt + 1) * spw + ct + 4;
                    int nbv[9];
#pragma unroll
                    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                        for (int dx = -1; dx <= 1; ++dx) nbv[(dy + 1) * 3 + dx + 1] = sp[dy * spw + dx];
                    const int S = nbv[4];
                    const bool xl = X - 1 >= xlo, xr = X + 1 < xhi, yu = Y - 1 >= ylo, yd = Y + 1 < yhi;
                    bool ok = true;
#pragma unroll
                    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                        for (int dx = -1; dx <= 1; ++dx) {
                            if (dx == 0 && dy == 0) continue;
                            const bool inCell = (dx < 0 ? xl : dx > 0 ? xr : true) & (dy < 0 ? yu : dy > 0 ? yd : true);
                            const int nb = inCell ? nbv[(dy + 1) * 3 + dx + 1] : 0;
                            ok &= S - 1 > (nb ? nb - 1 : 0);
                        }
                    keep = ok;
                }
            }
            // survivors overwrite the front of the list (k0 + 64 > sn: no unread entry is hit)
            const uint64_t m = __ballot(keep);
            pq[select_by_mask(m, FT_Q, sn + lanes_below(m))] = e;
            sn += __popcll(m);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        for (int k = lane; k < sn; k += 64) {
            const uint16_t e = pq[k];
            const int rt = e >> 9, ct = e & 511;
            const int X = t.x0 + ct, Y = t.y0 + rt;
            const int ci = cell_row(Y);
            const int cj = cell_col(X);
            if constexpr (AGG) {
                s_rk[wave * FT_CL + k] = (uint16_t)atomicAdd(&s_cc[(ci - ciT0) * ncT + (cj - cjT0)], 1);
            } else {
                const int c = ci * lg.cols + cj;
                const int S = s_S[(rt + 1) * spw + ct + 4];
                const int pos = atomicAdd(fcount + c, 1);
                if (pos < lg.capMax)
                    fcand[c * lg.capMax + pos] = ((uint32_t)(S - 1) << 24) | ((uint32_t)Y << 12) | (uint32_t)X;
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        return sn;
    };
    // the NMS on the wave's own corner list (filled by its strength passes), or, where a wave's
    // list overflowed, on the plane's interior corners (ballot-compacted, flattened over th x
    // tw4 dwords) by all waves
    if (!s_ovf && nT <= 64) {  // (workgroup-uniform)
        if (tid < 64) s_cc[tid] = 0;
        __syncthreads();
        const int sn = ncl ? nms_emit(cl, ncl, std::true_type{}) : 0;
        __syncthreads();
        if (tid < nT) {
            const int cnt = s_cc[tid];
            if (cnt) s_base[tid] = atomicAdd(fcount + (ciT0 + tid / ncT) * lg.cols + cjT0 + tid % ncT, cnt);
        }
        __syncthreads();
        for (int k = lane; k < sn; k += 64) {
            const uint16_t e = pq[k];
            const int rt = e >> 9, ct = e & 511;
            const int X = t.x0 + ct, Y = t.y0 + rt;
            const int ci = cell_row(Y);
            const int cj = cell_col(X);
            const int S = s_S[(rt + 1) * spw + ct + 4];
            const int pos = s_base[(ci - ciT0) * ncT + (cj - cjT0)] + s_rk[wave * FT_CL + k];
            if (pos < lg.capMax)
                fcand[(ci * lg.cols + cj) * lg.capMax + pos] = ((uint32_t)(S - 1) << 24) | ((uint32_t)Y << 12) | (uint32_t)X;
        }
    } else if (!s_ovf) {
        if (ncl) nms_emit(cl, ncl, std::false_type{});
    } else {
        int cn = 0;
        const int nI = t.th * t.tw4;
        for (int it = wave; it * 64 < nI; it += 4) {  // wave-uniform
            const int i = it * 64 + lane;
            uint32_t w4 = 0u;
            int r = 0, d = 0;
            if (i < nI) {
                r = (int)__umulhi((uint32_t)i, t.rcpI);
                d = i - r * t.tw4;
                w4 = *(const uint32_t*)(s_S + (r + 1) * spw + 4 + 4 * d);
            }
            if (__ballot(w4 != 0u) == 0ull) continue;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool v = ((w4 >> (8 * j)) & 0xFFu) != 0u;
                const uint64_t m = __ballot(v);
                pq[select_by_mask(m, FT_Q, cn + lanes_below(m))] = (uint16_t)((r << 9) | (4 * d + j));
                cn += __popcll(m);
            }
            if (cn > FT_Q - 256) {
                nms_emit(pq, cn, std::false_type{});
                cn = 0;
            }
        }
        if (cn) nms_emit(pq, cn, std::false_type{});
    }
#if KF_TIMING
    KF_T(5);
    if (lane == 0) {
        atomicAdd(&g_kftime[0], kft1 - kft0);
        atomicAdd(&g_kftime[1], kft2 - kft1);
        atomicAdd(&g_kftime[2], kft3 - kft2);
        atomicAdd(&g_kftime[3], kft4 - kft3);
        atomicAdd(&g_kftime[4], kft5 - kft4);
        atomicAdd(&g_kftime[5], 1ull);
    }
#endif
}

// ---- the launchers orb_hip.hip calls ---------------------------------------------------------
void orb_ilp_init() {
    hipFuncSetAttribute((const void*)k_pyr_stream, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
}

void orb_ilp_pyr_stream(int B, size_t lds, hipStream_t st, const uint8_t* imgs, int stride, long long fpitch,
                        uint8_t* pyr, const uint32_t* scol, const uint4* srows, const StreamLevel* slv,
                        const uint32_t* srounds, const StreamGeom& sg, int* cellCount, int nCells) {
    hipLaunchKernelGGL(k_pyr_stream, dim3(B), dim3(PS_THREADS), lds, st, imgs, stride, fpitch, pyr, scol, srows, slv,
                       srounds, sg, cellCount, nCells);
}

void orb_ilp_fast(int nTiles, int B, hipStream_t st, const uint8_t* pyr, const Geom& g, const FastTile* tiles,
                  uint32_t* cand, int* cellCount) {
    hipLaunchKernelGGL(k_fast, dim3(nTiles, B), dim3(256), 0, st, pyr, g, tiles, cand, cellCount);
}

// ---- the probes' readers (experiment builds) ------------------------------------------------
#if PS_TIMING
extern "C" int orb_debug_ps_timing(unsigned long long* out6) {
    ORB_HIPCHK(hipDeviceSynchronize());
    ORB_HIPCHK(hipMemcpyFromSymbol(out6, HIP_SYMBOL(g_pstime), 32 * sizeof(unsigned long long)));
    unsigned long long z[32] = {};
    ORB_HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_pstime), z, sizeof(z)));
    return ORB_OK;
}
#endif
#if KF_TIMING
// experiment builds: k_fast's per-phase s_memtime sums {stage, rows, drain, barrier, nms, waves}
extern "C" int orb_debug_kf_timing(unsigned long long* out6) {
    ORB_HIPCHK(hipDeviceSynchronize());
    ORB_HIPCHK(hipMemcpyFromSymbol(out6, HIP_SYMBOL(g_kftime), 6 * sizeof(unsigned long long)));
    unsigned long long z[8] = {};
    ORB_HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_kftime), z, sizeof(z)));
    return ORB_OK;
}
#endif
