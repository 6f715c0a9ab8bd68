// orb_extract.h — what the extraction units share (orb_hip.hip: the extractor handle, the C ABI
// and every kernel but two; orb_ilp.hip: k_pyr_stream and k_fast under their own scheduler
// flags): the geometry structs and size constants of orb_extract_geom.h (HIP-free, shared with
// the host planner), the device helpers used on both sides of the split, and orb_ilp.hip's launchers.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "orb_extract_geom.h"

// ---- device helpers -----------------------------------------------------------------------
// (m & a) | (~m & b) in one VALU
__device__ __forceinline__ uint32_t bfi(uint32_t m, uint32_t a, uint32_t b) {
    uint32_t r;
    asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(r) : "v"(m), "v"(a), "v"(b));
    return r;
}

// LDS-only barrier: the ring and stage hand-offs are LDS; the pyramid stores need not drain
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

typedef short i16x2 __attribute__((ext_vector_type(2)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

// Compass pre-filter of cv::FAST for the 4 pixels of a dword, in packed 16-bit arithmetic on
// the dword's even and odd bytes (pixels x, x+2 / x+1, x+3) split into u16 lanes by the caller.
// Bright: (q0 > v+t or q8 > v+t) and (q4 or q12 likewise) <=> M = min(max(q0, q8), max(q4, q12))
// > v + t; dark: m = max(min(q0, q8), min(q4, q12)) < v - t; so the pixel passes <=>
// max(M - v, v - m) > t, the sign of t - max(M - v, v - m) (all values within i16).
// Returns a 4-bit mask (bit j = pixel j passes).
__device__ __forceinline__ uint32_t compass_half(uint32_t v, uint32_t q0, uint32_t q4, uint32_t q8, uint32_t q12,
                                                 uint32_t tt) {
    const u16x2 a = __builtin_bit_cast(u16x2, q0), b = __builtin_bit_cast(u16x2, q4);
    const u16x2 d = __builtin_bit_cast(u16x2, q8), e = __builtin_bit_cast(u16x2, q12);
    const i16x2 M = __builtin_bit_cast(
        i16x2, __builtin_elementwise_min(__builtin_elementwise_max(a, d), __builtin_elementwise_max(b, e)));
    const i16x2 m = __builtin_bit_cast(
        i16x2, __builtin_elementwise_max(__builtin_elementwise_min(a, d), __builtin_elementwise_min(b, e)));
    const i16x2 vv = __builtin_bit_cast(i16x2, v);
    const i16x2 X = __builtin_elementwise_max((i16x2)(M - vv), (i16x2)(vv - m));
    return __builtin_bit_cast(uint32_t, (i16x2)(__builtin_bit_cast(i16x2, tt) - X));  // bit 15 / 31: passes
}
__device__ __forceinline__ uint32_t compass_mask(uint32_t pe, uint32_t po) {
    // bit 15 / 31 of even -> pixels 0 / 2, of odd -> pixels 1 / 3: bytes (even 1, odd 1, even 3,
    // odd 3) gathered by one v_perm, their sign bits to bit 0 of each byte, packed by one v_dot4
    const uint32_t g4 = (__builtin_amdgcn_perm(po, pe, 0x07030501u) >> 7) & 0x01010101u;
    return __builtin_amdgcn_udot4(g4, 0x08040201u, 0u, false);
}
__device__ __forceinline__ uint32_t even_bytes(uint32_t w) { return __builtin_amdgcn_perm(0u, w, 0x0c020c00u); }
__device__ __forceinline__ uint32_t odd_bytes(uint32_t w) { return __builtin_amdgcn_perm(0u, w, 0x0c030c01u); }

// ---- FAST strength --------------------------------------------------------------------------
// S(p) = 1 + cornerScore<16>(p) of cv::FAST: the largest t for which p is a corner is S - 1,
// so p is a corner at threshold t <=> S > t; records carry S - 1 as the score.
// Both sides in one packed register of two exact f16 values: lane 0 carries the dark
// contrast v - c, lane 1 the bright contrast c - v, as multiples of 2^-24 (a byte b loaded
// into a VGPR is the f16 denormal b * 2^-24, so the pair is one v_pk_add_f16 of the two
// loaded bytes, no packing; all values are integers in [-255, 255] times 2^-24, exact).  Arcs
// of 9 as windows of 3 (two v_pk_minimum3_f16 per arc, gfx950), the best arc by
// v_pk_maximum3_f16: ~45 VALU per pixel (round 2's 1024 + b normal encoding needed a shift and
// an or per circle pixel before the add: ~75; the i16 version ~150).  Cheap enough to
// run on every pre-filter survivor instead of a 9-arc test followed by a second gather for the
// corners (k_fast's queue is LDS-latency bound).
typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ int fast_strength_packed(const uint8_t* p, int TP) {
    const uint32_t v = p[0];
    // a byte b read into a VGPR is the f16 denormal b * 2^-24: (v - c, c - v) is one v_pk_add_f16
    // of the two loaded bytes with both lanes on the low halves and one side negated per lane
    // (exact: differences of denormals are exact; f16 denormals are not flushed).  The circle's
    // bytes are read from one base per row (rows y-3 .. y+3, from column x-3) with the column as
    // the ds_read immediate: seven address adds instead of one per circle point
    constexpr int kDy[16] = {3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1, 0, 1, 2, 3};
    constexpr int kDx[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
    // (the base column x-3 made opaque: the compiler otherwise re-derives the bases from p and
    // adds the negative column offsets separately, DS offsets being unsigned)
    typedef const __attribute__((address_space(3))) uint8_t* lds_u8p;
    uint32_t a0 = (uint32_t)(uintptr_t)(lds_u8p)p - 3u;
    asm volatile("" : "+v"(a0));
    lds_u8p rowp[7];
#pragma unroll
    for (int r = 0; r < 7; ++r) rowp[r] = (lds_u8p)(uintptr_t)(a0 + (uint32_t)((r - 3) * TP));
    f16x2_t d[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const uint32_t c = rowp[kDy[k] + 3][kDx[k] + 3];
        uint32_t r;
        asm("v_pk_add_f16 %0, %1, %2 op_sel_hi:[0,0] neg_lo:[0,1] neg_hi:[1,0]" : "=v"(r) : "v"(v), "v"(c));
        d[k] = __builtin_bit_cast(f16x2_t, r);
    }
    f16x2_t m3[16];
#pragma unroll
    for (int k = 0; k < 16; ++k)
        m3[k] = __builtin_elementwise_minimum(__builtin_elementwise_minimum(d[k], d[(k + 1) & 15]), d[(k + 2) & 15]);
    f16x2_t best = __builtin_elementwise_minimum(__builtin_elementwise_minimum(m3[0], m3[3]), m3[6]);
#pragma unroll
    for (int k = 1; k < 16; k += 2) {
        const f16x2_t a = __builtin_elementwise_minimum(__builtin_elementwise_minimum(m3[k], m3[(k + 3) & 15]), m3[(k + 6) & 15]);
        const f16x2_t c = k + 1 < 16 ? __builtin_elementwise_minimum(__builtin_elementwise_minimum(m3[k + 1], m3[(k + 4) & 15]), m3[(k + 7) & 15]) : a;
        best = __builtin_elementwise_maximum(__builtin_elementwise_maximum(best, a), c);
    }
    // back to integers: a positive denormal's bits are its value; a negative one (or -0) is a
    // negative i16 (sign bit set), and S <= 0 is no corner at any threshold >= 0
    const uint32_t bb = __builtin_bit_cast(uint32_t, best);
    return max((int)(short)(bb & 0xFFFFu), (int)(short)(bb >> 16));
}

// ---- orb_ilp.hip's launchers of its kernels (library-internal) -----------------------------
__attribute__((visibility("hidden"))) void orb_ilp_init();  // once per process, before the first launch
__attribute__((visibility("hidden"))) void orb_ilp_pyr_stream(int B, size_t lds, hipStream_t st, const uint8_t* imgs,
                                                             int stride, long long fpitch, uint8_t* pyr,
                                                             const uint32_t* scol, const uint4* srows,
                                                             const StreamLevel* slv, const uint32_t* srounds,
                                                             const StreamGeom& sg, int* cellCount, int nCells);
__attribute__((visibility("hidden"))) void orb_ilp_fast(int nTiles, int B, hipStream_t st, const uint8_t* pyr,
                                                       const Geom& g, const FastTile* tiles, uint32_t* cand,
                                                       int* cellCount);
