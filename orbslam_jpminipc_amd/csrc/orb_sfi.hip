// orb_sfi.hip — ORBmatcher::SearchForInitialization (ORBmatcher.cc:598-713) on the GPU:
//   k_match_init  per frame pair (one workgroup): the window search, best / second-best distances,
//                 the ratio test, the F2 ownership replay and the orientation histogram
// with its host launcher and the three entry points of include/orb_abi.h:
// orb_search_for_initialization (host buffers, one pair), orb_search_for_initialization_batch_device
// (device buffers, P pairs) and orb_match_release_stream_scratch.
//
// Reference behaviour that lives in OpenCV 2.4 / libstdc++ / glibc is restated per
// SURVEY.md Appendix A; DESIGN.md lists every arithmetic rule and where it is pinned.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/orb_abi.h"
#include "orb_internal.h"
#include "orb_device.h"
#include "orb_rot_hist.h"

using namespace orbdev;

// ======================================================================================
// kernel
// ======================================================================================
struct MatchGeom {
    int minX, maxX, minY, maxY;
    float invW, invH;  // FRAME_GRID_COLS / (maxX - minX), FRAME_GRID_ROWS / (maxY - minY)
};

// One workgroup (KM_THREADS = 8 waves) per frame pair.
//   phase 0  F2's octave-0, in-grid keypoints — the only possible candidates of
//            GetFeaturesInArea(x, y, window, 0, 0) (Frame.cc:200-265) — are staged,
//            ranked by grid-traversal order (ix, iy, index: Frame.cc:233-258), so a slot
//            number IS the reference's candidate order; F1's octave-0 queries are listed in
//            index order.
//   phase 1  (parallel) every query's window candidates are scored; each keeps its 8
//            smallest keys (dist << KB | slot) = the reference's (distance, first-in-order).
//   phase 2  (one wave, sequential: vMatchedDistance / vnMatches21 feed later queries)
//            best = first candidate with vMatchedDistance > dist, second = the next such;
//            if a truncated top-8 holds < 2 such candidates the wave rescans the window.
//   phase 3  rotation histogram, ComputeThreeMaxima, vnMatches12 / vbPrevMatched out.
// Two instantiations of the same body, both run by k_match_init's workgroup of a pair:
//   <false>  every per-slot array in LDS (nmax octave-0 keypoints per frame, nmax <= 1024 by
//            the batch size, see orb_search_for_initialization_batch_device); a pair with more
//            returns true and is redone by
//   <true>   the large-capacity body (e.g. the reference init extractor at 1280x720:
//            nFeatures*2 = 5000, Tracking.cc:126/217, ~1086 level-0 keypoints): only the greedy
//            state (vMatchedDistance / vnMatches21, vnMatches12, bins) stays in LDS, the staged
//            descriptors / coordinates / top-8 lists live in the pair's global scratch slot
//            (L2-resident); up to 8192 keypoints per frame.
#define MATCH_TOPK 8
#ifndef KM_THREADS
#define KM_THREADS 512  // one workgroup (8 waves) per pair: at most a few pairs share a CU
#endif
#define KM_WIDE_PAIRS 256  // fewer pairs: 16-wave workgroups (phase 1: NT / 256 lanes per query)
#define MATCH_BIG_NMAX 8192
#ifndef KM_TIMING  // 1: per-phase s_memrealtime sums of k_match_init's pairs (experiment builds only)
#define KM_TIMING 0
#endif
#if KM_TIMING
__device__ unsigned long long g_kmtime[8];
#define KM_T(i) const unsigned long long kmt##i = __builtin_amdgcn_s_memrealtime()
#else
#define KM_T(i)
#endif
// Insert key into the sorted list t, keeping the smallest entries: the new t[i] is the median
// of (old t[i-1], key, old t[i]) -- one v_med3_u32 per entry, all independent (the min / max
// insertion chain was two dependent ops per entry)
__device__ __forceinline__ void topk_insert(uint32_t (&t)[MATCH_TOPK], uint32_t key) {
#pragma unroll
    for (int i = MATCH_TOPK - 1; i >= 1; --i) {
        uint32_t r;
        asm("v_med3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(t[i - 1]), "v"(key), "v"(t[i]));
        t[i] = r;
    }
    t[0] = min(t[0], key);
}

struct MatchArgs {
    const orb_keypoint_t* kps;
    const uint8_t* desc;
    const int* counts;
    int cap, nmax;
    const int* pf1;
    const int* pf2;
    MatchGeom mg;
    float nnratio;
    int checkOri;
    float r;
    float* prev;
    int* m12out;
    int* nmOut;
    int P;
    int* done;    // host call (P == 1): pinned flag the kernel sets to doneSeq once its outputs are
    int doneSeq;  // visible to the host (the caller spins on it instead of a stream synchronisation)
    int fixOff;   // LDS byte offset of the fixed-point phase 2's arrays (16-wave launches), 0: sequential
};

using orb_rot::HISTO_LENGTH;
using orb_rot::rot_bin;  // ORBmatcher.cc:664-670: the rotation's histogram bin (orb_rot_hist.h)

// Byte size of one global scratch slot of the large-capacity body (nmax slots / queries).
__host__ __device__ inline size_t match_big_slot_bytes(int cap, int nmax) {
    // d2 32 + x2,y2,a2,cell 16 per F2 slot; q2i,qx,qy,lcnt 16 per query; top-8 lists
    // (also phase 0's key scratch: max(cap, 8 nmax) u32)
    const size_t keys = (size_t)(cap > MATCH_TOPK * nmax ? cap : MATCH_TOPK * nmax);
    return ((size_t)nmax * 64 + keys * 4 + 255) & ~(size_t)255;
}

// Returns true (block-uniform) when the pair exceeded nmax and was left at -2 (-1 for BIG).
template <bool BIG, int NT>
__device__ __forceinline__ bool match_pair(const MatchArgs& A, int p, int nmax, uint8_t* __restrict__ smem,
                                           uint8_t* __restrict__ gs) {
    constexpr int KB = BIG ? 13 : 11;  // slot bits of a (distance, slot) key
    constexpr uint32_t SLOT = (1u << KB) - 1u;
    __shared__ int s_n2c, s_n1c;
    __shared__ int s_hist[32];
    __shared__ int s_ind[3];
    __shared__ int s_col[65];  // first slot of grid column cx (slots are in (cx, cy, index) order)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int cap = A.cap;
    const MatchGeom mg = A.mg;
    const float r = A.r, nnratio = A.nnratio;
    float* __restrict__ prev = A.prev;
    const int f1 = A.pf1[p], f2 = A.pf2[p];
    const int n1 = A.counts[f1], n2 = A.counts[f2];
    const orb_keypoint_t* K1 = A.kps + (long long)f1 * cap;
    const orb_keypoint_t* K2 = A.kps + (long long)f2 * cap;
    const uint32_t* D1 = (const uint32_t*)(A.desc + (long long)f1 * cap * 32);
    const uint32_t* D2 = (const uint32_t*)(A.desc + (long long)f2 * cap * 32);
    // per F2 slot: x = vMatchedDistance (low 16 bits, 0xFFFF = INT_MAX) | (vnMatches21 + 1) << 16,
    // y = the F2 keypoint index — one LDS read gives the greedy pass all it needs of a slot
    uint32_t* s_d2;
    uint2* s_st;
    float *s_x2, *s_y2, *s_qx, *s_qy, *s_a2, *s_qa = nullptr;
    int *s_cell, *s_q2i, *s_lcnt, *s_m12;
    uint32_t* s_list;
    short* s_bslot;
    if constexpr (!BIG) {
        s_d2 = (uint32_t*)smem;  // nmax x 8
        s_st = (uint2*)(s_d2 + (size_t)nmax * 8);
        s_x2 = (float*)(s_st + nmax);
        s_y2 = s_x2 + nmax;
        s_cell = (int*)(s_y2 + nmax);  // posX * 48 + posY
        s_q2i = s_cell + nmax;         // query -> i1
        s_qx = (float*)(s_q2i + nmax);
        s_qy = s_qx + nmax;
        s_a2 = s_qy + nmax;                       // F2 slot angle
        s_qa = s_a2 + nmax;                       // query angle (the F1 keypoint's)
        s_list = (uint32_t*)(s_qa + nmax);        // nmax x TOPK
        s_lcnt = (int*)(s_list + (size_t)nmax * MATCH_TOPK);
        s_m12 = s_lcnt + nmax;                    // vnMatches12 (cap)
        s_bslot = (short*)(s_m12 + cap);          // F2 slot of each accepted i1 (cap)
    } else {
        s_st = (uint2*)smem;                      // LDS: greedy state
        s_m12 = (int*)(s_st + nmax);
        s_bslot = (short*)(s_m12 + cap);
        s_d2 = (uint32_t*)gs;                     // global scratch slot
        s_x2 = (float*)(s_d2 + (size_t)nmax * 8);
        s_y2 = s_x2 + nmax;
        s_cell = (int*)(s_y2 + nmax);
        s_a2 = (float*)(s_cell + nmax);
        s_q2i = (int*)(s_a2 + nmax);
        s_qx = (float*)(s_q2i + nmax);
        s_qy = s_qx + nmax;
        s_lcnt = (int*)(s_qy + nmax);
        s_list = (uint32_t*)(s_lcnt + nmax);
    }
    uint32_t* s_key = s_list;  // phase-0 scratch (cap entries)
    KM_T(0);
    // ---- phase 0: keys in parallel, then ordered compaction ----
    // s_key[i2] = traversal key of F2 keypoint i2 or ~0 (not octave 0 / outside the grid);
    // s_m12[i1] = 1 if F1 keypoint i1 is a query (octave 0), as scratch.
    for (int i = tid; i < n2; i += NT) {
        const orb_keypoint_t kp = K2[i];
        const int px = cvt_x86(roundf((kp.x - mg.minX) * mg.invW));
        const int py = cvt_x86(roundf((kp.y - mg.minY) * mg.invH));
        const bool ok = kp.octave == 0 && !(px < 0 || px >= 64 || py < 0 || py >= 48);
        s_key[i] = ok ? (((uint32_t)(px * 48 + py) << 16) | (uint32_t)i) : 0xFFFFFFFFu;
    }
    for (int i = tid; i < n1; i += NT) s_m12[i] = K1[i].octave == 0;  // level1 > 0 -> continue (ORBmatcher.cc:615)
    if constexpr (BIG) __threadfence_block();
    __syncthreads();
    if constexpr (!BIG) {
        // both lists compacted by the whole workgroup, NT entries per round (per wave a ballot
        // count, the waves' offsets from a table of NT / 64); the single-wave loops below took
        // ~2.6 us per pair alone
        __shared__ int s_wc2[16], s_wc1[16];
        int base2 = 0, base1 = 0;
        for (int i0 = 0; i0 < max(n1, n2); i0 += NT) {
            const int i = i0 + tid;
            const uint32_t key = i < n2 ? s_key[i] : 0xFFFFFFFFu;
            const bool ok2 = key != 0xFFFFFFFFu;
            const bool ok1 = i < n1 && s_m12[i];
            const uint64_t m2 = __ballot(ok2), m1 = __ballot(ok1);
            if (lane == 0) {
                s_wc2[wave] = __popcll(m2);
                s_wc1[wave] = __popcll(m1);
            }
            __syncthreads();  // (also: every read of s_key's round precedes the writes below)
            int o2 = base2, o1 = base1, t2 = 0, t1 = 0;
            for (int w = 0; w < NT / 64; ++w) {
                const int c2 = s_wc2[w], c1 = s_wc1[w];
                if (w < wave) o2 += c2, o1 += c1;
                t2 += c2;
                t1 += c1;
            }
            if (ok2) s_key[o2 + lanes_below(m2)] = key;
            if (ok1 && o1 + lanes_below(m1) < nmax) s_q2i[o1 + lanes_below(m1)] = i;
            base2 += t2;
            base1 += t1;
            __syncthreads();
        }
        if (tid == 0) {
            s_n2c = base2;
            s_n1c = base1;
        }
    } else if (wave == 0) {  // in-place, in-order compaction (one wave: reads precede writes)
        int base = 0;
        for (int i0 = 0; i0 < n2; i0 += 64) {
            const uint32_t key = i0 + lane < n2 ? s_key[i0 + lane] : 0xFFFFFFFFu;
            const bool ok = key != 0xFFFFFFFFu;
            const uint64_t m = __ballot(ok);
            if (ok) s_key[base + lanes_below(m)] = key;
            base += __popcll(m);
        }
        if (lane == 0) s_n2c = base;
    } else if (wave == 1) {
        int base = 0;
        for (int i0 = 0; i0 < n1; i0 += 64) {
            const int i1 = i0 + lane;
            const bool ok = i1 < n1 && s_m12[i1];
            const uint64_t m = __ballot(ok);
            if (ok && base + lanes_below(m) < nmax) s_q2i[base + lanes_below(m)] = i1;
            base += __popcll(m);
        }
        if (lane == 0) s_n1c = base;
    }
    if constexpr (BIG) __threadfence_block();
    __syncthreads();
    const int n2c = s_n2c, n1c = s_n1c;
    if (n2c > nmax || n1c > nmax) {  // capacity exceeded: fall back / report, never truncate silently
        if (tid == 0) A.nmOut[p] = BIG ? -1 : -2;
        return true;
    }
    KM_T(1);
    // rank F2 candidates by traversal key -> slot.  16-wave launches with few candidates: LPK
    // adjacent lanes per key, each counting every LPK-th key, summed on DPP (one thread per key
    // counted all n2c keys).  Every global read of this stage (the candidates' records and
    // descriptors, the queries' records and positions, phase 1's query descriptors: host memory
    // in a host call) is issued before the counting, so their latencies overlap it and each other
    // instead of following one another (phase 1's then starts with its descriptors in registers;
    // with the med3 top-8 and the row-only window test, phase 1 11.2 -> 8.2 us per pair alone)
    int lpk = 1;
    if constexpr (!BIG && NT == 1024) lpk = n2c <= 256 ? 4 : n2c <= 512 ? 2 : 1;
    constexpr bool early = !BIG;
    uint32_t d1pre[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    orb_keypoint_t qkp{};
    float2 qprev = make_float2(0.f, 0.f);
    const bool qEarly = early && n1c <= NT && tid < n1c;
    if constexpr (early) {
        const int qP = tid / (NT / 256);  // phase 1's first round: NT / 256 lanes per query
        if (qP < n1c) {
            const int i1 = s_q2i[qP];
#pragma unroll
            for (int w = 0; w < 2; ++w) {
                const uint4 v4 = ((const uint4*)D1)[(long long)i1 * 2 + w];
                d1pre[4 * w] = v4.x, d1pre[4 * w + 1] = v4.y, d1pre[4 * w + 2] = v4.z, d1pre[4 * w + 3] = v4.w;
            }
        }
        if (qEarly) {
            const int i1 = s_q2i[tid];
            qkp = K1[i1];
            if (prev) qprev = *(const float2*)(prev + ((long long)p * cap + i1) * 2);
        }
    }
    for (int t0 = tid; t0 < n2c * lpk; t0 += NT) {
        const int t = t0 / lpk, sub = t0 - t * lpk;  // (lpk divides NT: a key's lanes share a wave)
        const uint32_t k = s_key[t];
        const int i2 = (int)(k & 0xFFFF);
        orb_keypoint_t kp{};
        if (sub == 0) kp = K2[i2];
        uint32_t dv[8];
#pragma unroll
        for (int w = 0; w < 8; ++w)
            if (w % lpk == sub) dv[w] = D2[(long long)i2 * 8 + w];
        int rank = 0;
        for (int u = sub; u < n2c; u += lpk) rank += s_key[u] < k;
        if constexpr (early) {
            if (lpk >= 2) rank += __builtin_amdgcn_mov_dpp(rank, 0xB1, 0xF, 0xF, false);  // quad_perm xor 1
            if (lpk >= 4) rank += __builtin_amdgcn_mov_dpp(rank, 0x4E, 0xF, 0xF, false);  // quad_perm xor 2
        }
#pragma unroll
        for (int w = 0; w < 8; ++w)
            if (w % lpk == sub) s_d2[rank * 8 + w] = dv[w];
        if (sub != 0) continue;
        s_x2[rank] = kp.x;
        s_y2[rank] = kp.y;
        s_a2[rank] = kp.angle;
        s_cell[rank] = (int)(k >> 16);
        s_st[rank] = make_uint2(0xFFFFu, (uint32_t)i2);
    }
    if (qEarly) {
        s_qx[tid] = prev ? qprev.x : qkp.x;
        s_qy[tid] = prev ? qprev.y : qkp.y;
        if constexpr (!BIG) s_qa[tid] = qkp.angle;
    }
    if (!qEarly || !early)
        for (int q = (early && n1c <= NT) ? n1c : tid; q < n1c; q += NT) {
            const int i1 = s_q2i[q];
            const orb_keypoint_t kp = K1[i1];
            s_qx[q] = prev ? prev[((long long)p * cap + i1) * 2] : kp.x;
            s_qy[q] = prev ? prev[((long long)p * cap + i1) * 2 + 1] : kp.y;
            if constexpr (!BIG) s_qa[q] = kp.angle;  // (only queries are ever accepted)
        }
    if constexpr (BIG) __threadfence_block();
    __syncthreads();
    for (int i = tid; i < n1; i += NT) {
        s_m12[i] = -1;
        s_bslot[i] = -1;
    }
    if (tid <= 64) {  // lower_bound(s_cell, tid * 48): a window's columns are one slot range
        int lo = 0, hi = n2c;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s_cell[mid] < tid * 48)
                lo = mid + 1;
            else
                hi = mid;
        }
        s_col[tid] = lo;
    }
    __syncthreads();
    // A slot in the window's column range [s_col[minCX], s_col[maxCX + 1]) already has its grid
    // column inside the window: only its grid row is tested, so the LDS body keeps the row alone
    // (no division by 48 per candidate)
    if constexpr (!BIG) {
        for (int j = tid; j < n2c; j += NT) s_cell[j] = s_cell[j] % 48;
        __syncthreads();
    }
    KM_T(2);
    // ---- phase 1: per-query top-8 (dist, order), two lanes per query (candidates j of one
    // parity each), their sorted lists merged on DPP ----
    for (int q0 = 0; q0 < n1c; q0 += NT / (NT / 256)) {
        const int q = q0 + tid / (NT / 256), sub = tid & ((NT / 256) - 1);
        const bool act = q < n1c;
        float qx = 0.f, qy = 0.f;
        int minCX = 1, maxCX = 0, minCY = 1, maxCY = 0;
        uint32_t d1[8] = {};
        if (act) {
            qx = s_qx[q];
            qy = s_qy[q];
            minCX = max(0, cvt_x86(floorf((qx - mg.minX - r) * mg.invW)));
            maxCX = min(63, cvt_x86(ceilf((qx - mg.minX + r) * mg.invW)));
            minCY = max(0, cvt_x86(floorf((qy - mg.minY - r) * mg.invH)));
            maxCY = min(47, cvt_x86(ceilf((qy - mg.minY + r) * mg.invH)));
            if (early && q0 == 0) {
#pragma unroll
                for (int w = 0; w < 8; ++w) d1[w] = d1pre[w];
            } else {
                const int i1 = s_q2i[q];
#pragma unroll
                for (int w = 0; w < 2; ++w) {  // two 16-B loads (descriptor rows are 32-B aligned)
                    const uint4 v4 = ((const uint4*)D1)[(long long)i1 * 2 + w];
                    d1[4 * w] = v4.x, d1[4 * w + 1] = v4.y, d1[4 * w + 2] = v4.z, d1[4 * w + 3] = v4.w;
                }
            }
        }
        uint32_t top[MATCH_TOPK];
#pragma unroll
        for (int k = 0; k < MATCH_TOPK; ++k) top[k] = 0xFFFFFFFFu;
        int cnt = 0;
        // the window's grid columns only (an empty column range gives j0 >= j1)
        const int j0 = s_col[min(minCX, 64)], j1 = s_col[max(maxCX + 1, 0)];
        for (int j = j0 + sub; j < j1; j += (NT / 256)) {
            // every read of the candidate issued at once (one LDS round trip per candidate, not
            // three dependent ones behind the window tests; prefetching the next candidate's
            // reads one iteration ahead measured slower: 15.8 vs 13.6 us per pair alone)
            const int cell = s_cell[j];
            const float x2 = s_x2[j], y2 = s_y2[j];
            const uint4 da = *(const uint4*)(s_d2 + j * 8), db = *(const uint4*)(s_d2 + j * 8 + 4);
            if constexpr (BIG) {
                const int cx = cell / 48, cy = cell - cx * 48;
                if (cx < minCX || cx > maxCX || cy < minCY || cy > maxCY) continue;
            } else {
                if (cell < minCY || cell > maxCY) continue;  // (the grid row)
            }
            if (fabsf(x2 - qx) > r || fabsf(y2 - qy) > r) continue;
            const int dist = __popc(d1[0] ^ da.x) + __popc(d1[1] ^ da.y) + __popc(d1[2] ^ da.z) + __popc(d1[3] ^ da.w) +
                             __popc(d1[4] ^ db.x) + __popc(d1[5] ^ db.y) + __popc(d1[6] ^ db.z) + __popc(d1[7] ^ db.w);
            topk_insert(top, ((uint32_t)dist << KB) | (uint32_t)j);
            ++cnt;
        }
        // merge with the partner lanes' lists (DPP quad_perm xor 1, then xor 2): the 8 smallest
        // of two sorted lists are min(a[i], b[7-i]) (a bitonic sequence), sorted by a 3-stage
        // bitonic merge
        uint32_t m8[MATCH_TOPK];
#pragma unroll
        for (int k = 0; k < MATCH_TOPK; ++k) m8[k] = top[k];
        auto merge_round = [&](auto ctlC) {
            constexpr int ctl = decltype(ctlC)::value;
            cnt += __builtin_amdgcn_mov_dpp(cnt, ctl, 0xF, 0xF, false);
            uint32_t o[MATCH_TOPK];
#pragma unroll
            for (int k = 0; k < MATCH_TOPK; ++k) o[k] = (uint32_t)__builtin_amdgcn_mov_dpp((int)m8[MATCH_TOPK - 1 - k], ctl, 0xF, 0xF, false);
#pragma unroll
            for (int k = 0; k < MATCH_TOPK; ++k) m8[k] = min(m8[k], o[k]);
#pragma unroll
            for (int d = 4; d >= 1; d >>= 1)
#pragma unroll
                for (int k = 0; k < MATCH_TOPK; ++k)
                    if ((k & d) == 0) {
                        const uint32_t lo = min(m8[k], m8[k + d]), hi = max(m8[k], m8[k + d]);
                        m8[k] = lo;
                        m8[k + d] = hi;
                    }
        };
        merge_round(std::integral_constant<int, 0xB1>{});
        if constexpr ((NT / 256) == 4) merge_round(std::integral_constant<int, 0x4E>{});
        if (act && sub == 0) {
#pragma unroll
            for (int k = 0; k < MATCH_TOPK; ++k) s_list[q * MATCH_TOPK + k] = m8[k];
            s_lcnt[q] = cnt;
        }
    }
    if constexpr (BIG) __threadfence_block();
    __syncthreads();
    KM_T(3);
    // ---- phase 2: the sequential greedy pass (ORBmatcher.cc:611-680) on one wave ----
    // Speculated eight queries at a time (lane 8g + c: query q0 + g, candidate c of its top-8),
    // exact: query q's outcome is fixed by its best and second live candidates (the first two of
    // its sorted top-8 whose vMatchedDistance exceeds their distance), and an accepted query
    // changes exactly one slot (its best), lowering its vMatchedDistance.  So every query of the
    // batch is decided from the batch-start state unless an earlier query of the batch accepted
    // its best or second slot (a live slot can only die; a taken best is a steal), or it needs
    // the window rescan (a truncated top-8 with < 2 live candidates); the batch commits
    // its queries before the first such one (their slots are distinct, their vnMatches21
    // predecessors precede the batch) and the next batch starts there.  A rescan query heading
    // a batch runs alone on the whole wave.
    // the exact rescan of query q0's whole window, on all 64 lanes of wave 0 (a query whose
    // truncated top-8 holds fewer than two live candidates)
    // the exact rescan of query q0's whole window on all 64 lanes of a wave: the smallest live
    // key and the second-smallest live distance (live(j, dist): candidate slot j not excluded)
    auto rescan_best = [&](const int q0, auto&& live, uint32_t& gbOut, int& contribOut) {
        const int i1 = s_q2i[q0];
        const float qx = s_qx[q0], qy = s_qy[q0];
        const int minCX = max(0, cvt_x86(floorf((qx - mg.minX - r) * mg.invW)));
        const int maxCX = min(63, cvt_x86(ceilf((qx - mg.minX + r) * mg.invW)));
        const int minCY = max(0, cvt_x86(floorf((qy - mg.minY - r) * mg.invH)));
        const int maxCY = min(47, cvt_x86(ceilf((qy - mg.minY + r) * mg.invH)));
        uint32_t d1[8];
#pragma unroll
        for (int w = 0; w < 2; ++w) {  // two 16-B loads (descriptor rows are 32-B aligned)
            const uint4 v4 = ((const uint4*)D1)[(long long)i1 * 2 + w];
            d1[4 * w] = v4.x, d1[4 * w + 1] = v4.y, d1[4 * w + 2] = v4.z, d1[4 * w + 3] = v4.w;
        }
        uint32_t lb = 0xFFFFFFFFu;
        int ls = 0x7fffffff;
        const int j1 = s_col[max(maxCX + 1, 0)];
        for (int j = s_col[min(minCX, 64)] + lane; j < j1; j += 64) {
            const int cell = s_cell[j];
            if constexpr (BIG) {
                const int cx = cell / 48, cy = cell - cx * 48;
                if (cx < minCX || cx > maxCX || cy < minCY || cy > maxCY) continue;
            } else {
                if (cell < minCY || cell > maxCY) continue;  // (the grid row)
            }
            if (fabsf(s_x2[j] - qx) > r || fabsf(s_y2[j] - qy) > r) continue;
            const int dist = hamming256(d1, s_d2 + j * 8);
            if (!live(j, dist)) continue;
            const uint32_t key = ((uint32_t)dist << KB) | (uint32_t)j;
            if (key < lb) {
                if (lb != 0xFFFFFFFFu) ls = (int)(lb >> KB);
                lb = key;
            } else if (dist < ls) {
                ls = dist;
            }
        }
        uint32_t gb = lb;
        gb = wave_min_u32(gb);
        int contrib = (lb == gb) ? ls : (lb == 0xFFFFFFFFu ? 0x7fffffff : (int)(lb >> KB));
        contrib = (int)wave_min_u32((uint32_t)contrib);  // (non-negative)
        gbOut = gb;
        contribOut = contrib;
    };
    auto rescan_query = [&](const int q0) {
        uint32_t gb;
        int contrib;
        rescan_best(q0, [&](int j, int dist) { return (int)(s_st[j].x & 0xFFFFu) > dist; }, gb, contrib);
        if (gb == 0xFFFFFFFFu) return;
        const int i1 = s_q2i[q0];
        const int rDist = (int)(gb >> KB), rSlot = (int)(gb & SLOT);
        if (rDist <= 50 && (float)rDist < (float)contrib * nnratio && lane == 0) {
            const uint2 sb = s_st[rSlot];
            const int old = (int)(sb.x >> 16) - 1;
            if (old >= 0) s_m12[old] = -1;
            s_m12[i1] = (int)(sb.y & 0x1FFFu);
            s_st[rSlot].x = (uint32_t)rDist | ((uint32_t)(i1 + 1) << 16);
            s_bslot[i1] = (short)rSlot;
        }
    };
    // Phase 2 as a fixed point (the single-pair call, 16 waves, when its arrays fit the LDS):
    // query q's decision depends only on the earlier queries' acceptances -- candidate slot s is
    // live for q iff dist < MD_q(s) = min{d_j : j < q accepted s} (vMatchedDistance as q sees
    // it) -- so every query is decided in parallel from the previous iteration's acceptances
    // until they repeat; the sequential result is the unique fixed point and is reached (after
    // iteration k the first k queries are final; SearchByProjection(local)'s resolver, orb_match).
    // Up to three acceptors per slot and iteration (more: the sequential pass below decides).
    // Final: every accepting query keeps its slot (bins count the stolen ones too), the slot's
    // last acceptor owns the match (vnMatches21).
    bool fixDone = false;
    if constexpr (!BIG) {
        if (A.fixOff) {  // (the host enables it only when every query has a thread: nmax <= NT)
            __shared__ int s_fn, s_fch, s_fovf;
            uint32_t* faB[2];
            int* fcB[2];
            faB[0] = (uint32_t*)(smem + A.fixOff);
            faB[1] = faB[0] + 3 * nmax;
            fcB[0] = (int*)(faB[1] + 3 * nmax);
            fcB[1] = fcB[0] + nmax;
            int* fdec = fcB[1] + nmax;  // per query: (dist << 16) | slot, -1 none
            int* fnew = fdec + nmax;
            uint16_t* fres = (uint16_t*)(fnew + nmax);
            for (int i = tid; i < n2c; i += NT) fcB[0][i] = 0;
            for (int i = tid; i < n1c; i += NT) fdec[i] = -1;
            if (tid == 0) s_fovf = 0;
            const int q = tid;
            const bool qin = q < n1c;
            const int cnt = qin ? s_lcnt[q] : 0;
            uint32_t el[MATCH_TOPK];
#pragma unroll
            for (int k = 0; k < MATCH_TOPK; ++k) el[k] = qin ? s_list[q * MATCH_TOPK + k] : 0xFFFFFFFFu;
            int cur = 0;
            bool conv = false;
            for (int it = 0; it < n1c + 2 && !conv; ++it) {
                const uint32_t* fa = faB[cur];
                const int* fc = fcB[cur];
                uint32_t* na = faB[cur ^ 1];
                int* nc = fcB[cur ^ 1];
                for (int i = tid; i < n2c; i += NT) nc[i] = 0;
                if (tid == 0) {
                    s_fn = 0;
                    s_fch = 0;
                }
                __syncthreads();
                auto md = [&](int sl, int qq) {  // MD_qq(sl): 0xFFFF = INT_MAX
                    int m = 0xFFFF;
                    const int c = min(fc[sl], 3);
                    for (int i = 0; i < c; ++i) {
                        const uint32_t v = fa[3 * sl + i];
                        if ((int)(v >> 9) < qq) m = min(m, (int)(v & 511u));
                    }
                    return m;
                };
                int dec = -1;
                if (qin && cnt > 0) {
                    const int k = min(cnt, MATCH_TOPK);
                    uint32_t b1 = 0xFFFFFFFFu, b2 = 0xFFFFFFFFu;
#pragma unroll
                    for (int j = 0; j < MATCH_TOPK; ++j) {
                        if (j < k && b2 == 0xFFFFFFFFu) {
                            const uint32_t e = el[j];
                            if (md((int)(e & SLOT), q) > (int)(e >> KB)) {
                                if (b1 == 0xFFFFFFFFu)
                                    b1 = e;
                                else
                                    b2 = e;
                            }
                        }
                    }
                    if (cnt > MATCH_TOPK && b2 == 0xFFFFFFFFu) {
                        fres[atomicAdd(&s_fn, 1)] = (uint16_t)q;
                        dec = -2;
                    } else if (b1 != 0xFFFFFFFFu) {
                        const int bd = (int)(b1 >> KB);
                        const int second = b2 != 0xFFFFFFFFu ? (int)(b2 >> KB) : 0x7fffffff;
                        if (bd <= 50 && (float)bd < (float)second * nnratio) dec = (bd << 16) | (int)(b1 & SLOT);
                    }
                    if (dec >= 0) {
                        const int sl = dec & 0xFFFF;
                        const int ix = atomicAdd(&nc[sl], 1);
                        if (ix < 3)
                            na[3 * sl + ix] = ((uint32_t)q << 9) | (uint32_t)(dec >> 16);
                        else
                            s_fovf = 1;
                    }
                }
                if (qin && dec != -2) fnew[q] = dec;
                __syncthreads();
                const int nres = s_fn;
                for (int rr = wave; rr < nres; rr += NT / 64) {  // exact rescans, a wave each
                    const int qq = fres[rr];
                    uint32_t gb;
                    int contrib;
                    rescan_best(qq, [&](int j, int dist) { return md(j, qq) > dist; }, gb, contrib);
                    int d2 = -1;
                    if (gb != 0xFFFFFFFFu) {
                        const int rd = (int)(gb >> KB);
                        if (rd <= 50 && (float)rd < (float)contrib * nnratio) d2 = (rd << 16) | (int)(gb & SLOT);
                    }
                    if (lane == 0) {
                        fnew[qq] = d2;
                        if (d2 >= 0) {
                            const int sl = d2 & 0xFFFF;
                            const int ix = atomicAdd(&nc[sl], 1);
                            if (ix < 3)
                                na[3 * sl + ix] = ((uint32_t)qq << 9) | (uint32_t)(d2 >> 16);
                            else
                                s_fovf = 1;
                        }
                    }
                }
                __syncthreads();
                if (qin && fnew[q] != fdec[q]) {
                    fdec[q] = fnew[q];
                    s_fch = 1;
                }
                __syncthreads();
                conv = s_fch == 0 || s_fovf != 0;
                cur ^= 1;
                __syncthreads();  // s_fch / s_fovf read by every thread before the next reset
            }
            if (conv && s_fovf == 0) {
                fixDone = true;
                // (the lists of the last iteration, faB[cur] / fcB[cur], hold the final acceptances)
                const uint32_t* fa = faB[cur];
                const int* fc = fcB[cur];
                if (qin && fdec[q] >= 0) s_bslot[s_q2i[q]] = (short)(fdec[q] & 0xFFFF);
                for (int sl = tid; sl < n2c; sl += NT) {
                    const int c = min(fc[sl], 3);
                    int owner = -1;
                    for (int i = 0; i < c; ++i) owner = max(owner, (int)(fa[3 * sl + i] >> 9));
                    if (owner >= 0) s_m12[s_q2i[owner]] = (int)(s_st[sl].y & 0x1FFFu);
                }
            }
            __syncthreads();
        }
    }
    if (!fixDone && wave == 0 && n1c > 0) {
        const int grp = lane >> 3, cand = lane & 7;
        int q0 = 0;
        while (q0 < n1c) {
            const int q = q0 + grp;
            const bool qin = q < n1c;
            // the group's count, list entry and query index read together (one LDS round trip)
            const int qc = min(q, n1c - 1);
            const int cntR = s_lcnt[qc];
            const uint32_t eR = s_list[qc * MATCH_TOPK + cand];
            const int i1q = s_q2i[qc];
            const int cnt = qin ? cntR : 0;
            const int k = min(cnt, MATCH_TOPK);
            const uint32_t e = cand < k ? eR : 0xFFFFFFFFu;
            const uint2 st = cand < k ? s_st[e & SLOT] : make_uint2(0u, 0u);
            const bool valid = cand < k && (int)(st.x & 0xFFFFu) > (int)(e >> KB);
            // the group's best (smallest live key: the lists are sorted) and second, by 8-lane
            // min reductions on DPP (quad_perm xor 1, xor 2, row_half_mirror); the best lane
            // keeps its own slot state for the commit
            const uint32_t key = valid ? e : 0xFFFFFFFFu;
            const uint32_t best = min8(key);
            const uint32_t sec = min8(valid && e != best ? e : 0xFFFFFFFFu);
            const bool rescan = cnt > MATCH_TOPK && sec == 0xFFFFFFFFu;  // < 2 live in a truncated list
            const int second = sec != 0xFFFFFFFFu ? (int)(sec >> KB) : 0x7fffffff;
            const int bestDist = (int)(best >> KB), bestSlot = (int)(best & SLOT);
            const bool accept = best != 0xFFFFFFFFu && !rescan && bestDist <= 50 &&
                                (float)bestDist < (float)second * nnratio;
            // first query the batch-start state cannot decide
            const uint64_t accM = __ballot(accept && cand == 0);  // bit 8g: group g accepts
            // lane 8g + c checks group c's accepted slot against query g's best and second
            // (query g's decision reads only those two slots: the rescan test included, both
            // live means >= 2 live), one ds_bpermute for the eight groups' slots
            const int bsC = __shfl(bestSlot, 8 * cand, 64);
            const bool hit = cand < grp && ((accM >> (8 * cand)) & 1ull) &&
                             ((best != 0xFFFFFFFFu && bestSlot == bsC) || (sec != 0xFFFFFFFFu && (int)(sec & SLOT) == bsC));
            const uint64_t stopM = __ballot(hit || (rescan && cand == 0));
            const int jstop = stopM ? (__ffsll((unsigned long long)stopM) - 1) >> 3 : 8;
            if (accept && valid && e == best && grp < jstop) {
                // by the best candidate's lane; distinct slots: these writes commute, and the
                // next batch's reads follow them
                const int i1 = i1q;
                const int old = (int)(st.x >> 16) - 1;  // vnMatches21[bestIdx2]
                if (old >= 0) s_m12[old] = -1;
                s_m12[i1] = (int)(st.y & 0x1FFFu);
                s_st[bestSlot].x = (uint32_t)bestDist | ((uint32_t)(i1 + 1) << 16);
                s_bslot[i1] = (short)bestSlot;
            }
            if (jstop > 0) {
                q0 += jstop;
                continue;
            }
            rescan_query(q0);
            q0 += 1;
        }
    }
    __syncthreads();
    KM_T(4);
    // ---- phase 3 ----
    if (A.checkOri) {
        if (tid < 32) s_hist[tid] = 0;
        __syncthreads();
        // rotation bin of every accepted i1, the stolen ones included (ORBmatcher.cc:664-676); only
        // queries are ever accepted, so the LDS body walks its queries (angles from LDS: s_qa /
        // s_a2, the slot kept for the output pass); the histogram is a count, so order is free
        const int nw = BIG ? n1 : n1c;
        for (int t = tid; t < nw; t += NT) {
            const int i = BIG ? t : s_q2i[t];
            const int sl = s_bslot[i];
            if (sl < 0) continue;
            atomicAdd(&s_hist[rot_bin(BIG ? K1[i].angle : s_qa[t], s_a2[sl])], 1);
        }
        __syncthreads();
        if (wave == 0) {
            // ComputeThreeMaxima (ORBmatcher.cc:1748-1789) on one wave.  The rule is
            // orb_rot::three_maxima (orb_rot_hist.h); this restates it: its strict-> insertion scan
            // keeps the three largest non-zero counts, ties in bin order, so the bins are the
            // three largest keys (count << 8 | 255 - bin) by wave-max reductions (tid 0 scanning
            // the 30 bins took ~1 us per pair)
            const int v = lane < HISTO_LENGTH ? s_hist[lane] : 0;
            const uint32_t key = v > 0 ? ((uint32_t)v << 8) | (uint32_t)(255 - lane) : 0u;
            const uint32_t k1 = ~wave_min_u32(~key);
            const uint32_t k2 = ~wave_min_u32(~(key == k1 ? 0u : key));
            const uint32_t k3 = ~wave_min_u32(~(key == k1 || key == k2 ? 0u : key));
            const int max1 = (int)(k1 >> 8), max2 = (int)(k2 >> 8), max3 = (int)(k3 >> 8);
            int ind1 = k1 ? 255 - (int)(k1 & 255u) : -1, ind2 = k2 ? 255 - (int)(k2 & 255u) : -1;
            int ind3 = k3 ? 255 - (int)(k3 & 255u) : -1;
            if (max2 < 0.1f * (float)max1) {
                ind2 = -1;
                ind3 = -1;
            } else if (max3 < 0.1f * (float)max1) {
                ind3 = -1;
            }
            if (lane == 0) {
                s_ind[0] = ind1;
                s_ind[1] = ind2;
                s_ind[2] = ind3;
            }
        }
        __syncthreads();
        const int i1x = s_ind[0], i2x = s_ind[1], i3x = s_ind[2];
        for (int t = tid; t < nw; t += NT) {
            const int i = BIG ? t : s_q2i[t];
            const int sl = s_bslot[i];
            if (sl < 0) continue;
            const int bn = rot_bin(BIG ? K1[i].angle : s_qa[t], s_a2[sl]);
            if (bn != i1x && bn != i2x && bn != i3x) s_m12[i] = -1;
        }
        __syncthreads();
    }
    int nm = 0;
    for (int i = tid; i < n1; i += NT) {
        const int m = s_m12[i];
        A.m12out[(long long)p * cap + i] = m;
        if (m >= 0) {
            nm++;
            if (prev) {  // vbPrevMatched[i1] = F2.mvKeysUn[i2].pt: the accepted slot's staged position
                const int sl = s_bslot[i];
                prev[((long long)p * cap + i) * 2] = s_x2[sl];
                prev[((long long)p * cap + i) * 2 + 1] = s_y2[sl];
            }
        }
    }
    nm = wave_total(nm);
    if (lane == 0) s_hist[wave] = nm;
    __syncthreads();
    if (tid == 0) {
        int t = 0;
#pragma unroll
        for (int w = 0; w < NT / 64; ++w) t += s_hist[w];
        A.nmOut[p] = t;
    }
#if KM_TIMING
    KM_T(5);
    if (tid == 0 && !BIG) {
        atomicAdd(&g_kmtime[0], kmt1 - kmt0);  // phase 0: keys + compaction
        atomicAdd(&g_kmtime[1], kmt2 - kmt1);  // ranking + staging
        atomicAdd(&g_kmtime[2], kmt3 - kmt2);  // phase 1
        atomicAdd(&g_kmtime[3], kmt4 - kmt3);  // phase 2
        atomicAdd(&g_kmtime[4], kmt5 - kmt4);  // phase 3 + output
        atomicAdd(&g_kmtime[5], 1ull);
        atomicAdd(&g_kmtime[6], (unsigned long long)n1c);
        atomicAdd(&g_kmtime[7], (unsigned long long)n2c);
    }
#endif
    return false;
}

// One workgroup per pair.  A pair whose F1 queries or F2 candidates exceed the LDS capacity
// A.nmax is redone in the same workgroup by the large-capacity body (nmaxBig, up to 8192
// keypoints), its staged arrays in the pair's own slot of the global scratch `big` (null when
// cap <= A.nmax: nothing can overflow).  The dynamic LDS covers both bodies' needs, so no
// second launch and nothing per call beyond this kernel.
// NT threads: KM_THREADS (8 waves) when pairs share CUs; 16 waves when each pair has a CU to
// itself (fewer pairs than KM_WIDE_PAIRS, e.g. one SearchForInitialization call): phase 1 then
// scores each query with four lanes instead of two.
template <int NT>
__global__ void __launch_bounds__(NT) k_match_init(MatchArgs A, uint8_t* __restrict__ big, int nmaxBig) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int p = blockIdx.x;
    if (match_pair<false, NT>(A, p, A.nmax, smem, nullptr) && big) {
        __syncthreads();  // the static LDS (counts, bins) is reused
        match_pair<true, NT>(A, p, nmaxBig, smem, big + (size_t)p * match_big_slot_bytes(A.cap, nmaxBig));
    }
    if (A.done) {  // (a host call's single workgroup) every wave's output stores complete, the
                   // workgroup's writes made visible to the host (system-scope release), then the flag
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (threadIdx.x == 0) publish_done(A.done, A.doneSeq);
    }
}

// ======================================================================================
// host side
// ======================================================================================
#ifndef MATCH_NMAX_NUM
#define MATCH_NMAX_NUM 9  // k_match_init's octave-0 capacity: NUM / 40 of the keypoint capacity
#endif
#ifndef MATCH_NMAX_MIN
#define MATCH_NMAX_MIN 256
#endif
static size_t match_lds_bytes(int cap, int nmax) {
    // F2 slots (desc 32 + state 8 + x,y,a,cell 16) + queries (q2i,qx,qy,angle 16 + top-8 32 +
    // cnt 4) + cap x (m12 4 + slot 2): nmax 1024 and cap 8192 fit (156 KB)
    return (size_t)nmax * (56 + 52) + (size_t)cap * 6 + 32;
}
static size_t match_big_lds_bytes(int cap, int nmax) { return (size_t)nmax * 8 + (size_t)cap * 6 + 16; }

// Global scratch of the large-capacity matcher body: one slot per pair, grow-only, one buffer per
// (device, stream) so launches on one stream reuse it in stream order and concurrent streams
// never share one.  Grown by a stream-ordered free + allocation on that stream; steady state:
// no allocator call.  Only the slots of pairs that overflow the LDS capacity are ever touched.
// The caller holds g_bigMu from the lookup until its launch is enqueued: two host threads
// sharing one stream (e.g. the null stream) then cannot interleave a grow (whose free is
// stream-ordered after the other thread's launch) between the other's lookup and launch.
static std::mutex g_bigMu;
static std::vector<std::pair<std::pair<int, hipStream_t>, std::pair<void*, size_t>>> g_big;
static int match_big_scratch_locked(hipStream_t st, size_t bytes, void** out) {
    int dev = 0;
    ORB_HIPCHK(hipGetDevice(&dev));
    for (auto& e : g_big)
        if (e.first.first == dev && e.first.second == st) {
            if (e.second.second < bytes) {
                ORB_HIPCHK(hipFreeAsync(e.second.first, st));
                e.second = {nullptr, 0};
                ORB_HIPCHK(hipMallocAsync(&e.second.first, bytes, st));
                e.second.second = bytes;
            }
            *out = e.second.first;
            return ORB_OK;
        }
    void* p = nullptr;
    ORB_HIPCHK(hipMallocAsync(&p, bytes, st));
    g_big.push_back({{dev, st}, {p, bytes}});
    *out = p;
    return ORB_OK;
}

// The batched launch; `done` / `doneSeq`: a host call's completion flag (P == 1), else null.
static int sfi_launch(const orb_keypoint_t* d_kps, const uint8_t* d_desc, const int32_t* d_counts, int cap, int P,
                      const int32_t* d_pair_f1, const int32_t* d_pair_f2, orb_frame_bounds_t bounds, float nnratio,
                      int check_ori, int window, float* d_prev_xy, int32_t* d_matches12, int32_t* d_nmatches,
                      void* stream, int* done, int doneSeq) {
    if (!d_kps || !d_desc || !d_counts || cap <= 0 || P < 0 || !d_pair_f1 || !d_pair_f2 || !d_matches12 ||
        !d_nmatches)
        return orb_internal_set_error(ORB_EINVAL, "bad arguments");
    if (((uintptr_t)d_desc & 15) != 0) return orb_internal_set_error(ORB_EINVAL, "descriptors must be 16-B aligned");
    if (P == 0) return ORB_OK;
    if (bounds.max_x <= bounds.min_x || bounds.max_y <= bounds.min_y)
        return orb_internal_set_error(ORB_EINVAL, "bad bounds");
    if (cap > MATCH_BIG_NMAX) return orb_internal_set_error(ORB_ENOTSUP, "more than 8192 keypoints per frame");
    // octave-0 keypoints per frame held in LDS by k_match_init.  The extractor keeps at most
    // mnFeaturesPerLevel[0] of them (0.217 nFeatures at scale 1.2, 8 levels), so when the pairs
    // fill the chip, 0.225 of the capacity covers its output and leaves room for two or more
    // work-groups per CU (640x480: 0.233 -> 0.129 ms for 511 pairs, 1241x376: 0.47 -> 0.26);
    // any frame beyond (another producer, another scale factor) is redone exactly by
    // the large-capacity body in the same workgroup.  Fewer pairs than CUs: one work-group per CU anyway, and the
    // full capacity spares the per-frame path the fallback scratch.
    const int capA = (cap + 3) & ~3;  // nmax a multiple of 4: k_match_init's LDS arrays 16-B aligned
    const int nmax = P < 256 ? std::min(capA, 1024)
                             : std::min({capA, 1024, std::max(MATCH_NMAX_MIN,
                                                             (int)(((long long)cap * MATCH_NMAX_NUM / 40 + 31) & ~31))});
    const int nmaxBig = std::min(cap, MATCH_BIG_NMAX);
    // the large-capacity body runs in the same workgroup: the dynamic LDS covers both
    size_t lds = std::max(match_lds_bytes(cap, nmax), cap > nmax ? match_big_lds_bytes(cap, nmaxBig) : 0);
    if (lds > 159 * 1024)  // 160 KB per CU minus the kernel's static LDS
        return orb_internal_set_error(ORB_ENOTSUP, "per-frame keypoint capacity too large for LDS");
    // the fixed-point phase 2 of the 16-wave launch: two acceptor lists (3 entries + count per
    // slot), decisions old / new and the rescan list per query, after the body's arrays
    int fixOff = 0;
    const size_t fixAt = (match_lds_bytes(cap, nmax) + 15) & ~(size_t)15;
    const size_t fixEnd = fixAt + (size_t)nmax * (2 * 16 + 8 + 2);
    const bool wide = P < KM_WIDE_PAIRS;  // 16-wave workgroups
    const int ntLaunch = wide ? 2 * KM_THREADS : KM_THREADS;
    if (wide && nmax <= ntLaunch && fixEnd <= 158 * 1024) {
        fixOff = (int)fixAt;
        lds = std::max(lds, fixEnd);
    }
    static std::once_flag attrOnce;
    std::call_once(attrOnce, [] {
        (void)hipFuncSetAttribute((const void*)k_match_init<KM_THREADS>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  159 * 1024);
        (void)hipFuncSetAttribute((const void*)k_match_init<2 * KM_THREADS>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 159 * 1024);
        (void)hipGetLastError();  // an unsupported attribute value must not surface as the launch's error
    });
    MatchGeom mg{bounds.min_x, bounds.max_x, bounds.min_y, bounds.max_y,
                 static_cast<float>(64) / static_cast<float>(bounds.max_x - bounds.min_x),
                 static_cast<float>(48) / static_cast<float>(bounds.max_y - bounds.min_y)};
    MatchArgs A{d_kps,      d_desc,    d_counts,     cap,       nmax,   d_pair_f1,         d_pair_f2,
                mg,         nnratio,   check_ori,    (float)window, d_prev_xy, d_matches12, d_nmatches,
                P,          P == 1 ? done : nullptr, doneSeq, fixOff};
    hipStream_t st = (hipStream_t)stream;
    void* big = nullptr;
    std::unique_lock<std::mutex> lk(g_bigMu, std::defer_lock);
    if (cap > nmax) {  // a pair may overflow the LDS capacity: its slot of the large-capacity scratch
        lk.lock();     // held until the launch that uses it is enqueued
        if (int r = match_big_scratch_locked(st, match_big_slot_bytes(cap, nmaxBig) * (size_t)P, &big)) return r;
    }
    if (wide)
        hipLaunchKernelGGL(k_match_init<2 * KM_THREADS>, dim3(P), dim3(2 * KM_THREADS), lds, st, A, (uint8_t*)big, nmaxBig);
    else
        hipLaunchKernelGGL(k_match_init<KM_THREADS>, dim3(P), dim3(KM_THREADS), lds, st, A, (uint8_t*)big, nmaxBig);
    ORB_HIPCHK(hipGetLastError());
    return ORB_OK;
}

extern "C" {

int orb_match_release_stream_scratch(void* stream) {
    hipStream_t st = (hipStream_t)stream;
    int dev = 0;
    ORB_HIPCHK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_bigMu);
    for (size_t i = 0; i < g_big.size(); ++i)
        if (g_big[i].first.first == dev && g_big[i].first.second == st) {
            ORB_HIPCHK(hipFreeAsync(g_big[i].second.first, st));  // after the stream's queued launches
            g_big.erase(g_big.begin() + (long)i);
            return ORB_OK;
        }
    return ORB_OK;
}

int orb_search_for_initialization_batch_device(const orb_keypoint_t* d_kps, const uint8_t* d_desc,
                                               const int32_t* d_counts, int cap, int P, const int32_t* d_pair_f1,
                                               const int32_t* d_pair_f2, orb_frame_bounds_t bounds, float nnratio,
                                               int check_ori, int window, float* d_prev_xy, int32_t* d_matches12,
                                               int32_t* d_nmatches, void* stream) {
    return sfi_launch(d_kps, d_desc, d_counts, cap, P, d_pair_f1, d_pair_f2, bounds, nnratio, check_ori, window,
                      d_prev_xy, d_matches12, d_nmatches, stream, nullptr, 0);
}

int orb_search_for_initialization(const orb_keypoint_t* kps1, const uint8_t* desc1, int n1, const orb_keypoint_t* kps2,
                                  const uint8_t* desc2, int n2, orb_frame_bounds_t bounds, float nnratio,
                                  int check_ori, int window, float* prev_xy, int32_t* matches12, int* n_matches) {
    if (n1 < 0 || n2 < 0 || !n_matches || (n1 > 0 && (!kps1 || !desc1 || !prev_xy || !matches12)) ||
        (n2 > 0 && (!kps2 || !desc2)))
        return orb_internal_set_error(ORB_EINVAL, "bad arguments");
    for (int i = 0; i < n1; ++i)
        if (kps1[i].octave < 0) return orb_internal_set_error(ORB_EINVAL, "negative octave in F1");
    *n_matches = 0;
    if (n1 == 0) return ORB_OK;
    const int cap = std::max(std::max(n1, n2), 1);
    if (n1 > MATCH_BIG_NMAX || n2 > MATCH_BIG_NMAX)
        return orb_internal_set_error(ORB_ENOTSUP, "more than 8192 keypoints in a frame");
    int dev = 0;
    ORB_HIPCHK(hipGetDevice(&dev));
    // the calling thread's context: grow-only pinned staging, its own stream (no per-call
    // allocation, no device-wide synchronisation).  The kernel reads its inputs from the pinned
    // staging and writes vnMatches12 / vbPrevMatched / nmatches back into it: no H2D or D2H
    // command (one SearchForInitialization call 64 -> 57 us at 640x480 / 1000 kp,
    // scripts/sfi_breakdown.cpp)
    OrbHostCtx* C = orb_internal_thread_ctx(dev);
    if (!C) return orb_internal_set_error(ORB_EINVAL, "device ordinal out of range");
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t oK = 0, oD = oK + al((size_t)2 * cap * sizeof(orb_keypoint_t)), oC = oD + al((size_t)2 * cap * 32),
                 oP = oC + al(6 * sizeof(int)), oM = oP + al((size_t)cap * 8), oF = oM + al((size_t)cap * 4 + 4),
                 total = oF + 256;
    if (int r = C->reserve(0, total)) return r;
    uint8_t* hs = C->pinned;
    std::memcpy(hs + oK, kps1, (size_t)n1 * sizeof(orb_keypoint_t));
    if (n2) std::memcpy(hs + oK + (size_t)cap * sizeof(orb_keypoint_t), kps2, (size_t)n2 * sizeof(orb_keypoint_t));
    std::memcpy(hs + oD, desc1, (size_t)n1 * 32);
    if (n2) std::memcpy(hs + oD + (size_t)cap * 32, desc2, (size_t)n2 * 32);
    const int hostc[6] = {n1, n2, 0, 1, 0, 0};  // counts of frames 0/1, pair (0, 1)
    std::memcpy(hs + oC, hostc, sizeof(hostc));
    std::memcpy(hs + oP, prev_xy, (size_t)n1 * 8);
    hipStream_t s = C->stream;
    int* dc = (int*)(hs + oC);
    int* dm = (int*)(hs + oM);
    // completion: the kernel's last act is a system-scope release then a flag store into the
    // staging; the call spins on the flag (~1 us after the kernel's write, where a stream
    // synchronisation takes several) and synchronises the stream only when the flag does not
    // come (an error, or a kernel beyond the bound) -- the staging is then reused by the next call
    // only after the flag: the kernel writes nothing after it
    OrbDoneFlag done;
    const int seq = done.arm(hs + oF);
    int st = sfi_launch((const orb_keypoint_t*)(hs + oK), hs + oD, dc, cap, 1, dc + 2, dc + 3, bounds, nnratio, check_ori,
                        window, (float*)(hs + oP), dm, dm + cap, s, (int*)(hs + oF), seq);
    const bool seen = st == ORB_OK && done.wait();
    const hipError_t e = seen ? hipSuccess : hipStreamSynchronize(s);
    if (st) return st;
    if (e != hipSuccess) return orb_internal_set_error(ORB_EDEVICE, std::string("match: ") + hipGetErrorString(e));
    int nm = 0;
    std::memcpy(&nm, hs + oM + (size_t)cap * 4, 4);
    if (nm < 0) return orb_internal_set_error(ORB_ENOTSUP, "more octave-0 keypoints than the matcher holds");
    std::memcpy(matches12, hs + oM, (size_t)n1 * 4);
    std::memcpy(prev_xy, hs + oP, (size_t)n1 * 8);
    *n_matches = nm;
    return ORB_OK;
}

}  // extern "C"

#if KM_TIMING
// experiment builds: k_match_init's per-phase s_memrealtime (100 MHz) sums
// {phase 0, rank, phase 1, phase 2, phase 3, pairs, queries, candidates}
extern "C" int orb_debug_km_timing(unsigned long long* out8) {
    ORB_HIPCHK(hipDeviceSynchronize());
    ORB_HIPCHK(hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_kmtime), 8 * sizeof(unsigned long long)));
    unsigned long long z[8] = {};
    ORB_HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_kmtime), z, sizeof(z)));
    return ORB_OK;
}
#endif
