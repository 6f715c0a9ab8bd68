// orb_localmapref.hip — the local map of a tracked frame and a keyframe's covisibility, as counting over
// flat observation tables.
//
//   orb_local_map_reference        Tracking::UpdateReferenceKeyFrames (Tracking.cc:804-879),
//                                  UpdateReferencePoints (778-801) and the "already matched" pass of
//                                  SearchReferencePointsInFrustum (718-734)
//   orb_keyframe_update_connections  KeyFrame::UpdateConnections (KeyFrame.cc:332-411), without the
//                                  reverse AddConnection calls and the parent step
//
// The caller owns the map and hands over tables; nothing here mutates them.  std::map<KeyFrame*, ...>'s
// pointer order is ascending keyframe index.  Integer only: no floating point anywhere in this unit.
//
// Rules kept by every kernel: no workgroup waits for another; every loop is bounded by a size read
// before it starts; atomics only where the result does not depend on their order (counts, minima,
// maxima, bit sets); every position in an output list comes from a scan.
//
// Call 1, per chunk of frames (the chunk keeps the per-frame scratch under the byte cap):
//   k_lm_vote    one workgroup per frame: votes in packed u16 LDS counters, the voted list by a scan
//                over the table, the reference keyframe by one maximum on a packed key, the neighbour
//                step by one wave, the prefix of the local keyframes' row lengths
//   k_lm_mark    (list position x frame): atomicMin(mark[p], rank) over every entry of the local rows
//   k_lm_count   the entries whose rank won, per list position
//   k_lm_scan    one workgroup per frame: exclusive scan of those counts, the capacity decision
//   k_lm_write   the winners in keypoint order to their positions; the position replaces the rank
//   k_lm_finish  f_mp_out, seen, the keyframe list, the vote table, the info record
// Call 2: k_uc, one workgroup per keyframe: the same counters, two passes over the table (sizes, then
// a scan that writes), a bitonic sort of the (weight, index) keys in the workgroup.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <string>

#include "../../include/orb_abi.h"
#include "../../include/orb_debug.h"
#include "orb_device.h"
#include "orb_internal.h"

namespace {

using orbdev::lanes_below;
using orbdev::wave_incl_scan;

int fail(int code, const std::string& msg) { return orb_internal_set_error(code, msg); }

constexpr int LM_THREADS = 512;  // k_lm_vote, k_lm_scan, k_lm_finish, k_uc
constexpr int LM_WAVES = LM_THREADS / 64;
constexpr int LM_ROW_THREADS = 256;  // the kernels over (list position x frame)
constexpr int LM_ROW_WAVES = LM_ROW_THREADS / 64;
constexpr int LM_POS_BLOCKS = 96;  // list positions in flight per frame; the rest by stride
constexpr int UC_THRESHOLD = 15;   // KeyFrame.cc:372

// Two u16 vote counters share a dword and are bumped by atomicAdd of 1 or 1 << 16.  A frame or a
// keyframe row has at most ORB_LM_MAX_ROW entries, each entry votes at most once for a keyframe (the
// observation rows are strictly ascending), so a counter never passes ORB_LM_MAX_ROW: the low half
// cannot carry into its neighbour, and the count fits the packed keys below.
static_assert(ORB_LM_MAX_ROW < 65536, "a u16 vote counter must hold a whole row's votes without a carry");
static_assert(ORB_LM_MAX_KF <= 65536, "a keyframe index is the low 16 bits of the packed (votes, index) keys");
static_assert((long long)ORB_LM_MAX_KF * ORB_LM_MAX_ROW < (1ll << 31), "an entry's rank fits the u32 marks");
static_assert(sizeof(orb_local_map_info_t) == 28 && sizeof(orb_update_connections_info_t) == 16, "record layout");

// the table status: the larger code wins, so that atomicMax gives the same answer in any order
constexpr int TS_OK = 0, TS_ENOTSUP = 1, TS_EINVAL = 2;
__host__ __device__ inline int ts_code(int ts) { return ts == TS_EINVAL ? ORB_EINVAL : ts == TS_ENOTSUP ? ORB_ENOTSUP : ORB_OK; }

struct LmTables {
    int n_kf, n_pt, n_kf_mp, n_obs;
    const uint8_t* kf_bad;
    const int32_t *kf_mp_off, *kf_mp, *kf_cov;
    const uint8_t* pt_bad;
    const int32_t *pt_obs_off, *pt_obs_kf;
    int* tstatus;  // TS_*, written by k_lm_validate
};

struct LmArgs {
    LmTables T;
    int cap, cap_kf, cap_pt;
    const int32_t *f_mp, *counts;
    int32_t *f_mp_out, *local_kf, *local_pt;
    uint8_t* local_pt_seen;
    int32_t* kf_votes;
    orb_local_map_info_t* info;
    // per chunk: frames [f0, f0 + nf) and their scratch, indexed by the frame's place in the chunk
    int f0, nf;
    uint32_t* mark;               // nf x n_pt: 0xFFFFFFFF, then the least rank, then the output position
    int32_t *list, *rowpre, *wcnt;  // nf x n_kf each: local keyframes, row-length prefix, winners / positions
    int32_t* votes;               // nf x n_kf, only where kf_votes is asked for
    orb_local_map_info_t* rec;    // nf working records
};

struct UcArgs {
    LmTables T;
    int cap_conn, cap_ord, pmax;  // pmax: keys per keyframe in `keys`, a power of two >= n_kf
    const int32_t* kf_idx;
    int32_t *conn_kf, *conn_w, *ord_kf, *ord_w;
    orb_update_connections_info_t* info;
    int k0, nk;
    uint32_t* keys;  // nk x pmax
};

__device__ __forceinline__ uint32_t votes_of(const uint32_t* cnt, int k) { return (cnt[k >> 1] >> ((k & 1) * 16)) & 0xffffu; }
__device__ __forceinline__ void vote(uint32_t* cnt, int k) { atomicAdd(&cnt[k >> 1], 1u << ((k & 1) * 16)); }

// Exclusive prefix of `v` over the workgroup's threads in thread order, and the total; s_wave holds one
// int per wave.  Two barriers: s_wave is free again on return.
template <int WAVES>
__device__ __forceinline__ int block_excl_scan(int v, int* s_wave, int* total) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int inc = wave_incl_scan(v);
    if (lane == 63) s_wave[w] = inc;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int i = 0; i < WAVES; ++i) {
        const int t = s_wave[i];
        before += i < w ? t : 0;
        all += t;
    }
    __syncthreads();
    *total = all;
    return before + inc - v;
}

// One pass over the tables: offsets monotone and inside their arrays, rows no longer than
// ORB_LM_MAX_ROW, every index in range, every observation row strictly ascending.
__global__ void __launch_bounds__(256) k_lm_validate(LmTables T, int n_items) {
    int worst = TS_OK;
    for (long long i = blockIdx.x * 256 + threadIdx.x; i < n_items; i += gridDim.x * 256) {
        if (i < T.n_kf) {
            const int lo = T.kf_mp_off[i], hi = T.kf_mp_off[i + 1];
            if (lo < 0 || hi < lo || hi > T.n_kf_mp) worst = max(worst, TS_EINVAL);
            else if (hi - lo > ORB_LM_MAX_ROW) worst = max(worst, TS_ENOTSUP);
        }
        if (i < T.n_kf_mp) {
            const int p = T.kf_mp[i];
            if (p < -1 || p >= T.n_pt) worst = max(worst, TS_EINVAL);
        }
        if (i < T.n_kf * 10) {
            const int c = T.kf_cov[i];
            if (c < -1 || c >= T.n_kf) worst = max(worst, TS_EINVAL);
        }
        if (i < T.n_pt) {
            const int lo = T.pt_obs_off[i], hi = T.pt_obs_off[i + 1];
            if (lo < 0 || hi < lo || hi > T.n_obs) worst = max(worst, TS_EINVAL);
            else {
                int prev = -1;
                for (int e = lo; e < hi; ++e) {
                    const int k = T.pt_obs_kf[e];
                    if (k <= prev || k >= T.n_kf) worst = max(worst, TS_EINVAL);
                    prev = max(prev, k);
                }
            }
        }
    }
    if (worst != TS_OK) atomicMax(T.tstatus, worst);
}

__device__ __forceinline__ orb_local_map_info_t lm_refused(int status) {
    orb_local_map_info_t r;
    r.status = status, r.n_voted = 0, r.n_local_kf = 0, r.ref_kf = -1, r.ref_votes = 0, r.n_local_pt = 0, r.n_cleared = 0;
    return r;
}

// LDS: (n_kf + 1) / 2 packed counters, (n_kf + 31) / 32 membership words, LM_WAVES scan slots, 4 words.
__host__ __device__ inline size_t lm_cnt_words(int n_kf) { return (((size_t)n_kf + 1) / 2 + 3) & ~(size_t)3; }
__host__ __device__ inline size_t lm_bit_words(int n_kf) { return (((size_t)n_kf + 31) / 32 + 3) & ~(size_t)3; }
inline size_t lm_vote_lds(int n_kf) { return (lm_cnt_words(n_kf) + lm_bit_words(n_kf) + 16 + 4) * 4; }
inline size_t uc_lds(int n_kf) { return (lm_cnt_words(n_kf) + 16 + 4) * 4; }

__global__ void __launch_bounds__(LM_THREADS) k_lm_vote(LmArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const LmTables& T = a.T;
    uint32_t* cnt = (uint32_t*)smem;
    uint32_t* bits = cnt + lm_cnt_words(T.n_kf);
    int* s_wave = (int*)(bits + lm_bit_words(T.n_kf));
    int* s_misc = s_wave + 16;  // [0] bad input, [1] cleared, [2] best key, [3] list size
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int fl = blockIdx.x, f = a.f0 + fl;
    const int n = a.counts[f];
    {
        const int ts = *T.tstatus;
        const int st = ts != TS_OK ? ts_code(ts) : (n < 0 || n > a.cap) ? ORB_EINVAL : ORB_OK;
        if (st != ORB_OK) {
            if (tid == 0) a.rec[fl] = lm_refused(st);
            return;
        }
    }
    const int ncw = (int)lm_cnt_words(T.n_kf), nbw = (int)lm_bit_words(T.n_kf);
    for (int i = tid; i < ncw; i += LM_THREADS) cnt[i] = 0;
    for (int i = tid; i < nbw; i += LM_THREADS) bits[i] = 0;
    if (tid < 4) s_misc[tid] = 0;
    __syncthreads();

    // 1. votes (lines 808-824): a bad point does not vote and is counted as cleared
    const int32_t* mp = a.f_mp + (size_t)f * a.cap;
    for (int i = tid; i < n; i += LM_THREADS) {
        const int p = mp[i];
        if (p == -1) continue;
        if (p < -1 || p >= T.n_pt) {
            atomicOr(&s_misc[0], 1);
        } else if (T.pt_bad[p]) {
            atomicAdd(&s_misc[1], 1);
        } else {
            const int lo = T.pt_obs_off[p], hi = T.pt_obs_off[p + 1];
            for (int e = lo; e < hi; ++e) vote(cnt, T.pt_obs_kf[e]);
        }
    }
    __syncthreads();
    if (s_misc[0]) {
        if (tid == 0) a.rec[fl] = lm_refused(ORB_EINVAL);
        return;
    }

    // 2. the voted list in ascending index without the bad ones (833-848); the first strict maximum is
    // the largest (votes << 16 | 65535 - index)
    int32_t* list = a.list + (size_t)fl * T.n_kf;
    int32_t* dbg = a.votes ? a.votes + (size_t)fl * T.n_kf : nullptr;
    int nv = 0;
    uint32_t best = 0;
    for (int k0 = 0; k0 < T.n_kf; k0 += LM_THREADS) {
        const int k = k0 + tid;
        const uint32_t v = k < T.n_kf ? votes_of(cnt, k) : 0;
        if (dbg && k < T.n_kf) dbg[k] = (int32_t)v;
        const bool in = v > 0 && !T.kf_bad[k];
        int total;
        const int at = nv + block_excl_scan<LM_WAVES>(in ? 1 : 0, s_wave, &total);
        if (in) {
            list[at] = k;
            atomicOr(&bits[k >> 5], 1u << (k & 31));
            best = max(best, (v << 16) | (uint32_t)(65535 - k));
        }
        nv += total;
    }
    if (best) atomicMax((uint32_t*)&s_misc[2], best);
    __syncthreads();

    // 3. neighbours (852-876): the loop visits the voted list only (itEndKF is taken before it and the
    // reserve keeps it valid), stops once the list holds more than 80, and appends per visit the first
    // entry of the row that is neither bad nor in the list
    if (w == 0) {
        int size = nv;
        for (int i = 0; i < nv; ++i) {
            if (size > 80) break;
            const int kf = list[i];
            const int c = lane < 10 ? T.kf_cov[(size_t)kf * 10 + lane] : -1;
            const uint64_t endm = __ballot(lane < 10 && c < 0);
            const int row_end = endm ? (int)__builtin_ctzll(endm) : 10;
            bool ok = lane < row_end;
            if (ok) ok = !T.kf_bad[c] && !((__hip_atomic_load(&bits[c >> 5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >> (c & 31)) & 1u);
            const uint64_t m = __ballot(ok);
            if (m) {
                const int first = (int)__builtin_ctzll(m);
                if (lane == first) {
                    list[size] = c;
                    atomicOr(&bits[c >> 5], 1u << (c & 31));
                }
                ++size;
            }
        }
        if (lane == 0) s_misc[3] = size;
    }
    __syncthreads();
    const int nl = s_misc[3];

    // the prefix of the local keyframes' row lengths: an entry's rank is prefix + keypoint index
    int32_t* rowpre = a.rowpre + (size_t)fl * T.n_kf;
    int base = 0;
    for (int j0 = 0; j0 < nl; j0 += LM_THREADS) {
        const int j = j0 + tid;
        int len = 0;
        if (j < nl) {
            const int kf = list[j];
            len = T.kf_mp_off[kf + 1] - T.kf_mp_off[kf];
        }
        int total;
        const int ex = block_excl_scan<LM_WAVES>(len, s_wave, &total);
        if (j < nl) rowpre[j] = base + ex;
        base += total;
    }
    if (tid == 0) {
        const uint32_t b = (uint32_t)s_misc[2];
        orb_local_map_info_t r;
        r.status = ORB_OK, r.n_voted = nv, r.n_local_kf = nl;
        r.ref_kf = b ? 65535 - (int)(b & 0xffffu) : -1, r.ref_votes = (int)(b >> 16);
        r.n_local_pt = 0, r.n_cleared = s_misc[1];
        a.rec[fl] = r;
    }
}

// 4. points (782-800), first pass: the least rank of every point of the local rows
__global__ void __launch_bounds__(LM_ROW_THREADS) k_lm_mark(LmArgs a) {
    const LmTables& T = a.T;
    const int fl = blockIdx.y;
    if (a.rec[fl].status != ORB_OK) return;
    const int nl = a.rec[fl].n_local_kf;
    uint32_t* mark = a.mark + (size_t)fl * T.n_pt;
    for (int j = blockIdx.x; j < nl; j += gridDim.x) {
        const int kf = a.list[(size_t)fl * T.n_kf + j];
        const int lo = T.kf_mp_off[kf], len = T.kf_mp_off[kf + 1] - lo;
        const uint32_t base = (uint32_t)a.rowpre[(size_t)fl * T.n_kf + j];
        for (int i = threadIdx.x; i < len; i += LM_ROW_THREADS) {
            const int p = T.kf_mp[lo + i];
            if (p >= 0 && !T.pt_bad[p]) atomicMin(&mark[p], base + (uint32_t)i);
        }
    }
}

// second pass: how many entries of each local row are a first occurrence
__global__ void __launch_bounds__(LM_ROW_THREADS) k_lm_count(LmArgs a) {
    __shared__ int s_n;
    const LmTables& T = a.T;
    const int fl = blockIdx.y;
    if (a.rec[fl].status != ORB_OK) return;
    const int nl = a.rec[fl].n_local_kf;
    const uint32_t* mark = a.mark + (size_t)fl * T.n_pt;
    for (int j = blockIdx.x; j < nl; j += gridDim.x) {
        if (threadIdx.x == 0) s_n = 0;
        __syncthreads();
        const int kf = a.list[(size_t)fl * T.n_kf + j];
        const int lo = T.kf_mp_off[kf], len = T.kf_mp_off[kf + 1] - lo;
        const uint32_t base = (uint32_t)a.rowpre[(size_t)fl * T.n_kf + j];
        int mine = 0;
        for (int i = threadIdx.x; i < len; i += LM_ROW_THREADS) {
            const int p = T.kf_mp[lo + i];
            mine += (p >= 0 && !T.pt_bad[p] && mark[p] == base + (uint32_t)i) ? 1 : 0;
        }
        if (mine) atomicAdd(&s_n, mine);
        __syncthreads();
        if (threadIdx.x == 0) a.wcnt[(size_t)fl * T.n_kf + j] = s_n;
        __syncthreads();
    }
}

// the position of each local row's first winner, the point count, and whether the outputs fit
__global__ void __launch_bounds__(LM_THREADS) k_lm_scan(LmArgs a) {
    __shared__ int s_wave[16];
    const LmTables& T = a.T;
    const int fl = blockIdx.x, tid = threadIdx.x;
    if (a.rec[fl].status != ORB_OK) return;
    const int nl = a.rec[fl].n_local_kf;
    int32_t* wcnt = a.wcnt + (size_t)fl * T.n_kf;
    int base = 0;
    for (int j0 = 0; j0 < nl; j0 += LM_THREADS) {
        const int j = j0 + tid;
        const int c = j < nl ? wcnt[j] : 0;
        int total;
        const int ex = block_excl_scan<LM_WAVES>(c, s_wave, &total);
        if (j < nl) wcnt[j] = base + ex;
        base += total;
    }
    if (tid == 0) {
        a.rec[fl].n_local_pt = base;
        if (nl > a.cap_kf || base > a.cap_pt) a.rec[fl].status = ORB_ERANGE;
    }
}

// third pass: the winners in keypoint order.  The winner of p then stores its output position into
// mark[p]; a position is at most the winner's rank, which is below every losing rank of p, so a loser
// that reads mark[p] in another workgroup meanwhile still finds it different from its own rank.
__global__ void __launch_bounds__(LM_ROW_THREADS) k_lm_write(LmArgs a) {
    __shared__ int s_wave[16];
    const LmTables& T = a.T;
    const int fl = blockIdx.y, f = a.f0 + fl;
    if (a.rec[fl].status != ORB_OK) return;
    const int nl = a.rec[fl].n_local_kf;
    uint32_t* mark = a.mark + (size_t)fl * T.n_pt;
    int32_t* out_pt = a.local_pt + (size_t)f * a.cap_pt;
    uint8_t* out_seen = a.local_pt_seen + (size_t)f * a.cap_pt;
    for (int j = blockIdx.x; j < nl; j += gridDim.x) {
        const int kf = a.list[(size_t)fl * T.n_kf + j];
        const int lo = T.kf_mp_off[kf], len = T.kf_mp_off[kf + 1] - lo;
        const uint32_t base = (uint32_t)a.rowpre[(size_t)fl * T.n_kf + j];
        int at = a.wcnt[(size_t)fl * T.n_kf + j];
        for (int i0 = 0; i0 < len; i0 += LM_ROW_THREADS) {
            const int i = i0 + threadIdx.x;
            const int p = i < len ? T.kf_mp[lo + i] : -1;
            const bool win = p >= 0 && !T.pt_bad[p] &&
                             __hip_atomic_load(&mark[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == base + (uint32_t)i;
            int total;
            const int pos = at + block_excl_scan<LM_ROW_WAVES>(win ? 1 : 0, s_wave, &total);
            if (win) {
                out_pt[pos] = p;
                out_seen[pos] = 0;
                __hip_atomic_store(&mark[p], (uint32_t)pos, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            at += total;
        }
    }
}

// 1. and 5.: the frame's row with its bad points cleared, seen = 1 where the frame still holds a local
// point (718-734 with 744); the keyframe list, the vote table and the record
__global__ void __launch_bounds__(LM_THREADS) k_lm_finish(LmArgs a) {
    const LmTables& T = a.T;
    const int fl = blockIdx.x, f = a.f0 + fl, tid = threadIdx.x;
    if (tid == 0) a.info[f] = a.rec[fl];
    if (a.rec[fl].status != ORB_OK) return;
    const int nl = a.rec[fl].n_local_kf;
    const int n = a.counts[f];
    const uint32_t* mark = a.mark + (size_t)fl * T.n_pt;
    const int32_t* mp = a.f_mp + (size_t)f * a.cap;
    for (int i = tid; i < n; i += LM_THREADS) {
        int p = mp[i];
        if (p >= 0 && T.pt_bad[p]) p = -1;
        a.f_mp_out[(size_t)f * a.cap + i] = p;
        if (p >= 0) {
            const uint32_t m = mark[p];
            if (m != 0xFFFFFFFFu) a.local_pt_seen[(size_t)f * a.cap_pt + m] = 1;
        }
    }
    for (int j = tid; j < nl; j += LM_THREADS) a.local_kf[(size_t)f * a.cap_kf + j] = a.list[(size_t)fl * T.n_kf + j];
    if (a.kf_votes)
        for (int k = tid; k < T.n_kf; k += LM_THREADS) a.kf_votes[(size_t)f * T.n_kf + k] = a.votes[(size_t)fl * T.n_kf + k];
}

__device__ __forceinline__ orb_update_connections_info_t uc_record(int status, int n_conn, int n_ord, int unchanged) {
    orb_update_connections_info_t r;
    r.status = status, r.n_conn = n_conn, r.n_ord = n_ord, r.unchanged = unchanged;
    return r;
}

// KeyFrame::UpdateConnections for one keyframe per workgroup
__global__ void __launch_bounds__(LM_THREADS) k_uc(UcArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const LmTables& T = a.T;
    uint32_t* cnt = (uint32_t*)smem;
    int* s_wave = (int*)(cnt + lm_cnt_words(T.n_kf));
    int* s_misc = s_wave + 16;  // [0] n_conn, [1] at or above the threshold, [2] best key
    const int tid = threadIdx.x;
    const int ql = blockIdx.x, q = a.k0 + ql;
    const int self = a.kf_idx[q];
    {
        const int ts = *T.tstatus;
        const int st = ts != TS_OK ? ts_code(ts) : (self < 0 || self >= T.n_kf) ? ORB_EINVAL : ORB_OK;
        if (st != ORB_OK) {
            if (tid == 0) a.info[q] = uc_record(st, 0, 0, 0);
            return;
        }
    }
    const int ncw = (int)lm_cnt_words(T.n_kf);
    for (int i = tid; i < ncw; i += LM_THREADS) cnt[i] = 0;
    if (tid < 4) s_misc[tid] = 0;
    __syncthreads();

    // votes over the keyframe's points (lines 345-363): itself excluded, bad keyframes counted
    const int lo = T.kf_mp_off[self], len = T.kf_mp_off[self + 1] - lo;
    for (int i = tid; i < len; i += LM_THREADS) {
        const int p = T.kf_mp[lo + i];
        if (p < 0 || T.pt_bad[p]) continue;
        const int e0 = T.pt_obs_off[p], e1 = T.pt_obs_off[p + 1];
        for (int e = e0; e < e1; ++e) {
            const int k = T.pt_obs_kf[e];
            if (k != self) vote(cnt, k);
        }
    }
    __syncthreads();

    // sizes first: nothing is written where a capacity is too small
    int nc = 0, nt = 0;
    uint32_t best = 0;
    for (int k = tid; k < T.n_kf; k += LM_THREADS) {
        const uint32_t v = votes_of(cnt, k);
        nc += v > 0 ? 1 : 0;
        nt += v >= (uint32_t)UC_THRESHOLD ? 1 : 0;
        if (v) best = max(best, (v << 16) | (uint32_t)(65535 - k));
    }
    if (nc) atomicAdd(&s_misc[0], nc);
    if (nt) atomicAdd(&s_misc[1], nt);
    if (best) atomicMax((uint32_t*)&s_misc[2], best);
    __syncthreads();
    const int n_conn = s_misc[0], n_th = s_misc[1];
    const int n_ord = n_conn == 0 ? 0 : n_th ? n_th : 1;
    if (n_conn > a.cap_conn || n_ord > a.cap_ord) {
        if (tid == 0) a.info[q] = uc_record(ORB_ERANGE, n_conn, n_ord, 0);
        return;
    }
    if (n_conn == 0) {  // the early return of line 365
        if (tid == 0) a.info[q] = uc_record(ORB_OK, 0, 0, 1);
        return;
    }

    // KFcounter in ascending index, and the keys (weight << 16 | index) of vPairs
    uint32_t* keys = a.keys + (size_t)ql * a.pmax;
    int p2 = 1;
    while (p2 < n_ord) p2 <<= 1;
    int c_at = 0, o_at = 0;
    for (int k0 = 0; k0 < T.n_kf; k0 += LM_THREADS) {
        const int k = k0 + tid;
        const uint32_t v = k < T.n_kf ? votes_of(cnt, k) : 0;
        int total;
        const int cp = c_at + block_excl_scan<LM_WAVES>(v > 0 ? 1 : 0, s_wave, &total);
        c_at += total;
        if (v > 0) {
            a.conn_kf[(size_t)q * a.cap_conn + cp] = k;
            a.conn_w[(size_t)q * a.cap_conn + cp] = (int32_t)v;
        }
        if (n_th) {
            const bool in = v >= (uint32_t)UC_THRESHOLD;
            const int op = o_at + block_excl_scan<LM_WAVES>(in ? 1 : 0, s_wave, &total);
            o_at += total;
            if (in) keys[op] = (v << 16) | (uint32_t)k;
        }
    }
    if (!n_th && tid == 0) {  // the fallback of lines 390-394: the first strict maximum
        const uint32_t b = (uint32_t)s_misc[2];
        keys[0] = (b & 0xffff0000u) | (uint32_t)(65535 - (int)(b & 0xffffu));
    }
    for (int i = n_ord + tid; i < p2; i += LM_THREADS) keys[i] = 0;  // below every key: a weight is >= 1
    __syncthreads();

    // sort() then push_front (396-403): weight descending, index descending among equal weights, which
    // is the keys descending.  They are distinct, so any exact sort gives this order: bitonic, in place.
    for (int size = 2; size <= p2; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < (p2 >> 1); t += LM_THREADS) {
                const int i = ((t & ~(stride - 1)) << 1) | (t & (stride - 1));
                const int j = i | stride;
                const bool desc = (i & size) == 0;
                const uint32_t x = keys[i], y = keys[j];
                if ((x < y) == desc) keys[i] = y, keys[j] = x;
            }
            __syncthreads();
        }
    }
    for (int i = tid; i < n_ord; i += LM_THREADS) {
        const uint32_t key = keys[i];
        a.ord_kf[(size_t)q * a.cap_ord + i] = (int32_t)(key & 0xffffu);
        a.ord_w[(size_t)q * a.cap_ord + i] = (int32_t)(key >> 16);
    }
    if (tid == 0) a.info[q] = uc_record(ORB_OK, n_conn, n_ord, 0);
}

std::atomic<size_t> g_scratch_cap{0};  // 0: ORB_LM_MAX_SCRATCH_BYTES (orb_debug_set_local_map_scratch_cap)
size_t scratch_cap() {
    const size_t c = g_scratch_cap.load();
    return c ? c : (size_t)ORB_LM_MAX_SCRATCH_BYTES;
}

int check_tables(const std::string& who, const orb_local_map_tables_t* m, LmTables* T) {
    if (!m || m->n_kf < 0 || m->n_pt < 0 || m->n_kf_mp < 0 || m->n_obs < 0) return fail(ORB_EINVAL, who + ": bad arguments");
    if (m->n_kf > ORB_LM_MAX_KF) return fail(ORB_ENOTSUP, who + ": more than " + std::to_string(ORB_LM_MAX_KF) + " keyframes");
    if (!m->kf_mp_off || !m->pt_obs_off || (m->n_kf && (!m->kf_bad || !m->kf_cov)) || (m->n_pt && !m->pt_bad) ||
        (m->n_kf_mp && !m->kf_mp) || (m->n_obs && !m->pt_obs_kf))
        return fail(ORB_EINVAL, who + ": a table is NULL");
    T->n_kf = m->n_kf, T->n_pt = m->n_pt, T->n_kf_mp = m->n_kf_mp, T->n_obs = m->n_obs;
    T->kf_bad = m->kf_bad, T->kf_mp_off = m->kf_mp_off, T->kf_mp = m->kf_mp, T->kf_cov = m->kf_cov;
    T->pt_bad = m->pt_bad, T->pt_obs_off = m->pt_obs_off, T->pt_obs_kf = m->pt_obs_kf;
    return ORB_OK;
}

int launch_validate(const LmTables& T, hipStream_t st) {
    ORB_HIPCHK(hipMemsetAsync(T.tstatus, 0, sizeof(int), st));
    const long long items = std::max<long long>({(long long)T.n_kf * 10, T.n_kf_mp, T.n_pt, 1});
    const int blocks = (int)std::min<long long>((items + 255) / 256, 4096);
    hipLaunchKernelGGL(k_lm_validate, dim3(blocks), dim3(256), 0, st, T, (int)items);
    ORB_HIPCHK(hipGetLastError());
    return ORB_OK;
}

int set_lds_limits() {
    static const hipError_t e = [] {
        hipError_t r = hipFuncSetAttribute((const void*)k_lm_vote, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lm_vote_lds(ORB_LM_MAX_KF));
        if (r == hipSuccess) r = hipFuncSetAttribute((const void*)k_uc, hipFuncAttributeMaxDynamicSharedMemorySize, (int)uc_lds(ORB_LM_MAX_KF));
        return r;
    }();
    if (e != hipSuccess) return fail(ORB_EDEVICE, std::string("local map: LDS limit: ") + hipGetErrorString(e));
    return ORB_OK;
}

// the scratch of one frame of call 1; frames_per_chunk() of them stay under the cap
size_t lm_frame_bytes(const LmArgs& a) {
    const size_t nk = (size_t)a.T.n_kf;
    return orb_align256((size_t)a.T.n_pt * 4) + (3 + (a.kf_votes ? 1 : 0)) * orb_align256(nk * 4) + orb_align256(sizeof(orb_local_map_info_t));
}

// B frames of call 1 on `st`; a.T.tstatus and the chunk fields are set here
int launch_local_map(LmArgs a, int B, const std::string& who, hipStream_t st) {
    if (int r = set_lds_limits()) return r;
    const size_t per = lm_frame_bytes(a) + 256;
    if (per > scratch_cap()) return fail(ORB_ENOTSUP, who + ": one frame's scratch is above the cap of " + std::to_string(scratch_cap()) + " bytes");
    const int chunk = (int)std::min<size_t>((size_t)B, scratch_cap() / per);
    const size_t nk = (size_t)a.T.n_kf, np = (size_t)a.T.n_pt;
    void* block = nullptr;
    if (int r = orb_scratch_alloc(&block, st, who + ": scratch: ", [&](OrbLayout& Y) {
            a.T.tstatus = Y.take<int>(1);
            a.mark = Y.take<uint32_t>(np * chunk);
            a.list = Y.take<int32_t>(nk * chunk), a.rowpre = Y.take<int32_t>(nk * chunk), a.wcnt = Y.take<int32_t>(nk * chunk);
            a.votes = a.kf_votes ? Y.take<int32_t>(nk * chunk) : nullptr;
            a.rec = Y.take<orb_local_map_info_t>(chunk);
        }))
        return r;
    int r = launch_validate(a.T, st);
    const size_t lds = lm_vote_lds(a.T.n_kf);
    for (int f0 = 0; f0 < B && r == ORB_OK; f0 += chunk) {
        a.f0 = f0, a.nf = std::min(chunk, B - f0);
        const dim3 rows(LM_POS_BLOCKS, a.nf);
        hipError_t e = np ? hipMemsetAsync(a.mark, 0xFF, np * a.nf * 4, st) : hipSuccess;
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_lm_vote, dim3(a.nf), dim3(LM_THREADS), lds, st, a);
            hipLaunchKernelGGL(k_lm_mark, rows, dim3(LM_ROW_THREADS), 0, st, a);
            hipLaunchKernelGGL(k_lm_count, rows, dim3(LM_ROW_THREADS), 0, st, a);
            hipLaunchKernelGGL(k_lm_scan, dim3(a.nf), dim3(LM_THREADS), 0, st, a);
            hipLaunchKernelGGL(k_lm_write, rows, dim3(LM_ROW_THREADS), 0, st, a);
            hipLaunchKernelGGL(k_lm_finish, dim3(a.nf), dim3(LM_THREADS), 0, st, a);
            e = hipGetLastError();
        }
        if (e != hipSuccess) r = fail(ORB_EDEVICE, who + ": " + hipGetErrorString(e));
    }
    (void)hipFreeAsync(block, st);
    return r;
}

int launch_update_connections(UcArgs a, int K, const std::string& who, hipStream_t st) {
    if (int r = set_lds_limits()) return r;
    int pmax = 1;
    while (pmax < a.T.n_kf) pmax <<= 1;
    a.pmax = pmax;
    const size_t per = orb_align256((size_t)pmax * 4) + 256;
    if (per > scratch_cap()) return fail(ORB_ENOTSUP, who + ": one keyframe's scratch is above the cap of " + std::to_string(scratch_cap()) + " bytes");
    const int chunk = (int)std::min<size_t>((size_t)K, scratch_cap() / per);
    void* block = nullptr;
    if (int r = orb_scratch_alloc(&block, st, who + ": scratch: ", [&](OrbLayout& Y) {
            a.T.tstatus = Y.take<int>(1);
            a.keys = Y.take<uint32_t>((size_t)pmax * chunk);
        }))
        return r;
    int r = launch_validate(a.T, st);
    for (int k0 = 0; k0 < K && r == ORB_OK; k0 += chunk) {
        a.k0 = k0, a.nk = std::min(chunk, K - k0);
        hipLaunchKernelGGL(k_uc, dim3(a.nk), dim3(LM_THREADS), uc_lds(a.T.n_kf), st, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) r = fail(ORB_EDEVICE, who + ": " + hipGetErrorString(e));
    }
    (void)hipFreeAsync(block, st);
    return r;
}

// The offset tables of a host call, checked before anything is sized from them.
int check_host_offsets(const std::string& who, const orb_local_map_tables_t* m) {
    for (int i = 0; i < m->n_kf; ++i)
        if (m->kf_mp_off[i] < 0 || m->kf_mp_off[i + 1] < m->kf_mp_off[i])
            return fail(ORB_EINVAL, who + ": kf_mp_off is not monotone at " + std::to_string(i));
    for (int i = 0; i < m->n_pt; ++i)
        if (m->pt_obs_off[i] < 0 || m->pt_obs_off[i + 1] < m->pt_obs_off[i])
            return fail(ORB_EINVAL, who + ": pt_obs_off is not monotone at " + std::to_string(i));
    if (m->kf_mp_off[m->n_kf] > m->n_kf_mp || m->pt_obs_off[m->n_pt] > m->n_obs || m->kf_mp_off[m->n_kf] < 0 || m->pt_obs_off[m->n_pt] < 0)
        return fail(ORB_EINVAL, who + ": an offset table leaves its array");
    return ORB_OK;
}

// The tables of a host call as regions of its arena
struct TableRegions {
    OrbRegion<uint8_t> kf_bad, pt_bad;
    OrbRegion<int32_t> kf_mp_off, kf_mp, kf_cov, pt_obs_off, pt_obs_kf;
    void plan(OrbStagePlan& P, const orb_local_map_tables_t* m) {
        const size_t nk = (size_t)m->n_kf, np = (size_t)m->n_pt;
        kf_bad = P.in<uint8_t>(nk), pt_bad = P.in<uint8_t>(np);
        kf_mp_off = P.in<int32_t>(nk + 1), kf_mp = P.in<int32_t>((size_t)m->n_kf_mp), kf_cov = P.in<int32_t>(nk * 10);
        pt_obs_off = P.in<int32_t>(np + 1), pt_obs_kf = P.in<int32_t>((size_t)m->n_obs);
    }
    void send(const OrbHostCall& c, const orb_local_map_tables_t* m, LmTables* T) const {
        T->kf_bad = c.send(kf_bad, m->kf_bad), T->pt_bad = c.send(pt_bad, m->pt_bad);
        T->kf_mp_off = c.send(kf_mp_off, m->kf_mp_off), T->kf_mp = c.send(kf_mp, m->kf_mp), T->kf_cov = c.send(kf_cov, m->kf_cov);
        T->pt_obs_off = c.send(pt_obs_off, m->pt_obs_off), T->pt_obs_kf = c.send(pt_obs_kf, m->pt_obs_kf);
    }
};

const char* why(int status) {
    return status == ORB_EINVAL ? "an index is out of range, an offset table is not monotone or leaves its array, or a point's "
                                  "observations are not strictly ascending"
           : status == ORB_ENOTSUP ? "a keyframe's row holds more than 8192 entries"
           : status == ORB_ERANGE  ? "an output capacity is too small (the record holds the counts needed)"
                                   : "refused on the device";
}

}  // namespace

extern "C" {

int orb_debug_set_local_map_scratch_cap(size_t bytes) {
    g_scratch_cap.store(bytes);
    return ORB_OK;
}

int orb_local_map_reference(const orb_local_map_tables_t* map, int n, const int32_t* f_mp, int cap_kf, int cap_pt,
                            int32_t* f_mp_out, int32_t* local_kf, int32_t* local_pt, uint8_t* local_pt_seen,
                            int32_t* kf_votes, orb_local_map_info_t* info, int device) {
    const std::string who = "local_map_reference";
    LmArgs a{};
    if (int r = check_tables(who, map, &a.T)) return r;
    if (n < 0 || cap_kf < 0 || cap_pt < 0 || (n && (!f_mp || !f_mp_out)) || (cap_kf && !local_kf) ||
        (cap_pt && (!local_pt || !local_pt_seen)) || !info)
        return fail(ORB_EINVAL, who + ": bad arguments");
    if (n > ORB_LM_MAX_ROW) return fail(ORB_ENOTSUP, who + ": more than " + std::to_string(ORB_LM_MAX_ROW) + " frame entries");
    if (int r = check_host_offsets(who, map)) return r;
    const size_t nk = (size_t)map->n_kf;
    OrbStagePlan P;
    TableRegions R;
    R.plan(P, map);
    const auto rMp = P.in<int32_t>((size_t)n), rCnt = P.in<int32_t>(1);
    const auto rInfo = P.out<orb_local_map_info_t>(1);
    const auto rOut = P.out<int32_t>((size_t)n), rKf = P.out<int32_t>((size_t)cap_kf), rPt = P.out<int32_t>((size_t)cap_pt);
    const auto rSeen = P.out<uint8_t>((size_t)cap_pt);
    const auto rVotes = P.out<int32_t>(kf_votes ? nk : 0);
    OrbHostCall call(P, device);
    if (call.err) return call.err;
    R.send(call, map, &a.T);
    a.cap = n, a.cap_kf = cap_kf, a.cap_pt = cap_pt;
    a.f_mp = call.send(rMp, f_mp), a.counts = call.send(rCnt, &n);
    a.info = call.dev(rInfo), a.f_mp_out = call.dev(rOut), a.local_kf = call.dev(rKf), a.local_pt = call.dev(rPt);
    a.local_pt_seen = call.dev(rSeen), a.kf_votes = kf_votes ? call.dev(rVotes) : nullptr;
    if (int r = call.upload()) return r;
    if (int r = call.finish(launch_local_map(a, 1, who, call.stream()), hipSuccess, who + ": ")) return r;
    const orb_local_map_info_t* I = call.host(rInfo);
    call.get(rInfo, info);
    if (I->status != ORB_OK) return fail(I->status, who + ": " + why(I->status));
    call.get(rOut, f_mp_out);
    call.get(rKf, local_kf, (size_t)I->n_local_kf), call.get(rPt, local_pt, (size_t)I->n_local_pt);
    call.get(rSeen, local_pt_seen, (size_t)I->n_local_pt);
    call.get(rVotes, kf_votes);
    return ORB_OK;
}

int orb_local_map_reference_batch_device(const orb_local_map_tables_t* d_map, int B, int cap, const int32_t* d_f_mp,
                                         const int32_t* d_counts, int cap_kf, int cap_pt, int32_t* d_f_mp_out,
                                         int32_t* d_local_kf, int32_t* d_local_pt, uint8_t* d_local_pt_seen,
                                         int32_t* d_kf_votes, orb_local_map_info_t* d_info, void* stream) {
    const std::string who = "local_map_reference_batch";
    LmArgs a{};
    if (int r = check_tables(who, d_map, &a.T)) return r;
    if (B < 0 || cap < 0 || cap_kf < 0 || cap_pt < 0) return fail(ORB_EINVAL, who + ": bad arguments");
    if (B > 65535) return fail(ORB_ENOTSUP, who + ": more than 65535 frames per call");
    if (cap > ORB_LM_MAX_ROW) return fail(ORB_ENOTSUP, who + ": more than " + std::to_string(ORB_LM_MAX_ROW) + " frame entries");
    if (B == 0) return ORB_OK;
    if (!d_counts || !d_info || (cap && (!d_f_mp || !d_f_mp_out)) || (cap_kf && !d_local_kf) ||
        (cap_pt && (!d_local_pt || !d_local_pt_seen)))
        return fail(ORB_EINVAL, who + ": bad arguments");
    a.cap = cap, a.cap_kf = cap_kf, a.cap_pt = cap_pt, a.f_mp = d_f_mp, a.counts = d_counts;
    a.f_mp_out = d_f_mp_out, a.local_kf = d_local_kf, a.local_pt = d_local_pt, a.local_pt_seen = d_local_pt_seen;
    a.kf_votes = d_kf_votes, a.info = d_info;
    return launch_local_map(a, B, who, (hipStream_t)stream);
}

int orb_keyframe_update_connections(const orb_local_map_tables_t* map, int K, const int32_t* kf_idx, int cap_conn,
                                    int cap_ord, int32_t* conn_kf, int32_t* conn_w, int32_t* ord_kf, int32_t* ord_w,
                                    orb_update_connections_info_t* info, int device) {
    const std::string who = "keyframe_update_connections";
    UcArgs a{};
    if (int r = check_tables(who, map, &a.T)) return r;
    if (K < 0 || cap_conn < 0 || cap_ord < 0 || (K && (!kf_idx || !info)) || (K && cap_conn && (!conn_kf || !conn_w)) ||
        (K && cap_ord && (!ord_kf || !ord_w)))
        return fail(ORB_EINVAL, who + ": bad arguments");
    if (K > 65535) return fail(ORB_ENOTSUP, who + ": more than 65535 keyframes per call");
    if (K == 0) return ORB_OK;
    if (int r = check_host_offsets(who, map)) return r;
    const size_t NK = (size_t)K;
    OrbStagePlan P;
    TableRegions R;
    R.plan(P, map);
    const auto rIdx = P.in<int32_t>(NK);
    const auto rInfo = P.out<orb_update_connections_info_t>(NK);
    const auto rCk = P.out<int32_t>(NK * cap_conn), rCw = P.out<int32_t>(NK * cap_conn);
    const auto rOk = P.out<int32_t>(NK * cap_ord), rOw = P.out<int32_t>(NK * cap_ord);
    OrbHostCall call(P, device);
    if (call.err) return call.err;
    R.send(call, map, &a.T);
    a.cap_conn = cap_conn, a.cap_ord = cap_ord, a.kf_idx = call.send(rIdx, kf_idx);
    a.info = call.dev(rInfo), a.conn_kf = call.dev(rCk), a.conn_w = call.dev(rCw), a.ord_kf = call.dev(rOk), a.ord_w = call.dev(rOw);
    if (int r = call.upload()) return r;
    if (int r = call.finish(launch_update_connections(a, K, who, call.stream()), hipSuccess, who + ": ")) return r;
    const orb_update_connections_info_t* I = call.host(rInfo);
    call.get(rInfo, info);
    int first_bad = ORB_OK;
    for (int q = 0; q < K; ++q) {
        if (I[q].status != ORB_OK) {
            if (first_bad == ORB_OK) first_bad = I[q].status;
            continue;
        }
        const size_t c0 = (size_t)q * cap_conn, o0 = (size_t)q * cap_ord;
        call.get(rCk, conn_kf ? conn_kf + c0 : nullptr, (size_t)I[q].n_conn, c0);
        call.get(rCw, conn_w ? conn_w + c0 : nullptr, (size_t)I[q].n_conn, c0);
        call.get(rOk, ord_kf ? ord_kf + o0 : nullptr, (size_t)I[q].n_ord, o0);
        call.get(rOw, ord_w ? ord_w + o0 : nullptr, (size_t)I[q].n_ord, o0);
    }
    if (first_bad != ORB_OK) return fail(first_bad, who + ": " + why(first_bad));
    return ORB_OK;
}

int orb_keyframe_update_connections_batch_device(const orb_local_map_tables_t* d_map, int K, const int32_t* d_kf_idx,
                                                 int cap_conn, int cap_ord, int32_t* d_conn_kf, int32_t* d_conn_w,
                                                 int32_t* d_ord_kf, int32_t* d_ord_w,
                                                 orb_update_connections_info_t* d_info, void* stream) {
    const std::string who = "keyframe_update_connections_batch";
    UcArgs a{};
    if (int r = check_tables(who, d_map, &a.T)) return r;
    if (K < 0 || cap_conn < 0 || cap_ord < 0) return fail(ORB_EINVAL, who + ": bad arguments");
    if (K > 65535) return fail(ORB_ENOTSUP, who + ": more than 65535 keyframes per call");
    if (K == 0) return ORB_OK;
    if (!d_kf_idx || !d_info || (cap_conn && (!d_conn_kf || !d_conn_w)) || (cap_ord && (!d_ord_kf || !d_ord_w)))
        return fail(ORB_EINVAL, who + ": bad arguments");
    a.cap_conn = cap_conn, a.cap_ord = cap_ord, a.kf_idx = d_kf_idx;
    a.conn_kf = d_conn_kf, a.conn_w = d_conn_w, a.ord_kf = d_ord_kf, a.ord_w = d_ord_w, a.info = d_info;
    return launch_update_connections(a, K, who, (hipStream_t)stream);
}

}  // extern "C"
