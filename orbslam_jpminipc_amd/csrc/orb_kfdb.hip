// orb_kfdb.hip — KeyFrameDatabase and the L1 BoW score on the GPU (part of liborb_hip.so).
//
// Replaces, for the reference's place recognition:
//   L1Scoring::score (through TemplatedVocabulary::score)   Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68
//   KeyFrameDatabase::add / erase / clear                   src/KeyFrameDatabase.cc:39-72
//   KeyFrameDatabase::DetectLoopCandidates                                          75-196
//   KeyFrameDatabase::DetectRelocalisationCandidates                                198-308
//
// The reference keeps an inverted file (a std::list<KeyFrame*> per word) and walks the query's
// words over it.  Here the keyframes' BowVectors lie back to back in one entry pool and a query
// is a keyframe-major scan of that pool:
//
//   k_kfdb_scan    a wave per keyframe, the query's words and values staged in LDS once per
//                  workgroup (up to 2048 words = 24 KB, so occupancy holds; a longer query is
//                  searched in HBM).  Each lane takes one entry of the keyframe and binary-searches its
//                  word in the query (four 64-entry groups in flight); the wave ballots the hits.
//                  common += popcount, first = the first hit's word, and the L1 terms
//                  fabs(vi - wi) - fabs(vi) - fabs(wi) of the hit lanes are added one at a time in
//                  lane order (= ascending word order), so the
//                  double is the reference's sequential sum bit for bit and the chain's length is
//                  `common`, not the vector length.  All Q queries of a batch scan together
//                  (blockIdx.y).
//   k_kfdb_prepare a workgroup per query: maxCommon, minCommon and si = (float)score of the
//                  keyframes with common > minCommon.
//   k_kfdb_chain   a thread per slot, through the queries of a relocalisation batch in order:
//                  the stored reloc score as each query finds it (its own score, or the one the
//                  latest earlier query left, or the one from the calls before), and the stored
//                  score after the batch.  Only this chain orders the queries of a batch.
//   k_kfdb_select  a workgroup per query: the covisibility accumulation, bestAcc, the 0.75
//                  threshold, and the kept entries sorted by (first shared word, add sequence) =
//                  the order of the reference's lKFsSharingWords, de-duplicated in that order.
//   k_kfdb_query1  the three in one workgroup for a single query (the host entry points).
//   k_kfdb_pairs   score of P pairs of batched-transform BowVectors, a wave per pair.
//   k_kfdb_add, k_kfdb_compact, k_kfdb_set_cov   pool maintenance (plain copies).
//
// Only L1_NORM vocabularies (ORBvoc is one) are supported: every entry point here returns
// ORB_EINVAL for another scoring type.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/orb_abi.h"
#include "../../include/orb_debug.h"
#include "orb_internal.h"

namespace {

#define KFDB_MAX_WORDS 8192        // words of one BowVector (the transform's limit)
#define KFDB_MAX_KEYFRAMES 65536
#define KFDB_MAX_COV 10            // GetBestCovisibilityKeyFrames(10)
#define KFDB_SEL_THREADS 1024
#define KFDB_LDS_WORDS 2048        // queries up to this length are staged in LDS (24 KB), longer ones stay in HBM
#define KFDB_ILP 4                 // 64-entry groups of a keyframe in flight per wave
#define KFDB_ADD_CHUNK 128         // keyframes per k_kfdb_add launch (their metadata travels by value)

int fail(int code, const std::string& msg) { return orb_internal_set_error(code, msg); }

// score += term of every lane in `mask`, lowest lane first (mask is wave-uniform).
__device__ inline double ordered_add(double score, double term, unsigned long long mask) {
    while (mask) {
        const int l = __ffsll((long long)mask) - 1;
        score += __shfl(term, l);
        mask &= mask - 1;
    }
    return score;
}

// base[k] -> the last position of the ascending a[0 .. n) that can still hold w[k], for G keys at
// once: a branch-free lower bound with one trip count for every lane and key, so the G reads of a
// step are independent.  a[base[k]] < w[k] then tells whether the bound is base[k] or base[k] + 1.
template <int G, typename P>
__device__ inline void lower_bounds(P a, int n, const uint32_t (&w)[KFDB_ILP], int (&base)[KFDB_ILP]) {
    for (int len = n; len > 1;) {  // the lower bound stays in [base, base + len]
        const int half = len >> 1;
#pragma unroll
        for (int k = 0; k < G; ++k) base[k] += a[base[k] + half - 1] < w[k] ? half : 0;
        len -= half;
    }
}

static_assert(KFDB_ILP == 4, "wave_intersect's switch lists the group counts 1 .. 4");

// One wave: the entries (kw, kv)[0 .. L) of a keyframe against the query (qw, qv)[0 .. n).
// The L1 term takes vi from the query and wi from the keyframe, as score(query, keyframe).
// KFDB_ILP x 64 entries per step, loaded one step ahead: their binary searches (a branch-free lower
// bound with one trip count for every lane and entry) are independent and overlap; the ballots
// and the ordered adds then follow in entry order.
template <typename PW, typename PV>
__device__ inline void wave_intersect(const uint32_t* kw, const double* kv, int L, PW qw, PV qv, int n, int lane,
                                      int& common, uint32_t& first, double& sum) {
    common = 0;
    first = 0xFFFFFFFFu;
    sum = 0.0;
    if (n <= 0) return;
    uint32_t w[KFDB_ILP], wn[KFDB_ILP];
    double wi[KFDB_ILP], win[KFDB_ILP];
#pragma unroll
    for (int k = 0; k < KFDB_ILP; ++k) {
        const int i = 64 * k + lane;
        wn[k] = i < L ? kw[i] : 0u;
        win[k] = i < L ? kv[i] : 0.0;
    }
    for (int i0 = 0; i0 < L; i0 += 64 * KFDB_ILP) {
        int base[KFDB_ILP];
#pragma unroll
        for (int k = 0; k < KFDB_ILP; ++k) {  // this step's entries, and the next step's loads in flight
            w[k] = wn[k];
            wi[k] = win[k];
            base[k] = 0;
            const int i = i0 + 64 * (KFDB_ILP + k) + lane;
            wn[k] = i < L ? kw[i] : 0u;
            win[k] = i < L ? kv[i] : 0.0;
        }
        const int groups = min(KFDB_ILP, (L - i0 + 63) >> 6);  // wave-uniform: groups that hold entries
        switch (groups) {  // only the groups that hold entries are searched (short keyframes)
            case 1: lower_bounds<1>(qw, n, w, base); break;
            case 2: lower_bounds<2>(qw, n, w, base); break;
            case 3: lower_bounds<3>(qw, n, w, base); break;
            default: lower_bounds<KFDB_ILP>(qw, n, w, base); break;
        }
#pragma unroll
        for (int k = 0; k < KFDB_ILP; ++k) {
            if (k >= groups) break;
            const int j = base[k] + (qw[base[k]] < w[k] ? 1 : 0);
            const bool hit = i0 + 64 * k + lane < L && j < n && qw[j] == w[k];
            double term = 0.0;
            if (hit) {
                const double vi = qv[j];
                term = fabs(vi - wi[k]) - fabs(vi) - fabs(wi[k]);
            }
            const unsigned long long mask = __ballot(hit);
            if (mask) {
                if (common == 0) first = (uint32_t)__shfl((int)w[k], __ffsll((long long)mask) - 1);
                common += __popcll(mask);
                sum = ordered_add(sum, term, mask);
            }
        }
    }
}

__global__ void __launch_bounds__(256) k_kfdb_scan(const uint32_t* __restrict__ poolW, const double* __restrict__ poolV,
                                                   const int* __restrict__ off, const int* __restrict__ len, int hi,
                                                   const uint32_t* __restrict__ qW, const double* __restrict__ qV,
                                                   const int* __restrict__ qN, int qcap, int ldsCap,
                                                   int* __restrict__ common, uint32_t* __restrict__ first,
                                                   double* __restrict__ score, int stride) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    double* s_v = (double*)smem;
    uint32_t* s_w = (uint32_t*)(s_v + ldsCap);
    const int q = blockIdx.y;
    const int n = max(0, min(qN[q], qcap));
    const uint32_t* gw = qW + (size_t)q * qcap;
    const double* gv = qV + (size_t)q * qcap;
    const bool staged = n <= ldsCap;  // block-uniform; a longer query (rare) is searched where it lies
    if (staged)
        for (int i = threadIdx.x; i < n; i += 256) {
            s_w[i] = gw[i];
            s_v[i] = gv[i];
        }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int slot = blockIdx.x * 4 + wave; slot < hi; slot += gridDim.x * 4) {
        const int L = len[slot];
        int c = 0;
        uint32_t f = 0xFFFFFFFFu;
        double s = 0.0;
        if (L > 0) {
            const size_t base = (size_t)off[slot];
            if (staged) wave_intersect(poolW + base, poolV + base, L, s_w, s_v, n, lane, c, f, s);
            else wave_intersect(poolW + base, poolV + base, L, gw, gv, n, lane, c, f, s);
        }
        if (lane == 0) {
            const size_t o = (size_t)q * stride + slot;
            common[o] = c;
            first[o] = f;
            score[o] = -s / 2.0;
        }
    }
}

// Pair p: score(frame a, frame b) of batched-transform BowVectors; a wave per pair.
__global__ void __launch_bounds__(256) k_kfdb_pairs(int P, const uint32_t* __restrict__ bowW,
                                                    const double* __restrict__ bowV, const int* __restrict__ bowN,
                                                    int cap, const int* __restrict__ pa, const int* __restrict__ pb,
                                                    double* __restrict__ out) {
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (p >= P) return;
    const int a = pa[p], b = pb[p];
    const int na = max(0, min(bowN[a], cap)), nb = max(0, min(bowN[b], cap));
    int c;
    uint32_t f;
    double s;
    // the walk is over b's entries, looked up in a: the shared words come in the same ascending order
    wave_intersect(bowW + (size_t)b * cap, bowV + (size_t)b * cap, nb, bowW + (size_t)a * cap, bowV + (size_t)a * cap,
                   na, lane, c, f, s);
    if (lane == 0) out[p] = -s / 2.0;
}

struct AddChunk {
    int n;                       // keyframes in this launch
    int slot[KFDB_ADD_CHUNK];
    int off[KFDB_ADD_CHUNK];     // position in the pool
    int len[KFDB_ADD_CHUNK];     // entries, or -1 = erase the slot
    int src[KFDB_ADD_CHUNK];     // frame of the source batch (copy skipped when srcW == NULL)
    uint32_t seq[KFDB_ADD_CHUNK];
};

__global__ void __launch_bounds__(256) k_kfdb_add(AddChunk c, const uint32_t* __restrict__ srcW,
                                                  const double* __restrict__ srcV, int cap,
                                                  uint32_t* __restrict__ poolW, double* __restrict__ poolV,
                                                  int* __restrict__ off, int* __restrict__ len,
                                                  uint32_t* __restrict__ seq, float* __restrict__ reloc) {
    const int k = blockIdx.y;
    if (k >= c.n) return;
    const int L = c.len[k];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        off[c.slot[k]] = c.off[k];
        len[c.slot[k]] = L;
        seq[c.slot[k]] = c.seq[k];
        reloc[c.slot[k]] = 0.0f;
    }
    if (!srcW) return;
    const size_t s = (size_t)c.src[k] * cap, d = (size_t)c.off[k];
    for (int i = blockIdx.x * 256 + threadIdx.x; i < L; i += gridDim.x * 256) {
        poolW[d + i] = srcW[s + i];
        poolV[d + i] = srcV[s + i];
    }
}

// Live keyframes to their new places in the other pool buffer.
__global__ void __launch_bounds__(256) k_kfdb_compact(int hi, const int* __restrict__ len, const int* __restrict__ off,
                                                      const int* __restrict__ newOff,
                                                      const uint32_t* __restrict__ srcW, const double* __restrict__ srcV,
                                                      uint32_t* __restrict__ dstW, double* __restrict__ dstV) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int slot = blockIdx.x * 4 + wave; slot < hi; slot += gridDim.x * 4) {
        const int L = len[slot];
        if (L <= 0) continue;
        const size_t s = (size_t)off[slot], d = (size_t)newOff[slot];
        for (int i = lane; i < L; i += 64) {
            dstW[d + i] = srcW[s + i];
            dstV[d + i] = srcV[s + i];
        }
    }
}

struct CovArgs {
    int slot, n;
    int ids[KFDB_MAX_COV];
};
__global__ void k_kfdb_set_cov(CovArgs a, int* cov, uint8_t* covN) {
    if (threadIdx.x < KFDB_MAX_COV) cov[a.slot * KFDB_MAX_COV + threadIdx.x] = threadIdx.x < a.n ? a.ids[threadIdx.x] : -1;
    if (threadIdx.x == 0) covN[a.slot] = (uint8_t)a.n;
}

struct SelArgs {
    int hi, stride, pstride, Q, loop;  // loop = 1: DetectLoopCandidates (Q = 1), 0: relocalisation
    float minScore;              // loop only
    const int* len;              // per slot: entries, < 0 = not live
    const uint32_t* seq;
    const int* cov;
    const uint8_t* covN;
    float* reloc;                // persistent mRelocScore: read and written by the chain
    const uint8_t* connected;    // loop only
    const int* common;           // [Q x stride] from the scan
    const uint32_t* first;
    const double* score;
    uint8_t* scored;             // [Q x stride] prepare: common > minCommon (and in the sharing list)
    float* si;                   // [Q x stride] prepare: (float)score where scored; chain: the rest
    // scratch of select, [Q x stride]
    float* acc;
    int* bestKF;
    uint8_t* entry;
    int* firstPos;
    // scratch of select per kept entry, [Q x pstride] (pstride = stride padded to a power of two)
    unsigned long long* key;
    int* pay;
    // results
    int* outIds;                 // [Q x outCap]
    int outCap;
    int* nOut;                   // [Q]
};

// Query q: maxCommonWords, minCommonWords and the float scores of the keyframes above it.
__device__ inline void prepare_query(const SelArgs& A, int q, int* s_max) {
    const int tid = threadIdx.x, T = KFDB_SEL_THREADS;
    const int* cm = A.common + (size_t)q * A.stride;
    const double* sc = A.score + (size_t)q * A.stride;
    uint8_t* scored = A.scored + (size_t)q * A.stride;
    float* si = A.si + (size_t)q * A.stride;
    if (tid == 0) *s_max = 0;
    __syncthreads();
    // the sharing list's maxCommonWords (connected keyframes never enter the list)
    int m = 0;
    for (int s = tid; s < A.hi; s += T)
        if (A.len[s] >= 0 && !(A.loop && A.connected[s])) m = max(m, cm[s]);
    if (m > 0) atomicMax(s_max, m);
    __syncthreads();
    const int maxCommon = *s_max;
    const int minCommon = (int)((float)maxCommon * 0.8f);
    for (int s = tid; s < A.hi; s += T) {
        const bool in = A.len[s] >= 0 && cm[s] >= 1 && !(A.loop && A.connected[s]);
        const bool sco = in && cm[s] > minCommon;
        scored[s] = sco ? 1 : 0;
        if (sco) si[s] = (float)sc[s];
    }
}

// Slot s through the queries of a relocalisation batch in order: where query q did not score the
// slot, si[q][s] becomes the score the slot carries at that time (from the latest query before q
// that scored it, else from the calls before), so si[q][s] is mRelocScore as query q finds it.
// This chain is all that orders the queries of a batch.  The last value is the stored score.
__device__ inline void chain_slot(const SelArgs& A, int s) {
    float v = A.reloc[s];
    for (int q = 0; q < A.Q; ++q) {
        const size_t o = (size_t)q * A.stride + s;
        const float x = A.si[o];
        v = A.scored[o] ? x : v;
        A.si[o] = v;
    }
    A.reloc[s] = v;
}

// Query q: covisibility accumulation, bestAcc, the threshold, and the kept entries in the order
// of the reference's list, de-duplicated.
__device__ inline void select_query(const SelArgs& A, int q, int* s_cnt, float* s_red, int* s_scan) {
    const int tid = threadIdx.x, T = KFDB_SEL_THREADS;
    const int* cm = A.common + (size_t)q * A.stride;
    const uint32_t* fw = A.first + (size_t)q * A.stride;
    const uint8_t* scored = A.scored + (size_t)q * A.stride;
    const float* si = A.si + (size_t)q * A.stride;
    float* accA = A.acc + (size_t)q * A.stride;
    int* bestKF = A.bestKF + (size_t)q * A.stride;
    uint8_t* entry = A.entry + (size_t)q * A.stride;
    int* firstPos = A.firstPos + (size_t)q * A.stride;
    unsigned long long* key = A.key + (size_t)q * A.pstride;
    int* pay = A.pay + (size_t)q * A.pstride;
    if (tid == 0) *s_cnt = 0;
    // ---- accumulate over the covisible keyframes ----
    float localBest = A.loop ? A.minScore : 0.0f;
    for (int s = tid; s < A.hi; s += T) {
        firstPos[s] = INT_MAX;
        const bool e = scored[s] && (!A.loop || si[s] >= A.minScore);
        entry[s] = e ? 1 : 0;
        if (!e) continue;
        const int nc = A.covN[s];
        int nbv[KFDB_MAX_COV];
        float val[KFDB_MAX_COV];
        bool use[KFDB_MAX_COV];
#pragma unroll
        for (int j = 0; j < KFDB_MAX_COV; ++j) nbv[j] = j < nc ? A.cov[s * KFDB_MAX_COV + j] : -1;
#pragma unroll
        for (int j = 0; j < KFDB_MAX_COV; ++j) {  // the neighbours' loads do not wait for each other
            const bool ok = nbv[j] >= 0 && nbv[j] < A.hi;
            const int o = ok ? nbv[j] : s;
            // loop: in this query's list, not connected, common > minCommon -> this query's score;
            // relocalisation: mnRelocQuery == this query -> this query's score, or a stale one
            use[j] = ok && A.len[o] >= 0 && (A.loop ? scored[o] != 0 : cm[o] >= 1);
            val[j] = si[o];
        }
        float acc = si[s], best = acc;
        int bk = s;
#pragma unroll
        for (int j = 0; j < KFDB_MAX_COV; ++j)  // in the neighbours' order
            if (use[j]) {
                acc += val[j];
                if (val[j] > best) {
                    best = val[j];
                    bk = nbv[j];
                }
            }
        accA[s] = acc;
        bestKF[s] = bk;
        if (acc > localBest) localBest = acc;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const float t = __shfl_xor(localBest, o);
        if (t > localBest) localBest = t;
    }
    if ((tid & 63) == 0) s_red[tid >> 6] = localBest;
    __syncthreads();
    float bestAcc = s_red[0];
    for (int w = 1; w < T / 64; ++w)
        if (s_red[w] > bestAcc) bestAcc = s_red[w];
    const float minScoreToRetain = 0.75f * bestAcc;
    // ---- the kept entries, then their list order ----
    for (int s = tid; s < A.hi; s += T)
        if (entry[s] && accA[s] > minScoreToRetain) {
            const int i = atomicAdd(s_cnt, 1);
            key[i] = ((unsigned long long)fw[s] << 32) | A.seq[s];
            pay[i] = bestKF[s];
        }
    __syncthreads();
    const int K = *s_cnt;
    int P = 1;
    while (P < K) P <<= 1;
    for (int i = K + tid; i < P; i += T) key[i] = ~0ull;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += T) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const unsigned long long a = key[i], b = key[ixj];
                    if ((a > b) == ((i & k) == 0)) {
                        key[i] = b;
                        key[ixj] = a;
                        const int pa = pay[i];
                        pay[i] = pay[ixj];
                        pay[ixj] = pa;
                    }
                }
            }
            __syncthreads();
        }
    // ---- first occurrence of every bestKF, in list order ----
    for (int i = tid; i < K; i += T) atomicMin(&firstPos[pay[i]], i);
    __syncthreads();
    // threads 0 .. nAct-1 own C consecutive entries each; an inclusive scan of their counts
    const int C = (K + T - 1) / T, i0 = tid * C, i1 = min(K, i0 + C);
    const int nAct = C ? (K + C - 1) / C : 0;
    int cnt = 0;
    for (int i = i0; i < i1; ++i) cnt += firstPos[pay[i]] == i;
    s_scan[tid] = cnt;
    __syncthreads();
    for (int d = 1; d < nAct; d <<= 1) {
        const int v = (tid < nAct && tid >= d) ? s_scan[tid - d] : 0;
        __syncthreads();
        s_scan[tid] += v;
        __syncthreads();
    }
    int u = s_scan[tid] - cnt;
    for (int i = i0; i < i1; ++i)
        if (firstPos[pay[i]] == i) {
            if (u < A.outCap) A.outIds[(size_t)q * A.outCap + u] = pay[i];
            ++u;
        }
    if (tid == 0) A.nOut[q] = nAct ? s_scan[nAct - 1] : 0;
}

__global__ void __launch_bounds__(KFDB_SEL_THREADS) k_kfdb_prepare(SelArgs A) {
    __shared__ int s_max;
    prepare_query(A, blockIdx.x, &s_max);
}

__global__ void __launch_bounds__(256) k_kfdb_chain(SelArgs A) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s < A.hi) chain_slot(A, s);
}

__global__ void __launch_bounds__(KFDB_SEL_THREADS) k_kfdb_select(SelArgs A) {
    __shared__ int s_cnt;
    __shared__ float s_red[KFDB_SEL_THREADS / 64];
    __shared__ int s_scan[KFDB_SEL_THREADS];
    select_query(A, blockIdx.x, &s_cnt, s_red, s_scan);
}

// The three steps of one query (a host call) in one workgroup.
__global__ void __launch_bounds__(KFDB_SEL_THREADS) k_kfdb_query1(SelArgs A) {
    __shared__ int s_int;
    __shared__ float s_red[KFDB_SEL_THREADS / 64];
    __shared__ int s_scan[KFDB_SEL_THREADS];
    prepare_query(A, 0, &s_int);
    __syncthreads();
    if (!A.loop) {
        for (int s = threadIdx.x; s < A.hi; s += KFDB_SEL_THREADS) chain_slot(A, s);
        __syncthreads();
    }
    select_query(A, 0, &s_int, s_red, s_scan);
}

double l1_score_host(const uint32_t* w1, const double* v1, int n1, const uint32_t* w2, const double* v2, int n2) {
    double score = 0;
    int i = 0, j = 0;
    while (i < n1 && j < n2) {
        if (w1[i] == w2[j]) {
            const double vi = v1[i], wi = v2[j];
            score += fabs(vi - wi) - fabs(vi) - fabs(wi);
            ++i;
            ++j;
        } else if (w1[i] < w2[j]) {
            ++i;
        } else {
            ++j;
        }
    }
    return -score / 2.0;
}

int check_l1(const orb_vocabulary_t* v, int* n_words) {
    if (!v) return fail(ORB_EINVAL, "NULL vocabulary");
    int32_t info[7];
    int st = orb_vocabulary_info(v, info);
    if (st) return st;
    if (info[2] != 0)
        return fail(ORB_EINVAL, "only L1_NORM vocabularies are supported (scoring type " + std::to_string(info[2]) + ")");
    if (n_words) *n_words = info[5];
    return ORB_OK;
}

// Words strictly ascending and < n_words.
int check_bow(const uint32_t* words, const double* values, int n, int n_words, const char* what) {
    if (n < 0 || (n > 0 && (!words || !values))) return fail(ORB_EINVAL, std::string(what) + ": bad BowVector arrays");
    if (n > KFDB_MAX_WORDS) return fail(ORB_ENOTSUP, std::string(what) + ": more than 8192 words in a BowVector");
    for (int i = 0; i < n; ++i) {
        if (words[i] >= (uint32_t)n_words)
            return fail(ORB_EINVAL, std::string(what) + ": word id " + std::to_string(words[i]) +
                                        " is not below the vocabulary's " + std::to_string(n_words) + " words");
        if (i > 0 && words[i] <= words[i - 1])
            return fail(ORB_EINVAL, std::string(what) + ": words are not strictly ascending at entry " + std::to_string(i));
    }
    return ORB_OK;
}

}  // namespace

struct orb_keyframe_db {
    int nWords = 0, device = 0, maxKF = 0;
    long long maxEntries = 0;
    std::mutex mu;
    hipStream_t stream = nullptr;      // the host entry points' stream
    // The device entry points enqueue on the caller's stream and record `done` there; the next call
    // on the handle waits for that event (the caller's stream itself is never touched again, so it
    // may be destroyed in between).  Host entry points leave their own stream idle.
    hipEvent_t done = nullptr;
    bool pending = false;              // `done` is recorded and not yet waited for by the host
    // host mirror of the slots
    std::vector<int> off, len;
    std::vector<uint32_t> seq;
    uint32_t nextSeq = 0;
    int hi = 0, nLive = 0;             // slots < hi have been used since the last clear
    long long liveEntries = 0, tail = 0;
    // device state
    uint32_t* d_poolW[2] = {nullptr, nullptr};
    double* d_poolV[2] = {nullptr, nullptr};
    int cur = 0;
    int *d_off = nullptr, *d_len = nullptr, *d_newOff = nullptr, *d_cov = nullptr;
    uint32_t* d_seq = nullptr;
    float* d_reloc = nullptr;
    uint8_t* d_covN = nullptr;
    // query scratch
    int qCap = 0, lastQ = 0;
    int* d_common = nullptr;
    uint32_t* d_first = nullptr;
    double* d_score = nullptr;
    uint8_t* d_scored = nullptr;
    float *d_si = nullptr, *d_acc = nullptr;
    int *d_bestKF = nullptr, *d_firstPos = nullptr, *d_pay = nullptr;
    uint8_t *d_entry = nullptr, *d_conn = nullptr;
    unsigned long long* d_key = nullptr;
    int pstride = 1;                   // maxKF padded to a power of two (the sort of the kept entries)
    // host-query staging, one pinned buffer.  Query: 16-byte header (n), n values, n words, copied
    // to d_qbuf in one transfer; result: the count, then the candidates, written there by the kernel.
    uint8_t* d_qbuf = nullptr;
    uint8_t* h_stage = nullptr;
    size_t resOff = 0;                 // the result's place in h_stage

    void release() {
        (void)hipSetDevice(device);
        if (pending) (void)hipEventSynchronize(done);
        if (stream) (void)hipStreamSynchronize(stream);
        if (done) (void)hipEventDestroy(done);
        void* all[] = {d_poolW[0], d_poolW[1], d_poolV[0], d_poolV[1], d_off, d_len, d_newOff, d_cov, d_seq, d_reloc,
                       d_covN, d_common, d_first, d_score, d_scored, d_si, d_acc, d_bestKF, d_firstPos, d_pay, d_entry,
                       d_conn, d_key, d_qbuf};
        for (void* p : all) (void)hipFree(p);
        if (h_stage) (void)hipHostFree(h_stage);
        if (stream) (void)hipStreamDestroy(stream);
    }

    // The host waits for the last device entry point's work.
    int wait_pending() {
        if (pending) ORB_HIPCHK(hipEventSynchronize(done));
        pending = false;
        return ORB_OK;
    }
    // A host entry point (synchronous, on the handle's stream) begins.
    int enter_host() {
        ORB_HIPCHK(hipSetDevice(device));
        return wait_pending();
    }
    // A device entry point begins / has enqueued its work on the caller's stream `s`.
    int enter_device(hipStream_t s) {
        ORB_HIPCHK(hipSetDevice(device));
        if (pending) ORB_HIPCHK(hipStreamWaitEvent(s, done, 0));
        return ORB_OK;
    }
    int leave_device(hipStream_t s) {
        ORB_HIPCHK(hipEventRecord(done, s));
        pending = true;
        return ORB_OK;
    }

    int reset_device(hipStream_t s) {
        ORB_HIPCHK(hipMemsetAsync(d_len, 0xFF, (size_t)maxKF * 4, s));
        ORB_HIPCHK(hipMemsetAsync(d_covN, 0, (size_t)maxKF, s));
        ORB_HIPCHK(hipMemsetAsync(d_reloc, 0, (size_t)maxKF * 4, s));
        ORB_HIPCHK(hipMemsetAsync(d_seq, 0, (size_t)maxKF * 4, s));
        ORB_HIPCHK(hipMemsetAsync(d_off, 0, (size_t)maxKF * 4, s));
        return ORB_OK;
    }

    int alloc() {
        ORB_HIPCHK(hipSetDevice(device));
        ORB_HIPCHK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        ORB_HIPCHK(hipEventCreateWithFlags(&done, hipEventDisableTiming));
        const size_t E = (size_t)std::max<long long>(maxEntries, 1), N = (size_t)maxKF;
        for (int b = 0; b < 2; ++b) {
            ORB_HIPCHK(hipMalloc(&d_poolW[b], E * 4));
            ORB_HIPCHK(hipMalloc(&d_poolV[b], E * 8));
        }
        ORB_HIPCHK(hipMalloc(&d_off, N * 4));
        ORB_HIPCHK(hipMalloc(&d_len, N * 4));
        ORB_HIPCHK(hipMalloc(&d_newOff, N * 4));
        ORB_HIPCHK(hipMalloc(&d_cov, N * KFDB_MAX_COV * 4));
        ORB_HIPCHK(hipMalloc(&d_seq, N * 4));
        ORB_HIPCHK(hipMalloc(&d_reloc, N * 4));
        ORB_HIPCHK(hipMalloc(&d_covN, N));
        ORB_HIPCHK(hipMalloc(&d_conn, N));
        while ((size_t)pstride < N) pstride <<= 1;
        ORB_HIPCHK(hipMalloc(&d_qbuf, 16 + (size_t)KFDB_MAX_WORDS * 12));
        resOff = (std::max(16 + (size_t)KFDB_MAX_WORDS * 12, N) + 255) & ~(size_t)255;
        ORB_HIPCHK(hipHostMalloc(&h_stage, resOff + (N + 1) * 4, hipHostMallocDefault));
        int st = reset_device(stream);
        if (st) return st;
        ORB_HIPCHK(hipMemsetAsync(d_cov, 0xFF, N * KFDB_MAX_COV * 4, stream));
        ORB_HIPCHK(hipStreamSynchronize(stream));
        return reserve_queries(1);
    }

    int reserve_queries(int Q) {
        if (Q <= qCap) return ORB_OK;
        int st = wait_pending();  // the scratch may still be in use
        if (st) return st;
        (void)hipFree(d_common);
        (void)hipFree(d_first);
        (void)hipFree(d_score);
        (void)hipFree(d_scored);
        (void)hipFree(d_si);
        (void)hipFree(d_acc);
        (void)hipFree(d_bestKF);
        (void)hipFree(d_firstPos);
        (void)hipFree(d_entry);
        (void)hipFree(d_key);
        (void)hipFree(d_pay);
        d_common = d_bestKF = d_firstPos = d_pay = nullptr;
        d_first = nullptr;
        d_score = nullptr;
        d_scored = d_entry = nullptr;
        d_si = d_acc = nullptr;
        d_key = nullptr;
        qCap = 0;
        lastQ = 0;
        const size_t n = (size_t)Q * maxKF, np = (size_t)Q * pstride;
        ORB_HIPCHK(hipMalloc(&d_common, n * 4));
        ORB_HIPCHK(hipMalloc(&d_first, n * 4));
        ORB_HIPCHK(hipMalloc(&d_score, n * 8));
        ORB_HIPCHK(hipMalloc(&d_scored, n));
        ORB_HIPCHK(hipMalloc(&d_si, n * 4));
        ORB_HIPCHK(hipMalloc(&d_acc, n * 4));
        ORB_HIPCHK(hipMalloc(&d_bestKF, n * 4));
        ORB_HIPCHK(hipMalloc(&d_firstPos, n * 4));
        ORB_HIPCHK(hipMalloc(&d_entry, n));
        ORB_HIPCHK(hipMalloc(&d_key, np * 8));
        ORB_HIPCHK(hipMalloc(&d_pay, np * 4));
        qCap = Q;
        return ORB_OK;
    }

    // Live keyframes, in pool order, to the front of the other buffer.
    int compact(hipStream_t s) {
        std::vector<int> order;
        for (int i = 0; i < hi; ++i)
            if (len[i] > 0) order.push_back(i);
        std::sort(order.begin(), order.end(), [&](int a, int b) { return off[a] < off[b]; });
        std::vector<int> newOff(off.begin(), off.begin() + hi);
        long long t = 0;
        for (int i : order) {
            newOff[i] = (int)t;
            t += len[i];
        }
        if (hi > 0) {
            ORB_HIPCHK(hipMemcpyAsync(d_newOff, newOff.data(), (size_t)hi * 4, hipMemcpyHostToDevice, s));
            ORB_HIPCHK(hipStreamSynchronize(s));  // newOff is a local
            hipLaunchKernelGGL(k_kfdb_compact, dim3(std::min((hi + 3) / 4, 1024)), dim3(256), 0, s, hi, d_len, d_off,
                               d_newOff, d_poolW[cur], d_poolV[cur], d_poolW[cur ^ 1], d_poolV[cur ^ 1]);
            ORB_HIPCHK(hipGetLastError());
            ORB_HIPCHK(hipMemcpyAsync(d_off, d_newOff, (size_t)hi * 4, hipMemcpyDeviceToDevice, s));
            std::copy(newOff.begin(), newOff.end(), off.begin());
        }
        cur ^= 1;
        tail = t;
        return ORB_OK;
    }

    // Slots for `B` new keyframes of lens[b] entries (validated by the caller): compacts when the
    // tail has no room, assigns offsets and sequence numbers, writes the slots on the device and,
    // with srcW, copies frame src[b] of a batched transform into the pool.
    int place(int B, const int* ids, const int* lens, const uint32_t* srcW, const double* srcV, int cap,
              hipStream_t s, std::vector<int>* offs) {
        long long sum = 0;
        for (int b = 0; b < B; ++b) sum += lens[b];
        if (tail + sum > maxEntries) {
            int st = compact(s);
            if (st) return st;
        }
        for (int b0 = 0; b0 < B; b0 += KFDB_ADD_CHUNK) {
            AddChunk c;
            c.n = std::min(KFDB_ADD_CHUNK, B - b0);
            int maxLen = 0;
            for (int k = 0; k < c.n; ++k) {
                const int b = b0 + k, id = ids[b];
                c.slot[k] = id;
                c.off[k] = (int)tail;
                c.len[k] = lens[b];
                c.src[k] = b;
                c.seq[k] = nextSeq;
                off[id] = (int)tail;
                len[id] = lens[b];
                seq[id] = nextSeq++;
                if (offs) offs->push_back((int)tail);
                tail += lens[b];
                liveEntries += lens[b];
                ++nLive;
                hi = std::max(hi, id + 1);
                maxLen = std::max(maxLen, lens[b]);
            }
            const int gx = srcW ? std::max(1, std::min((maxLen + 255) / 256, 8)) : 1;
            hipLaunchKernelGGL(k_kfdb_add, dim3(gx, c.n), dim3(256), 0, s, c, srcW, srcV, cap, d_poolW[cur], d_poolV[cur],
                               d_off, d_len, d_seq, d_reloc);
            ORB_HIPCHK(hipGetLastError());
        }
        return ORB_OK;
    }

    int check_new_ids(int B, const int* ids, const int* lens, const char* what) {
        long long sum = 0;
        for (int b = 0; b < B; ++b) {
            const int id = ids[b];
            if (id < 0 || id >= maxKF)
                return fail(ORB_EINVAL, std::string(what) + ": keyframe id " + std::to_string(id) +
                                            " is out of range [0, " + std::to_string(maxKF) + ")");
            if (len[id] >= 0)
                return fail(ORB_EINVAL, std::string(what) + ": keyframe id " + std::to_string(id) + " is already live");
            for (int a = 0; a < b; ++a)
                if (ids[a] == id)
                    return fail(ORB_EINVAL, std::string(what) + ": keyframe id " + std::to_string(id) + " is given twice");
            sum += lens[b];
        }
        if (liveEntries + sum > maxEntries)
            return fail(ORB_ERANGE, std::string(what) + ": " + std::to_string(liveEntries) + " live entries + " +
                                        std::to_string(sum) + " do not fit max_entries " + std::to_string(maxEntries));
        return ORB_OK;
    }

    // Scan + selection of Q queries in the batched-transform layout; results on the device.
    int query(int Q, const uint32_t* d_w, const double* d_v, const int* d_n, int cap, int loop, float minScore,
              int* d_out, int outCap, int* d_nout, hipStream_t s) {
        int st = reserve_queries(Q);
        if (st) return st;
        lastQ = Q;
        if (hi > 0) {
            const int ldsCap = std::max(1, std::min(cap, KFDB_LDS_WORDS));
            const int gx = std::max(1, std::min((hi + 3) / 4, std::max(8, 2048 / Q)));
            hipLaunchKernelGGL(k_kfdb_scan, dim3(gx, Q), dim3(256), (size_t)ldsCap * 12, s, d_poolW[cur], d_poolV[cur],
                               d_off, d_len, hi, d_w, d_v, d_n, cap, ldsCap, d_common, d_first, d_score, maxKF);
            ORB_HIPCHK(hipGetLastError());
        }
        SelArgs A;
        A.hi = hi;
        A.stride = maxKF;
        A.pstride = pstride;
        A.Q = Q;
        A.loop = loop;
        A.minScore = minScore;
        A.len = d_len;
        A.seq = d_seq;
        A.cov = d_cov;
        A.covN = d_covN;
        A.reloc = d_reloc;
        A.connected = d_conn;
        A.common = d_common;
        A.first = d_first;
        A.score = d_score;
        A.scored = d_scored;
        A.si = d_si;
        A.acc = d_acc;
        A.bestKF = d_bestKF;
        A.entry = d_entry;
        A.firstPos = d_firstPos;
        A.key = d_key;
        A.pay = d_pay;
        A.outIds = d_out;
        A.outCap = outCap;
        A.nOut = d_nout;
        if (Q == 1) {
            hipLaunchKernelGGL(k_kfdb_query1, dim3(1), dim3(KFDB_SEL_THREADS), 0, s, A);
        } else {
            hipLaunchKernelGGL(k_kfdb_prepare, dim3(Q), dim3(KFDB_SEL_THREADS), 0, s, A);
            if (!loop && hi > 0) hipLaunchKernelGGL(k_kfdb_chain, dim3((hi + 255) / 256), dim3(256), 0, s, A);
            hipLaunchKernelGGL(k_kfdb_select, dim3(Q), dim3(KFDB_SEL_THREADS), 0, s, A);
        }
        ORB_HIPCHK(hipGetLastError());
        return ORB_OK;
    }

    int host_query(const uint32_t* words, const double* values, int n, int loop, const int32_t* connected,
                   int n_connected, float minScore, int32_t* out_ids, int out_cap, int* n_out) {
        if (!n_out || out_cap < 0 || (out_cap > 0 && !out_ids)) return fail(ORB_EINVAL, "bad output arguments");
        *n_out = 0;
        int st = check_bow(words, values, n, nWords, "query");
        if (st) return st;
        if (loop && (n_connected < 0 || (n_connected > 0 && !connected)))
            return fail(ORB_EINVAL, "bad connected_ids");
        if (n == 0 || nLive == 0) {
            lastQ = 0;
            return ORB_OK;
        }
        const hipStream_t s = stream;
        st = enter_host();
        if (st) return st;
        if (loop) {
            std::memset(h_stage, 0, (size_t)hi);
            for (int i = 0; i < n_connected; ++i)
                if (connected[i] >= 0 && connected[i] < hi) h_stage[connected[i]] = 1;
            ORB_HIPCHK(hipMemcpyAsync(d_conn, h_stage, (size_t)hi, hipMemcpyHostToDevice, s));
            ORB_HIPCHK(hipStreamSynchronize(s));  // the staging buffer is reused for the query
        }
        const size_t qbytes = 16 + (size_t)n * 12;
        std::memcpy(h_stage, &n, 4);
        std::memcpy(h_stage + 16, values, (size_t)n * 8);
        std::memcpy(h_stage + 16 + (size_t)n * 8, words, (size_t)n * 4);
        ORB_HIPCHK(hipMemcpyAsync(d_qbuf, h_stage, qbytes, hipMemcpyHostToDevice, s));
        // the candidates and their count go straight to the pinned buffer: no copy back
        int32_t* res = (int32_t*)(h_stage + resOff);
        st = query(1, (const uint32_t*)(d_qbuf + 16 + (size_t)n * 8), (const double*)(d_qbuf + 16), (const int*)d_qbuf,
                   n, loop, minScore, res + 1, maxKF, res, s);
        if (st) return st;
        ORB_HIPCHK(hipStreamSynchronize(s));
        const int cnt = res[0];
        *n_out = cnt;
        if (cnt > out_cap)
            return fail(ORB_ERANGE, std::to_string(cnt) + " candidates do not fit out_cap " + std::to_string(out_cap));
        if (cnt > 0) std::memcpy(out_ids, res + 1, (size_t)cnt * 4);
        return ORB_OK;
    }
};

extern "C" {

int orb_vocabulary_score(const orb_vocabulary_t* v, const uint32_t* words1, const double* values1, int n1,
                         const uint32_t* words2, const double* values2, int n2, double* score) {
    if (!score) return fail(ORB_EINVAL, "score is NULL");
    int nWords = 0;
    int st = check_l1(v, &nWords);
    if (st) return st;
    if (n1 < 0 || n2 < 0 || (n1 > 0 && (!words1 || !values1)) || (n2 > 0 && (!words2 || !values2)))
        return fail(ORB_EINVAL, "bad BowVector arrays");
    *score = l1_score_host(words1, values1, n1, words2, values2, n2);
    return ORB_OK;
}

int orb_vocabulary_score_pairs_device(const orb_vocabulary_t* v, int P, const uint32_t* d_bow_words,
                                      const double* d_bow_values, const int32_t* d_bow_n, int cap,
                                      const int32_t* d_pair_a, const int32_t* d_pair_b, double* d_score, void* stream) {
    int st = check_l1(v, nullptr);
    if (st) return st;
    if (P < 0 || cap <= 0 || (P > 0 && (!d_bow_words || !d_bow_values || !d_bow_n || !d_pair_a || !d_pair_b || !d_score)))
        return fail(ORB_EINVAL, "bad arguments");
    if (cap > KFDB_MAX_WORDS) return fail(ORB_ENOTSUP, "more than 8192 words in a BowVector");
    if (P == 0) return ORB_OK;
    ORB_HIPCHK(hipSetDevice(orb_internal_vocabulary_device(v)));
    hipLaunchKernelGGL(k_kfdb_pairs, dim3((P + 3) / 4), dim3(256), 0, (hipStream_t)stream, P, d_bow_words,
                       d_bow_values, d_bow_n, cap, d_pair_a, d_pair_b, d_score);
    ORB_HIPCHK(hipGetLastError());
    return ORB_OK;
}

int orb_kfdb_create(const orb_vocabulary_t* voc, int max_keyframes, int64_t max_entries, int device,
                    orb_keyframe_db_t** out) {
    if (!out) return fail(ORB_EINVAL, "out is NULL");
    *out = nullptr;
    int nWords = 0;
    int st = check_l1(voc, &nWords);
    if (st) return st;
    if (max_keyframes < 1 || max_keyframes > KFDB_MAX_KEYFRAMES)
        return fail(ORB_EINVAL, "max_keyframes must be in [1, 65536]");
    if (max_entries < 1 || max_entries > INT_MAX) return fail(ORB_EINVAL, "max_entries must be in [1, 2^31)");
    int ndev = 0;
    ORB_HIPCHK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(ORB_EINVAL, "device ordinal out of range");
    auto* db = new orb_keyframe_db();
    db->nWords = nWords;
    db->device = device;
    db->maxKF = max_keyframes;
    db->maxEntries = max_entries;
    db->off.assign(max_keyframes, 0);
    db->len.assign(max_keyframes, -1);
    db->seq.assign(max_keyframes, 0u);
    st = db->alloc();
    if (st) {
        db->release();
        delete db;
        return st;
    }
    *out = db;
    return ORB_OK;
}

int orb_kfdb_destroy(orb_keyframe_db_t* db) {
    if (!db) return ORB_OK;
    db->release();
    delete db;
    return ORB_OK;
}

int orb_kfdb_clear(orb_keyframe_db_t* db) {
    if (!db) return fail(ORB_EINVAL, "NULL database");
    std::lock_guard<std::mutex> lock(db->mu);
    int st = db->enter_host();
    if (st) return st;
    st = db->reset_device(db->stream);
    if (st) return st;
    ORB_HIPCHK(hipStreamSynchronize(db->stream));
    std::fill(db->len.begin(), db->len.end(), -1);
    std::fill(db->off.begin(), db->off.end(), 0);
    std::fill(db->seq.begin(), db->seq.end(), 0u);
    db->hi = 0;
    db->nLive = 0;
    db->liveEntries = 0;
    db->tail = 0;
    db->lastQ = 0;
    return ORB_OK;
}

int orb_kfdb_size(const orb_keyframe_db_t* db) {
    if (!db) return fail(ORB_EINVAL, "NULL database");
    return db->nLive;
}

int orb_kfdb_add(orb_keyframe_db_t* db, int id, const uint32_t* words, const double* values, int n) {
    if (!db) return fail(ORB_EINVAL, "NULL database");
    std::lock_guard<std::mutex> lock(db->mu);
    int st = check_bow(words, values, n, db->nWords, "add");
    if (st) return st;
    st = db->check_new_ids(1, &id, &n, "add");
    if (st) return st;
    const hipStream_t s = db->stream;
    st = db->enter_host();
    if (st) return st;
    std::vector<int> offs;
    st = db->place(1, &id, &n, nullptr, nullptr, 0, s, &offs);
    if (st) return st;
    if (n > 0) {
        ORB_HIPCHK(hipMemcpyAsync(db->d_poolW[db->cur] + offs[0], words, (size_t)n * 4, hipMemcpyHostToDevice, s));
        ORB_HIPCHK(hipMemcpyAsync(db->d_poolV[db->cur] + offs[0], values, (size_t)n * 8, hipMemcpyHostToDevice, s));
    }
    ORB_HIPCHK(hipStreamSynchronize(s));
    return ORB_OK;
}

int orb_kfdb_add_batch_device(orb_keyframe_db_t* db, int B, const int32_t* ids, const uint32_t* d_bow_words,
                              const double* d_bow_values, const int32_t* d_bow_n, int cap, void* stream) {
    if (!db) return fail(ORB_EINVAL, "NULL database");
    if (B < 0 || cap <= 0 || (B > 0 && (!ids || !d_bow_words || !d_bow_values || !d_bow_n)))
        return fail(ORB_EINVAL, "bad arguments");
    if (B == 0) return ORB_OK;
    std::lock_guard<std::mutex> lock(db->mu);
    const hipStream_t s = (hipStream_t)stream;
    int st = db->enter_device(s);
    if (st) return st;
    std::vector<int> lens(B);
    ORB_HIPCHK(hipMemcpyAsync(lens.data(), d_bow_n, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    ORB_HIPCHK(hipStreamSynchronize(s));
    for (int b = 0; b < B; ++b) {
        if (lens[b] < 0 || lens[b] > cap) return fail(ORB_EINVAL, "add_batch_device: d_bow_n is not in [0, cap]");
        if (lens[b] > KFDB_MAX_WORDS) return fail(ORB_ENOTSUP, "add_batch_device: more than 8192 words in a BowVector");
    }
    st = db->check_new_ids(B, ids, lens.data(), "add_batch_device");
    if (st) return st;
    st = db->place(B, ids, lens.data(), d_bow_words, d_bow_values, cap, s, nullptr);
    return st ? st : db->leave_device(s);
}

int orb_kfdb_erase(orb_keyframe_db_t* db, int id) {
    if (!db) return fail(ORB_EINVAL, "NULL database");
    std::lock_guard<std::mutex> lock(db->mu);
    if (id < 0 || id >= db->maxKF || db->len[id] < 0) return ORB_OK;
    const hipStream_t s = db->stream;
    int st = db->enter_host();
    if (st) return st;
    AddChunk c;
    c.n = 1;
    c.slot[0] = id;
    c.off[0] = 0;
    c.len[0] = -1;
    c.src[0] = 0;
    c.seq[0] = 0;
    hipLaunchKernelGGL(k_kfdb_add, dim3(1, 1), dim3(256), 0, s, c, (const uint32_t*)nullptr, (const double*)nullptr, 0,
                       db->d_poolW[db->cur], db->d_poolV[db->cur], db->d_off, db->d_len, db->d_seq, db->d_reloc);
    ORB_HIPCHK(hipGetLastError());
    ORB_HIPCHK(hipStreamSynchronize(s));
    db->liveEntries -= db->len[id];
    db->len[id] = -1;
    db->off[id] = 0;
    db->seq[id] = 0;
    if (--db->nLive == 0) db->tail = 0;
    return ORB_OK;
}

int orb_kfdb_set_covisible(orb_keyframe_db_t* db, int id, const int32_t* neighbour_ids, int n) {
    if (!db) return fail(ORB_EINVAL, "NULL database");
    std::lock_guard<std::mutex> lock(db->mu);
    if (id < 0 || id >= db->maxKF)
        return fail(ORB_EINVAL, "set_covisible: keyframe id " + std::to_string(id) + " is out of range");
    if (n < 0 || n > KFDB_MAX_COV || (n > 0 && !neighbour_ids))
        return fail(ORB_EINVAL, "set_covisible: n must be in [0, 10]");
    CovArgs a;
    a.slot = id;
    a.n = n;
    for (int i = 0; i < KFDB_MAX_COV; ++i) a.ids[i] = -1;
    for (int i = 0; i < n; ++i) {
        if (neighbour_ids[i] < 0 || neighbour_ids[i] >= db->maxKF)
            return fail(ORB_EINVAL, "set_covisible: neighbour id " + std::to_string(neighbour_ids[i]) + " is out of range");
        a.ids[i] = neighbour_ids[i];
    }
    const hipStream_t s = db->stream;
    int st = db->enter_host();
    if (st) return st;
    hipLaunchKernelGGL(k_kfdb_set_cov, dim3(1), dim3(64), 0, s, a, db->d_cov, db->d_covN);
    ORB_HIPCHK(hipGetLastError());
    ORB_HIPCHK(hipStreamSynchronize(s));
    return ORB_OK;
}

int orb_kfdb_detect_relocalisation_candidates(orb_keyframe_db_t* db, const uint32_t* words, const double* values,
                                              int n, int32_t* out_ids, int out_cap, int* n_out) {
    if (!db) return fail(ORB_EINVAL, "NULL database");
    std::lock_guard<std::mutex> lock(db->mu);
    return db->host_query(words, values, n, 0, nullptr, 0, 0.0f, out_ids, out_cap, n_out);
}

int orb_kfdb_detect_loop_candidates(orb_keyframe_db_t* db, const uint32_t* words, const double* values, int n,
                                    const int32_t* connected_ids, int n_connected, float min_score, int32_t* out_ids,
                                    int out_cap, int* n_out) {
    if (!db) return fail(ORB_EINVAL, "NULL database");
    std::lock_guard<std::mutex> lock(db->mu);
    return db->host_query(words, values, n, 1, connected_ids, n_connected, min_score, out_ids, out_cap, n_out);
}

int orb_kfdb_detect_relocalisation_candidates_batch_device(orb_keyframe_db_t* db, int Q, const uint32_t* d_bow_words,
                                                           const double* d_bow_values, const int32_t* d_bow_n,
                                                           int cap, int32_t* d_out_ids, int out_cap,
                                                           int32_t* d_n_out, void* stream) {
    if (!db) return fail(ORB_EINVAL, "NULL database");
    if (Q < 0 || cap <= 0 || out_cap < 0 ||
        (Q > 0 && (!d_bow_words || !d_bow_values || !d_bow_n || !d_n_out || (out_cap > 0 && !d_out_ids))))
        return fail(ORB_EINVAL, "bad arguments");
    if (cap > KFDB_MAX_WORDS) return fail(ORB_ENOTSUP, "more than 8192 words in a BowVector");
    if (Q > 65535) return fail(ORB_ENOTSUP, "more than 65535 queries in a batch");
    if (Q == 0) return ORB_OK;
    std::lock_guard<std::mutex> lock(db->mu);
    const hipStream_t s = (hipStream_t)stream;
    int st = db->enter_device(s);
    if (st) return st;
    st = db->query(Q, d_bow_words, d_bow_values, d_bow_n, cap, 0, 0.0f, d_out_ids, out_cap, d_n_out, s);
    return st ? st : db->leave_device(s);
}

int orb_debug_kfdb_last_query(orb_keyframe_db_t* db, int q, int32_t* common, uint32_t* first_word, uint32_t* seq,
                              uint8_t* scored, double* score, int cap) {
    if (!db) return fail(ORB_EINVAL, "NULL database");
    std::lock_guard<std::mutex> lock(db->mu);
    if (q < 0 || q >= db->lastQ) return fail(ORB_EINVAL, "no such query in the last call");
    if (cap < 0 || (cap > 0 && (!common || !first_word || !seq || !scored || !score)))
        return fail(ORB_EINVAL, "bad arguments");
    int st = db->enter_host();
    if (st) return st;
    const int n = std::min(cap, db->hi);
    if (n > 0) {
        const size_t o = (size_t)q * db->maxKF;
        ORB_HIPCHK(hipMemcpy(common, db->d_common + o, (size_t)n * 4, hipMemcpyDeviceToHost));
        ORB_HIPCHK(hipMemcpy(first_word, db->d_first + o, (size_t)n * 4, hipMemcpyDeviceToHost));
        ORB_HIPCHK(hipMemcpy(score, db->d_score + o, (size_t)n * 8, hipMemcpyDeviceToHost));
        ORB_HIPCHK(hipMemcpy(scored, db->d_scored + o, (size_t)n, hipMemcpyDeviceToHost));
        std::copy(db->seq.begin(), db->seq.begin() + n, seq);
    }
    return n;
}

}  // extern "C"
