// orb_initializer.hip — the two-view model scoring of Initializer on the GPU (part of liborb_hip.so).
//
// Initializer::CheckHomography (reference src/Initializer.cc:303-386) and CheckFundamental
// (388-466) for every RANSAC hypothesis of a frame pair at once, plus the "keep the best" rule of
// FindHomography / FindFundamental (146-169, 197-220).  The hypotheses themselves (ComputeH21 /
// ComputeF21, cv::SVDecomp) are the caller's.
//
// Arithmetic: plain float, the TU is built -ffp-contract=off and the fused multiply-adds that
// g++ -O3 -march=native makes of the reference's expressions are written out
// (scripts/contraction_check_initializer.sh prints the disassembly they are read from):
//   a*x + b*y + c              ->  fmaf(a, x, b*y) + c
//   u - p*winv                 ->  fmaf(-p, winv, u)
//   dx*dx + dy*dy, a*a + b*b   ->  fmaf(dx, dx, dy*dy)
//   1.0/(float)                ->  a float divide (correctly rounded; equal to the double divide
//                                  rounded to float for every float divisor)
// `score` is ONE float accumulated in match order, first-image term before second-image term;
// the terms are computed in parallel, the adds of one hypothesis form one chain on one lane.
//
//   k_init_scores  one workgroup per (pair, model, tile of 64 hypotheses), 5 waves.  All waves
//                  compact the pair's matches in index order (ballot + prefix) and stage
//                  (u1, v1, u2, v2) in LDS.  Waves 1-4 then compute the terms of a 16-match chunk,
//                  lane = hypothesis (its matrix in registers, the match an LDS broadcast), into
//                  one half of a double buffer laid out [match][term][hypothesis]; wave 0 meanwhile
//                  adds the previous chunk's terms in reference order, lane = hypothesis.  One
//                  barrier per chunk.
//   k_init_best    one workgroup per (pair, model): the first maximum above 0 of the scores
//                  (strict >, NaN never wins), then the winner's inlier flags recomputed with a
//                  thread per match, written by match ordinal.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/orb_abi.h"
#include "orb_internal.h"

namespace {

int fail(int code, const std::string& msg) { return orb_internal_set_error(code, msg); }

constexpr int IN_MAX_CAP = 8192;
constexpr int IN_MAX_HYP = 1024;
constexpr int IN_TILE = 64;                          // hypotheses per workgroup = lanes of the chain wave
constexpr int IN_CHUNK = 16;                         // matches per pipeline step
constexpr int IN_CWAVES = 4;                         // compute waves (waves 1 .. IN_CWAVES)
constexpr int IN_THREADS = 64 * (1 + IN_CWAVES);     // 320
constexpr int IN_TERM_BYTES = 2 * IN_CHUNK * 2 * IN_TILE * 4;  // the double buffer: 16 KiB
constexpr int IN_BEST_THREADS = 256;

constexpr float TH_H = 5.991f;        // CheckHomography: test and score (Initializer.cc:331)
constexpr float TH_F = 3.841f;        // CheckFundamental: test (406)
constexpr float TH_SCORE = 5.991f;    //                   score (407)

struct InitArgs {
    const orb_keypoint_t* kps;
    const int32_t* counts;
    const int32_t* pair_f1;
    const int32_t* pair_f2;
    const int32_t* matches12;
    const float* M21[2];   // [0] H21, [1] F21 (P x n_hyp x 9); NULL = model absent
    const float* H12;
    float* scores[2];      // P x n_hyp (never NULL for a present model)
    int32_t* best[2];
    float* best_score[2];
    uint8_t* inliers[2];   // P x cap
    int32_t* n_matches;
    int cap, P, n_hyp;
    float inv_sigma2;
};

// chi-square of one reprojection, CheckHomography (Initializer.cc:350-356 / 366-372): (u, v)
// through the row-major 3x3 `m`, measured against (ut, vt).
__device__ __forceinline__ float chi_h(const float* m, float u, float v, float ut, float vt, float inv_s2) {
    const float winv = 1.0f / (__builtin_fmaf(m[6], u, m[7] * v) + m[8]);
    const float pu = __builtin_fmaf(m[0], u, m[1] * v) + m[2];
    const float pv = __builtin_fmaf(m[3], u, m[4] * v) + m[5];
    const float du = __builtin_fmaf(-pu, winv, ut);
    const float dv = __builtin_fmaf(-pv, winv, vt);
    return __builtin_fmaf(du, du, dv * dv) * inv_s2;
}

// chi-square of one epipolar distance, CheckFundamental (426-434 with m = F21, 444-452 with m =
// F21 transposed and the points swapped): the line m * (u, v, 1), distance of (ut, vt) to it.
__device__ __forceinline__ float chi_f(const float* m, float u, float v, float ut, float vt, float inv_s2) {
    const float a = __builtin_fmaf(m[0], u, m[1] * v) + m[2];
    const float b = __builtin_fmaf(m[3], u, m[4] * v) + m[5];
    const float c = __builtin_fmaf(m[6], u, m[7] * v) + m[8];
    const float num = __builtin_fmaf(a, ut, b * vt) + c;
    const float den = __builtin_fmaf(a, a, b * b);
    return num * num / den * inv_s2;
}

// The two matrices a lane needs for hypothesis `g` (= pair * n_hyp + hypothesis) of `model`:
// A serves the first-image term, B the second-image term.
__device__ __forceinline__ void load_model(const InitArgs& a, int model, long long g, float* A, float* B) {
    if (model == 0) {  // A = H12 (x2 into image 1), B = H21 (x1 into image 2)
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            A[k] = a.H12[g * 9 + k];
            B[k] = a.M21[0][g * 9 + k];
        }
    } else {  // A = F21 (l2 = F21 x1), B = F21^T (l1 = x2^T F21)
#pragma unroll
        for (int k = 0; k < 9; ++k) A[k] = a.M21[1][g * 9 + k];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) B[r * 3 + c] = A[c * 3 + r];
    }
}

// Both chi-squares of one match, in the reference's order.
__device__ __forceinline__ void chi_pair(int model, const float* A, const float* B, float4 p, float inv_s2,
                                         float* c1, float* c2) {
    if (model == 0) {
        *c1 = chi_h(A, p.z, p.w, p.x, p.y, inv_s2);
        *c2 = chi_h(B, p.x, p.y, p.z, p.w, inv_s2);
    } else {
        *c1 = chi_f(A, p.x, p.y, p.z, p.w, inv_s2);
        *c2 = chi_f(B, p.z, p.w, p.x, p.y, inv_s2);
    }
}

// The frames and clamped counts of pair p.  An entry of matches12 is a match only when it lies
// in [0, n2) and its index is below n1, so no read leaves the frames' rows.
struct PairView {
    const orb_keypoint_t* k1;
    const orb_keypoint_t* k2;
    const int32_t* m12;
    int n1, n2;
};
__device__ __forceinline__ PairView pair_view(const InitArgs& a, int p) {
    const int f1 = a.pair_f1[p], f2 = a.pair_f2[p];
    PairView v;
    v.k1 = a.kps + (size_t)f1 * a.cap;
    v.k2 = a.kps + (size_t)f2 * a.cap;
    v.m12 = a.matches12 + (size_t)p * a.cap;
    v.n1 = min(max(a.counts[f1], 0), a.cap);
    v.n2 = min(max(a.counts[f2], 0), a.cap);
    return v;
}

// mvMatches12 (Initializer.cc:54-63) in index order, NT threads: calls emit(ordinal, i, m) for every
// match and returns N.  s_wtot: one int per wave.  Uniform control flow (barriers inside).
template <int NT, class F>
__device__ __forceinline__ int compact_matches(const PairView& v, int* s_wtot, F emit) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int base = 0;
    for (int i0 = 0; i0 < v.n1; i0 += NT) {
        const int i = i0 + tid;
        const int m = i < v.n1 ? v.m12[i] : -1;
        const bool ok = (unsigned)m < (unsigned)v.n2;
        const unsigned long long bal = __ballot(ok);
        if (lane == 0) s_wtot[wave] = __popcll(bal);
        __syncthreads();
        int off = base, tot = 0;
#pragma unroll
        for (int w = 0; w < NT / 64; ++w) {
            const int t = s_wtot[w];
            if (w < wave) off += t;
            tot += t;
        }
        if (ok) emit(off + __popcll(bal & ((1ull << lane) - 1ull)), i, m);
        base += tot;
        __syncthreads();
    }
    return base;
}

__global__ void __launch_bounds__(IN_THREADS) k_init_scores(InitArgs a, int tiles) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    __shared__ int s_wtot[IN_THREADS / 64];
    const int model = blockIdx.y;
    if (!a.M21[model]) return;
    const int p = blockIdx.x / tiles, tile = blockIdx.x - p * tiles;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float* s_term = (float*)smem;                       // [2][IN_CHUNK][2][IN_TILE]
    float4* s_pts = (float4*)(smem + IN_TERM_BYTES);    // cap entries

    const PairView v = pair_view(a, p);
    const int N = compact_matches<IN_THREADS>(v, s_wtot, [&](int o, int i, int m) {
        s_pts[o] = make_float4(v.k1[i].x, v.k1[i].y, v.k2[m].x, v.k2[m].y);
    });
    // (the last barrier of compact_matches orders the staging before the reads below; N == 0
    // needs none)

    const int h = tile * IN_TILE + lane;
    const bool hv = h < a.n_hyp;
    const long long g = (long long)p * a.n_hyp + (hv ? h : a.n_hyp - 1);  // a tail lane repeats the last one
    float A[9], B[9];
    if (wave > 0) load_model(a, model, g, A, B);
    const float th = model == 0 ? TH_H : TH_F;
    float score = 0.0f;
#ifdef ORB_INIT_PLAIN
    // Measurement variant (scripts/build_variant.sh plain -DORB_INIT_PLAIN): the
    // reference loop as it stands, one lane per hypothesis over all matches, waves 2-4 idle.
    if (wave == 1) {
        for (int idx = 0; idx < N; ++idx) {
            float c1, c2;
            chi_pair(model, A, B, s_pts[idx], a.inv_sigma2, &c1, &c2);
            if (!(c1 > th)) score += TH_SCORE - c1;
            if (!(c2 > th)) score += TH_SCORE - c2;
        }
        if (hv) a.scores[model][(size_t)p * a.n_hyp + h] = score;
    }
    return;
#endif
    const int nchunks = (N + IN_CHUNK - 1) / IN_CHUNK;
    for (int k = 0; k <= nchunks; ++k) {
        if (wave > 0) {
            if (k < nchunks) {
                float* buf = s_term + (k & 1) * (IN_CHUNK * 2 * IN_TILE);
                for (int j = wave - 1; j < IN_CHUNK; j += IN_CWAVES) {
                    const int idx = k * IN_CHUNK + j;
                    if (idx < N) {
                        float c1, c2;
                        chi_pair(model, A, B, s_pts[idx], a.inv_sigma2, &c1, &c2);
                        // A rejected term is stored as +0.0f and added by the chain: exact, because
                        // score is only ever +0, positive or NaN (every accepted term thScore - chi
                        // is >= +0, chi <= th <= thScore), and x + (+0) == x for all of those.  A NaN
                        // chi is not > th: it stays and makes the score NaN.
                        buf[(j * 2 + 0) * IN_TILE + lane] = c1 > th ? 0.0f : TH_SCORE - c1;
                        buf[(j * 2 + 1) * IN_TILE + lane] = c2 > th ? 0.0f : TH_SCORE - c2;
                    }
                }
            }
        } else if (k > 0) {
            const float* buf = s_term + ((k - 1) & 1) * (IN_CHUNK * 2 * IN_TILE);
            const int cnt = min(IN_CHUNK, N - (k - 1) * IN_CHUNK);
            if (cnt == IN_CHUNK) {
                float t[2 * IN_CHUNK];
#pragma unroll
                for (int j = 0; j < 2 * IN_CHUNK; ++j) t[j] = buf[j * IN_TILE + lane];
#pragma unroll
                for (int j = 0; j < 2 * IN_CHUNK; ++j) score += t[j];
            } else {
                for (int j = 0; j < 2 * cnt; ++j) score += buf[j * IN_TILE + lane];
            }
        }
        __syncthreads();
    }
    if (wave == 0 && hv) a.scores[model][(size_t)p * a.n_hyp + h] = score;
}

__global__ void __launch_bounds__(IN_BEST_THREADS) k_init_best(InitArgs a) {
    __shared__ int s_wtot[IN_BEST_THREADS / 64];
    __shared__ float s_bs[IN_BEST_THREADS];
    __shared__ int s_bi[IN_BEST_THREADS];
    const int model = blockIdx.y, p = blockIdx.x, tid = threadIdx.x;
    if (!a.M21[model]) return;
    // FindHomography / FindFundamental (Initializer.cc:135, 163-168): score = 0.0, replaced on a
    // strict >.  Per thread over its ascending strided subset, then combined: the greater score,
    // the lower index between equal ones (an index of -1 only goes with score 0).
    const float* sc = a.scores[model] + (size_t)p * a.n_hyp;
    float bs = 0.0f;
    int bi = -1;
    for (int h = tid; h < a.n_hyp; h += IN_BEST_THREADS) {
        const float s = sc[h];
        if (s > bs) {
            bs = s;
            bi = h;
        }
    }
    s_bs[tid] = bs;
    s_bi[tid] = bi;
    __syncthreads();
    for (int step = IN_BEST_THREADS / 2; step > 0; step >>= 1) {
        if (tid < step) {
            const float os = s_bs[tid + step];
            const int oi = s_bi[tid + step];
            if (os > s_bs[tid] || (os == s_bs[tid] && oi >= 0 && oi < s_bi[tid])) {
                s_bs[tid] = os;
                s_bi[tid] = oi;
            }
        }
        __syncthreads();
    }
    bs = s_bs[0];
    bi = s_bi[0];
    if (tid == 0) {
        if (a.best[model]) a.best[model][p] = bi;
        if (a.best_score[model]) a.best_score[model][p] = bs;
    }
    float A[9], B[9];
    if (bi >= 0) load_model(a, model, (long long)p * a.n_hyp + bi, A, B);
    const float th = model == 0 ? TH_H : TH_F;
    uint8_t* mask = a.inliers[model] ? a.inliers[model] + (size_t)p * a.cap : nullptr;
    const PairView v = pair_view(a, p);
    const int N = compact_matches<IN_BEST_THREADS>(v, s_wtot, [&](int o, int i, int m) {
        if (!mask) return;
        bool in = false;
        if (bi >= 0) {  // bIn of the winning hypothesis (Initializer.cc:337, 358-382)
            float c1, c2;
            chi_pair(model, A, B, make_float4(v.k1[i].x, v.k1[i].y, v.k2[m].x, v.k2[m].y), a.inv_sigma2, &c1, &c2);
            in = !(c1 > th) && !(c2 > th);
        }
        mask[o] = in ? 1 : 0;
    });
    // one writer: the first model present
    if (tid == 0 && a.n_matches && model == (a.M21[0] ? 0 : 1)) a.n_matches[p] = N;
}

// Enqueue both kernels on `st`.  `a.scores` of a present model must be set.
int launch(const InitArgs& a, hipStream_t st) {
    const int tiles = (a.n_hyp + IN_TILE - 1) / IN_TILE;
    const size_t lds = (size_t)IN_TERM_BYTES + (size_t)a.cap * sizeof(float4);
    if (lds > 48 * 1024)
        ORB_HIPCHK(hipFuncSetAttribute((const void*)k_init_scores, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       150 * 1024));
    hipLaunchKernelGGL(k_init_scores, dim3((unsigned)((size_t)a.P * tiles), 2), dim3(IN_THREADS), lds, st, a, tiles);
    ORB_HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_init_best, dim3(a.P, 2), dim3(IN_BEST_THREADS), 0, st, a);
    ORB_HIPCHK(hipGetLastError());
    return ORB_OK;
}

int check_limits(int cap, int n_hyp, bool has_h, bool has_f) {
    if (cap > IN_MAX_CAP) return fail(ORB_ENOTSUP, "initializer: more than 8192 keypoints per frame");
    if (n_hyp < 1 || n_hyp > IN_MAX_HYP)
        return fail(ORB_EINVAL, "initializer: n_hyp must be in [1, 1024] (got " + std::to_string(n_hyp) + ")");
    if (!has_h && !has_f) return fail(ORB_EINVAL, "initializer: neither homographies nor fundamental matrices given");
    return ORB_OK;
}

}  // namespace

extern "C" {

int orb_initializer_check_batch_device(const orb_keypoint_t* d_kps, const int32_t* d_counts, int cap, int P,
                                       const int32_t* d_pair_f1, const int32_t* d_pair_f2,
                                       const int32_t* d_matches12, float sigma, int n_hyp, const float* d_H21,
                                       const float* d_H12, const float* d_F21, float* d_scores_h, float* d_scores_f,
                                       int32_t* d_best_h, float* d_best_score_h, uint8_t* d_inliers_h,
                                       int32_t* d_best_f, float* d_best_score_f, uint8_t* d_inliers_f,
                                       int32_t* d_n_matches, void* stream) {
    if (P < 0 || cap <= 0) return fail(ORB_EINVAL, "initializer: bad arguments");
    if ((d_H21 == nullptr) != (d_H12 == nullptr))
        return fail(ORB_EINVAL, "initializer: H21 and H12 are given together or not at all");
    if (int r = check_limits(cap, n_hyp, d_H21 != nullptr, d_F21 != nullptr)) return r;
    if (P == 0) return ORB_OK;
    if (P > 65535) return fail(ORB_ENOTSUP, "initializer: more than 65535 pairs per call");
    if (!d_kps || !d_counts || !d_pair_f1 || !d_pair_f2 || !d_matches12)
        return fail(ORB_EINVAL, "initializer: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    InitArgs a{};
    a.kps = d_kps;
    a.counts = d_counts;
    a.pair_f1 = d_pair_f1;
    a.pair_f2 = d_pair_f2;
    a.matches12 = d_matches12;
    a.M21[0] = d_H21;
    a.M21[1] = d_F21;
    a.H12 = d_H12;
    a.scores[0] = d_scores_h;
    a.scores[1] = d_scores_f;
    a.best[0] = d_best_h;
    a.best[1] = d_best_f;
    a.best_score[0] = d_best_score_h;
    a.best_score[1] = d_best_score_f;
    a.inliers[0] = d_inliers_h;
    a.inliers[1] = d_inliers_f;
    a.n_matches = d_n_matches;
    a.cap = cap;
    a.P = P;
    a.n_hyp = n_hyp;
    a.inv_sigma2 = 1.0f / (sigma * sigma);  // Initializer.cc:333, 409
    // a model whose scores the caller does not want still needs them between the two kernels:
    // stream-ordered scratch, freed after the second kernel
    void* tmp[2] = {nullptr, nullptr};
    for (int m = 0; m < 2; ++m)
        if (a.M21[m] && !a.scores[m]) {
            hipError_t e = hipMallocAsync(&tmp[m], (size_t)P * n_hyp * sizeof(float), st);
            if (e != hipSuccess) {
                if (tmp[0]) (void)hipFreeAsync(tmp[0], st);
                return fail(ORB_ENOMEM, std::string("initializer: score scratch: ") + hipGetErrorString(e));
            }
            a.scores[m] = (float*)tmp[m];
        }
    const int r = launch(a, st);
    for (int m = 0; m < 2; ++m)
        if (tmp[m]) (void)hipFreeAsync(tmp[m], st);
    return r;
}

int orb_initializer_check(const orb_keypoint_t* kps1, int n1, const orb_keypoint_t* kps2, int n2,
                          const int32_t* matches12, float sigma, int n_hyp, const float* H21, const float* H12,
                          const float* F21, float* scores_h, float* scores_f, int32_t* best_h, float* best_score_h,
                          uint8_t* inliers_h, int32_t* best_f, float* best_score_f, uint8_t* inliers_f,
                          int* n_matches, int device) {
    if (n1 < 0 || n2 < 0 || (n1 && (!kps1 || !matches12)) || (n2 && !kps2))
        return fail(ORB_EINVAL, "initializer: bad arguments");
    if ((H21 == nullptr) != (H12 == nullptr))
        return fail(ORB_EINVAL, "initializer: H21 and H12 are given together or not at all");
    const int cap = std::max(std::max(n1, n2), 1);
    if (int r = check_limits(cap, n_hyp, H21 != nullptr, F21 != nullptr)) return r;
    for (int i = 0; i < n1; ++i)
        if (matches12[i] < -1 || matches12[i] >= n2)
            return fail(ORB_EINVAL, "initializer: matches12[" + std::to_string(i) + "] = " +
                                        std::to_string(matches12[i]) + " is outside [-1, n2)");
    int ndev = 0;
    ORB_HIPCHK(hipGetDeviceCount(&ndev));
    if (device < 0) ORB_HIPCHK(hipGetDevice(&device));
    OrbHostCtx* C = device < ndev ? orb_internal_thread_ctx(device) : nullptr;
    if (!C) return fail(ORB_EINVAL, "device ordinal out of range");
    ORB_HIPCHK(hipSetDevice(device));
    // the pair as a 2-frame batch with one pair (0, 1); staging:
    // in:  [kps 2 x cap | counts 2, f1, f2 | matches12 cap | H21 | H12 | F21]
    // out: [scores_h | scores_f | best 2 | best_score 2 | n_matches | inliers 2 x cap]
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t hyp = (size_t)n_hyp * 9 * sizeof(float);
    const size_t oK = 0, oC = al(oK + 2 * (size_t)cap * sizeof(orb_keypoint_t)), oM = al(oC + 16),
                 oH21 = al(oM + (size_t)cap * 4), oH12 = al(oH21 + hyp), oF = al(oH12 + hyp), in_end = al(oF + hyp);
    const size_t oS = in_end, oB = al(oS + 2 * (size_t)n_hyp * 4), oI = al(oB + 20), total = al(oI + 2 * (size_t)cap);
    if (int r = C->reserve(total, total)) return r;
    uint8_t* hp = C->pinned;
    std::memset(hp, 0, in_end);
    if (n1) std::memcpy(hp + oK, kps1, (size_t)n1 * sizeof(orb_keypoint_t));
    if (n2) std::memcpy(hp + oK + (size_t)cap * sizeof(orb_keypoint_t), kps2, (size_t)n2 * sizeof(orb_keypoint_t));
    const int32_t hdr[4] = {n1, n2, 0, 1};
    std::memcpy(hp + oC, hdr, 16);
    int32_t* hm = (int32_t*)(hp + oM);
    for (int i = 0; i < cap; ++i) hm[i] = i < n1 ? matches12[i] : -1;
    if (H21) {
        std::memcpy(hp + oH21, H21, hyp);
        std::memcpy(hp + oH12, H12, hyp);
    }
    if (F21) std::memcpy(hp + oF, F21, hyp);
    ORB_HIPCHK(hipMemcpyAsync(C->buf, hp, in_end, hipMemcpyHostToDevice, C->stream));
    uint8_t* d = C->buf;
    InitArgs a{};
    a.kps = (const orb_keypoint_t*)(d + oK);
    a.counts = (const int32_t*)(d + oC);
    a.pair_f1 = a.counts + 2;
    a.pair_f2 = a.counts + 3;
    a.matches12 = (const int32_t*)(d + oM);
    a.M21[0] = H21 ? (const float*)(d + oH21) : nullptr;
    a.H12 = H21 ? (const float*)(d + oH12) : nullptr;
    a.M21[1] = F21 ? (const float*)(d + oF) : nullptr;
    for (int m = 0; m < 2; ++m) {
        a.scores[m] = (float*)(d + oS) + (size_t)m * n_hyp;
        a.best[m] = (int32_t*)(d + oB) + m;
        a.best_score[m] = (float*)(d + oB + 8) + m;
        a.inliers[m] = d + oI + (size_t)m * cap;
    }
    a.n_matches = (int32_t*)(d + oB + 16);
    a.cap = cap;
    a.P = 1;
    a.n_hyp = n_hyp;
    a.inv_sigma2 = 1.0f / (sigma * sigma);  // Initializer.cc:333, 409
    const int r = launch(a, C->stream);
    hipError_t e = hipSuccess;
    if (r == ORB_OK) e = hipMemcpyAsync(hp + oS, d + oS, total - oS, hipMemcpyDeviceToHost, C->stream);
    const hipError_t es = hipStreamSynchronize(C->stream);  // the staging is reused by the next call
    if (r) return r;
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(ORB_EDEVICE, std::string("initializer: ") + hipGetErrorString(e));
    int32_t nm;
    std::memcpy(&nm, hp + oB + 16, 4);
    if (n_matches) *n_matches = nm;
    const float* hs = (const float*)(hp + oS);
    const int32_t* hb = (const int32_t*)(hp + oB);
    const float* hbs = (const float*)(hp + oB + 8);
    if (H21) {
        if (scores_h) std::memcpy(scores_h, hs, (size_t)n_hyp * 4);
        if (best_h) *best_h = hb[0];
        if (best_score_h) *best_score_h = hbs[0];
        if (inliers_h && nm) std::memcpy(inliers_h, hp + oI, (size_t)nm);
    }
    if (F21) {
        if (scores_f) std::memcpy(scores_f, hs + n_hyp, (size_t)n_hyp * 4);
        if (best_f) *best_f = hb[1];
        if (best_score_f) *best_score_f = hbs[1];
        if (inliers_f && nm) std::memcpy(inliers_f, hp + oI + cap, (size_t)nm);
    }
    return ORB_OK;
}

}  // extern "C"
