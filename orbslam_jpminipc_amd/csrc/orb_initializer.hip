// orb_initializer.hip — the two-view model scoring of Initializer on the GPU (part of liborb_hip.so).
//
// Initializer::CheckHomography (reference src/Initializer.cc:303-386) and CheckFundamental
// (388-466) for every RANSAC hypothesis of a frame pair at once, plus the "keep the best" rule of
// FindHomography / FindFundamental (146-169, 197-220).  In orb_initializer_check[_batch_device] the
// hypotheses (ComputeH21 / ComputeF21, cv::SVDecomp) are the caller's; the second part of this file
// generates them on the device and runs the same two kernels behind them, and the third goes on
// from the winning model to ReconstructH / ReconstructF (CheckRT, Triangulate, DecomposeE).
//
// Arithmetic: plain float, the TU is built -ffp-contract=off and the fused multiply-adds that
// g++ -O3 -march=native makes of the reference's expressions are written out
// (scripts/contraction_check_initializer.sh prints the disassembly they are read from):
//   a*x + b*y + c              ->  fmaf(a, x, b*y) + c
//   u - p*winv                 ->  fmaf(-p, winv, u)
//   dx*dx + dy*dy, a*a + b*b   ->  fmaf(dx, dx, dy*dy)
//   1.0/(float)                ->  a float divide (correctly rounded; equal to the double divide
//                                  rounded to float for every float divisor)
// The cv::Mat arithmetic of the second and third part (3 x 3 products, inv(), determinant, norm, scale) is
// csrc/orb_cv_math.h's, Triangulate csrc/orb_jacobi_svd.h's.
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
#include "orb_initializer_scratch.h"
#include "orb_internal.h"
#include "orb_jacobi_svd.h"

namespace {

// cv::Mat arithmetic on 3-vectors and 3 x 3 matrices: csrc/orb_cv_math.h
using orb_cv::det3;
using orb_cv::gemm3;
using orb_cv::inv3;
using orb_cv::M3;
using orb_cv::mul3;
using orb_cv::mul3_alpha;
using orb_cv::neg3x3;
using orb_cv::norm3;
using orb_cv::scale3;

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

// matches12[i] in [-1, n2) for every i < n1 (`w`: the entry point's prefix); *N: how many are matches.
int check_matches(const std::string& w, const int32_t* matches12, int n1, int n2, int* N) {
    *N = 0;
    for (int i = 0; i < n1; ++i) {
        if (matches12[i] < -1 || matches12[i] >= n2)
            return fail(ORB_EINVAL, w + "matches12[" + std::to_string(i) + "] = " + std::to_string(matches12[i]) +
                                        " is outside [-1, n2)");
        *N += matches12[i] >= 0;
    }
    return ORB_OK;
}

// The first inputs of every host form: the pair as a 2-frame batch with one pair (0, 1).
// [kps 2 x cap | counts 2, f1, f2 and what the form adds | matches12 cap, padded with -1]
struct PairStage {
    OrbRegion<orb_keypoint_t> kps;
    OrbRegion<int32_t> hdr, matches;
    size_t cap;
    PairStage(OrbStagePlan& P, int cap_, int n_hdr)
        : kps(P.in<orb_keypoint_t>(2 * (size_t)cap_)), hdr(P.in<int32_t>(n_hdr)), matches(P.in<int32_t>(cap_)), cap(cap_) {}
    // Zeroes the whole in-span first: the kernels read the padding between n1 / n2 and cap.
    void fill(const OrbHostCall& c, const orb_keypoint_t* kps1, int n1, const orb_keypoint_t* kps2, int n2,
              const int32_t* matches12, int use_h = 0) const {
        c.zero_in();
        if (n1) std::memcpy(c.host(kps), kps1, (size_t)n1 * sizeof(orb_keypoint_t));
        if (n2) std::memcpy(c.host(kps) + cap, kps2, (size_t)n2 * sizeof(orb_keypoint_t));
        const int32_t h[5] = {n1, n2, 0, 1, use_h};
        c.put(hdr, h);
        int32_t* hm = c.host(matches);
        for (size_t i = 0; i < cap; ++i) hm[i] = i < (size_t)n1 ? matches12[i] : -1;
    }
};

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
    float* const given[2] = {d_scores_h, d_scores_f};
    void* tmp = nullptr;
    if (int r = orb_scratch_alloc(&tmp, st, "initializer: score scratch: ", [&](OrbLayout& L) {
            for (int m = 0; m < 2; ++m)
                a.scores[m] = given[m] || !a.M21[m] ? given[m] : L.take<float>((size_t)P * n_hyp);
        }))
        return r;
    const int r = launch(a, st);
    if (tmp) (void)hipFreeAsync(tmp, st);
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
    int N;
    if (int r = check_matches("initializer: ", matches12, n1, n2, &N)) return r;
    const size_t nh = (size_t)n_hyp;
    OrbStagePlan P;
    const PairStage pair(P, cap, 4);
    const auto rH21 = P.in<float>(nh * 9), rH12 = P.in<float>(nh * 9), rF = P.in<float>(nh * 9);
    const auto rS = P.out<float>(2 * nh);       // scores_h | scores_f
    const auto rB = P.out<int32_t>(5);          // best 2 | best_score 2 (floats) | n_matches
    const auto rI = P.out<uint8_t>(2 * (size_t)cap);  // inliers_h | inliers_f
    OrbHostCall call(P, device);
    if (call.err) return call.err;
    pair.fill(call, kps1, n1, kps2, n2, matches12);
    InitArgs a{};
    a.kps = call.dev(pair.kps);
    a.counts = call.dev(pair.hdr);
    a.pair_f1 = a.counts + 2;
    a.pair_f2 = a.counts + 3;
    a.matches12 = call.dev(pair.matches);
    a.M21[0] = H21 ? call.send(rH21, H21) : nullptr;
    a.H12 = H21 ? call.send(rH12, H12) : nullptr;
    a.M21[1] = F21 ? call.send(rF, F21) : nullptr;
    for (int m = 0; m < 2; ++m) {
        a.scores[m] = call.dev(rS) + (size_t)m * n_hyp;
        a.best[m] = call.dev(rB) + m;
        a.best_score[m] = (float*)(call.dev(rB) + 2) + m;
        a.inliers[m] = call.dev(rI) + (size_t)m * cap;
    }
    a.n_matches = call.dev(rB) + 4;
    a.cap = cap;
    a.P = 1;
    a.n_hyp = n_hyp;
    a.inv_sigma2 = 1.0f / (sigma * sigma);  // Initializer.cc:333, 409
    if (int r = call.upload()) return r;
    if (int r = call.finish(launch(a, call.stream()), hipSuccess, "initializer: ")) return r;
    const int32_t* hb = call.host(rB);
    const float* hbs = (const float*)(hb + 2);
    const size_t nm = (size_t)hb[4];  // the inliers are n_matches long, not cap
    if (n_matches) *n_matches = hb[4];
    if (H21) {
        call.get(rS, scores_h, nh);
        if (best_h) *best_h = hb[0];
        if (best_score_h) *best_score_h = hbs[0];
        call.get(rI, inliers_h, nm);
    }
    if (F21) {
        call.get(rS, scores_f, nh, nh);
        if (best_f) *best_f = hb[1];
        if (best_score_f) *best_score_f = hbs[1];
        call.get(rI, inliers_f, nm, cap);
    }
    return ORB_OK;
}

}  // extern "C"

// ---- the hypotheses: minimal sets, Normalize, ComputeH21 / ComputeF21 --------------------------
//
// Everything of Initializer::Initialize (Initializer.cc:44-221, 224-301, 747-793) before the two
// checks above, with the OpenCV 2.4 routines it calls restated as read (the CPU
// statement of the same reading is tests/native/initializer_ransac_model.cpp, which shares no text
// with this file).  Plain IEEE f32 / f64 operations only, no contraction, no libm call.
//
//   k_init_normalize   one workgroup per (pair, frame side).  Side 0 first lists the pair's matches
//                      in index order (the keypoint index of every match ordinal, and N).  Wave 0
//                      then runs Normalize's four float sums as the reference's chains: 64
//                      keypoints per step loaded one per lane, every lane adding all 64 in order
//                      (so the sum is uniform), and writes T, the means and the scales.  The
//                      normalised points themselves are recomputed by the lanes that gather them:
//                      (x - mean) * s is the same two operations.
//   k_init_hypotheses  one lane per (pair, model, hypothesis), workgroups of one wave.  The lane's
//                      work matrices live in LDS laid out [element][lane] (conflict free, any
//                      runtime index): the 9 x 16 At and 9 x 9 Vt of ComputeH21's decomposition,
//                      or the 9 x 9 of ComputeF21's with its 3 x 3 behind it, the doubles W, and
//                      the 8 moved entries of the index list.  Every dot product and sum of
//                      squares is one double accumulator with k ascending.
//   k_init_result      one thread per pair: the winning H21 / F21 (NaN without a winner), RH and
//                      which model Initialize would reconstruct from.
namespace {

constexpr int HY_A = 144;                                   // floats of the At region (9 x 16)
constexpr int HY_V = 81;                                    // floats of the Vt region (9 x 9)
constexpr int HY_LDS = (HY_A + HY_V) * 64 * 4 + 9 * 64 * 8;  // + W: 62208 bytes
constexpr int NORM_THREADS = 256;

struct HypArgs {
    const orb_keypoint_t* kps;
    const int32_t* counts;
    const int32_t* pair_f1;
    const int32_t* pair_f2;
    const int32_t* matches12;
    const int32_t* rand31;   // P x n_hyp x 8, or NULL when sets_in is given
    const int32_t* sets_in;  // P x n_hyp x 8 match ordinals, each in [0, N)
    int32_t* ord_i;          // P x cap: keypoint index in frame 1 of every match ordinal
    int32_t* nmatch;         // P
    float* norm;             // P x 2 x HY_NORM
    float* H21;              // P x n_hyp x 9 each; any may be NULL
    float* H12;
    float* F21;
    float* Hn;
    float* Fn;
    int32_t* sets_out;       // P x n_hyp x 8
    int cap, P, n_hyp;
};

__global__ void __launch_bounds__(NORM_THREADS) k_init_normalize(HypArgs a) {
    __shared__ int s_wtot[NORM_THREADS / 64];
    const int p = blockIdx.x, side = blockIdx.y, tid = threadIdx.x;
    InitArgs ia{};
    ia.kps = a.kps;
    ia.counts = a.counts;
    ia.pair_f1 = a.pair_f1;
    ia.pair_f2 = a.pair_f2;
    ia.matches12 = a.matches12;
    ia.cap = a.cap;
    const PairView v = pair_view(ia, p);
    if (side == 0) {
        int32_t* ord = a.ord_i + (size_t)p * a.cap;
        const int N = compact_matches<NORM_THREADS>(v, s_wtot, [&](int o, int i, int) { ord[o] = i; });
        if (tid == 0) a.nmatch[p] = N;
    }
    if (tid >= 64) return;
    // Normalize (Initializer.cc:747-793) over all n keypoints of the frame, matched or not
    const orb_keypoint_t* k = side ? v.k2 : v.k1;
    const int n = side ? v.n2 : v.n1;
    float meanX = 0, meanY = 0;
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + tid;
        const float x = i < n ? k[i].x : 0.0f, y = i < n ? k[i].y : 0.0f;
        const int cnt = min(64, n - i0);
        if (cnt == 64) {
#pragma unroll
            for (int j = 0; j < 64; ++j) {
                meanX += __shfl(x, j);
                meanY += __shfl(y, j);
            }
        } else {
            for (int j = 0; j < cnt; ++j) {
                meanX += __shfl(x, j);
                meanY += __shfl(y, j);
            }
        }
    }
    meanX = meanX / (float)n;
    meanY = meanY / (float)n;
    float meanDevX = 0, meanDevY = 0;
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + tid;
        const float x = i < n ? fabsf(k[i].x - meanX) : 0.0f, y = i < n ? fabsf(k[i].y - meanY) : 0.0f;
        const int cnt = min(64, n - i0);
        if (cnt == 64) {
#pragma unroll
            for (int j = 0; j < 64; ++j) {
                meanDevX += __shfl(x, j);
                meanDevY += __shfl(y, j);
            }
        } else {
            for (int j = 0; j < cnt; ++j) {
                meanDevX += __shfl(x, j);
                meanDevY += __shfl(y, j);
            }
        }
    }
    meanDevX = meanDevX / (float)n;
    meanDevY = meanDevY / (float)n;
    const float sX = 1.0f / meanDevX, sY = 1.0f / meanDevY;  // 1.0/(float) narrowed: the float quotient (§11)
    if (tid == 0) {
        float* T = a.norm + ((size_t)p * 2 + side) * HY_NORM;
        T[0] = sX;
        T[1] = 0.0f;
        T[2] = -meanX * sX;
        T[3] = 0.0f;
        T[4] = sY;
        T[5] = -meanY * sY;
        T[6] = 0.0f;
        T[7] = 0.0f;
        T[8] = 1.0f;
        T[9] = meanX;
        T[10] = meanY;
        T[11] = sX;
        T[12] = sY;
    }
}

__device__ __forceinline__ void hy_store9(float* dst, long long g, const M3& v) {
    if (!dst) return;
#pragma unroll
    for (int k = 0; k < 9; ++k) dst[g * 9 + k] = v.m[k];
}

__global__ void __launch_bounds__(64) k_init_hypotheses(HypArgs a, int tiles) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int model = blockIdx.y;
    const int p = blockIdx.x / tiles, tile = blockIdx.x - p * tiles;
    const int lane = threadIdx.x;
    const int h = tile * 64 + lane;
    if (h >= a.n_hyp) return;  // (no barrier below: every lane works on its own column)
    if (model == 0 ? (!a.H21 && !a.H12 && !a.Hn && !a.sets_out) : (!a.F21 && !a.Fn)) return;
    float* A = (float*)smem + lane;
    float* V = (float*)smem + HY_A * 64 + lane;
    double* W = (double*)(smem + (HY_A + HY_V) * 64 * 4) + lane;
    const long long g = (long long)p * a.n_hyp + h;
    const int N = a.nmatch[p];
    if (N < 8) {  // the reference would pop from an empty vector: nothing is generated
        M3 z;
#pragma unroll
        for (int k = 0; k < 9; ++k) z.m[k] = 0.0f;
        if (model == 0) {
            hy_store9(a.H21, g, z);
            hy_store9(a.H12, g, z);
            hy_store9(a.Hn, g, z);
            if (a.sets_out)
                for (int j = 0; j < 8; ++j) a.sets_out[g * 8 + j] = 0;
        } else {
            hy_store9(a.F21, g, z);
            hy_store9(a.Fn, g, z);
        }
        return;
    }
    // The minimal set (Initializer.cc:80-95).  vAvailableIndices is the identity except where a
    // removal wrote back() into the drawn position: at most 7 entries matter, kept as (position,
    // value) in the W region, a later write to a position hiding an earlier one.
    int* pos = (int*)W;          // [j * 128], [j * 128 + 1]: the two ints of the lane's double j
    int* val = (int*)W + 1;
    int* set = (int*)V;          // [j * 64]
#pragma unroll 1
    for (int j = 0; j < 8; ++j) {
        int idx;
        if (a.sets_in)
            idx = a.sets_in[g * 8 + j];
        else {
            const int size = N - j;
            const int r = max(a.rand31[g * 8 + j], 0);
            const int randi = (int)(((long long)r * size) >> 31);  // RandomInt(0, size - 1), §15
            idx = randi;
            int back = size - 1;
            for (int t = 0; t < j; ++t) {
                if (pos[t * 128] == randi) idx = val[t * 128];
                if (pos[t * 128] == size - 1) back = val[t * 128];
            }
            pos[j * 128] = randi;
            val[j * 128] = back;
        }
        set[j * 64] = idx;
        if (model == 0 && a.sets_out) a.sets_out[g * 8 + j] = idx;
    }
    InitArgs ia{};
    ia.kps = a.kps;
    ia.counts = a.counts;
    ia.pair_f1 = a.pair_f1;
    ia.pair_f2 = a.pair_f2;
    ia.matches12 = a.matches12;
    ia.cap = a.cap;
    const PairView v = pair_view(ia, p);
    const int32_t* ord = a.ord_i + (size_t)p * a.cap;
    const float* n1 = a.norm + (size_t)p * 2 * HY_NORM;
    const float* n2 = n1 + HY_NORM;
    M3 T1, T2;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        T1.m[k] = n1[k];
        T2.m[k] = n2[k];
    }
    const float m1x = n1[9], m1y = n1[10], s1x = n1[11], s1y = n1[12];
    const float m2x = n2[9], m2y = n2[10], s2x = n2[11], s2y = n2[12];
    // gather: vPn1[mvMatches12[idx].first], vPn2[mvMatches12[idx].second], and the rows of A
    int sidx[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) sidx[j] = set[j * 64];  // (V is written below)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int i = ord[sidx[j]];
        const int m = v.m12[i];
        const float u1 = (v.k1[i].x - m1x) * s1x, v1 = (v.k1[i].y - m1y) * s1y;
        const float u2 = (v.k2[m].x - m2x) * s2x, v2 = (v.k2[m].y - m2y) * s2y;
        if (model == 0) {
            // ComputeH21: A is 16 x 9, rows < cols is false, so At = A^T, 9 rows of 16
            const float r0[9] = {0.0f, 0.0f, 0.0f, -u1, -v1, -1.0f, v2 * u1, v2 * v1, v2};
            const float r1[9] = {u1, v1, 1.0f, 0.0f, 0.0f, 0.0f, -u2 * u1, -u2 * v1, -u2};
#pragma unroll
            for (int c = 0; c < 9; ++c) {
                A[(c * 16 + 2 * j) * 64] = r0[c];
                A[(c * 16 + 2 * j + 1) * 64] = r1[c];
            }
        } else {
            // ComputeF21: A is 8 x 9 and is worked on as it is; row 8 of the 9 x 9 starts as zeros
            const float r[9] = {u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, 1.0f};
#pragma unroll
            for (int c = 0; c < 9; ++c) A[(j * 9 + c) * 64] = r[c];
        }
    }
    if (model == 0) {
        hy_jacobi<16, 9, 0, true>(A, V, W);
        M3 Hn;
#pragma unroll
        for (int k = 0; k < 9; ++k) Hn.m[k] = V[(8 * 9 + k) * 64];  // vt.row(8)
        const M3 H21 = mul3(mul3(inv3(T2), Hn), T1);       // T2inv*Hn*T1
        hy_store9(a.Hn, g, Hn);
        hy_store9(a.H21, g, H21);
        hy_store9(a.H12, g, inv3(H21));
    } else {
#pragma unroll
        for (int c = 0; c < 9; ++c) A[(8 * 9 + c) * 64] = 0.0f;
        hy_jacobi<9, 8, 9, false>(A, nullptr, W);
        // Fpre = vt.row(8), the filled-in row; its decomposition takes the transpose path
        float* A3 = V;
        float* V3 = V + 9 * 64;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int k = 0; k < 3; ++k) A3[(i * 3 + k) * 64] = A[(8 * 9 + k * 3 + i) * 64];
        hy_jacobi<3, 3, 3, true>(A3, V3, W);
        M3 u, vt, D;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                u.m[r * 3 + c] = A3[(c * 3 + r) * 64];
                vt.m[r * 3 + c] = V3[(r * 3 + c) * 64];
                D.m[r * 3 + c] = 0.0f;
            }
        D.m[0] = (float)W[0];
        D.m[4] = (float)W[64];  // w[2] = 0
        const M3 Fn = mul3(mul3(u, D), vt);
        M3 T2t;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) T2t.m[r * 3 + c] = T2.m[c * 3 + r];
        hy_store9(a.Fn, g, Fn);
        hy_store9(a.F21, g, mul3(mul3(T2t, Fn), T1));  // T2t*Fn*T1
    }
}

struct ResultArgs {
    const float* H21;
    const float* F21;
    const int32_t* best[2];
    const float* best_score[2];
    float* best_H21;
    float* best_F21;
    float* RH;
    int32_t* use_h;
    int P, n_hyp;
};

__global__ void __launch_bounds__(64) k_init_result(ResultArgs a) {
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= a.P) return;
    const float nan = __builtin_nanf("");
    const int bh = a.best[0][p], bf = a.best[1][p];
    if (a.best_H21)
        for (int k = 0; k < 9; ++k) a.best_H21[(size_t)p * 9 + k] = bh >= 0 ? a.H21[((size_t)p * a.n_hyp + bh) * 9 + k] : nan;
    if (a.best_F21)
        for (int k = 0; k < 9; ++k) a.best_F21[(size_t)p * 9 + k] = bf >= 0 ? a.F21[((size_t)p * a.n_hyp + bf) * 9 + k] : nan;
    const float SH = a.best_score[0][p], SF = a.best_score[1][p];
    const float RH = SH / (SH + SF);  // Initializer.cc:110
    if (a.RH) a.RH[p] = RH;
    if (a.use_h) a.use_h[p] = (double)RH > 0.40 ? 1 : 0;  // Initializer.cc:113: a float against the double 0.40
}

// normalise -> hypotheses -> (when `score`) k_init_scores, k_init_best, k_init_result, enqueued on
// `st`.  `scratch`: `scratch_bytes` of device memory for chain_regions(), or NULL for a stream-ordered
// allocation freed after the last kernel.
int run_chain(const orb_keypoint_t* d_kps, const int32_t* d_counts, int cap, int P, const int32_t* d_pair_f1,
              const int32_t* d_pair_f2, const int32_t* d_matches12, float sigma, int n_hyp, const int32_t* d_rand31,
              const int32_t* d_sets, bool score, const ChainOut& o, uint8_t* scratch, size_t scratch_bytes,
              hipStream_t st) {
    HypArgs h{};
    InitArgs a{};
    void* owned = nullptr;
    if (scratch) {
        OrbLayout L(scratch);
        chain_regions(L, o, score, cap, P, n_hyp, h, a);
        assert(L.end <= scratch_bytes);
    } else if (int r = orb_scratch_alloc(&owned, st, "initializer: scratch: ", [&](OrbLayout& L) {
                   chain_regions(L, o, score, cap, P, n_hyp, h, a);
               }))
        return r;
    h.kps = d_kps;
    h.counts = d_counts;
    h.pair_f1 = d_pair_f1;
    h.pair_f2 = d_pair_f2;
    h.matches12 = d_matches12;
    h.rand31 = d_rand31;
    h.sets_in = d_sets;
    h.Hn = o.Hn;
    h.Fn = o.Fn;
    h.sets_out = o.sets_out;
    h.cap = cap;
    h.P = P;
    h.n_hyp = n_hyp;
    int r = ORB_OK;
    hipError_t e = hipSuccess;
    const int tiles = (n_hyp + 63) / 64;
    hipLaunchKernelGGL(k_init_normalize, dim3(P, 2), dim3(NORM_THREADS), 0, st, h);
    if ((e = hipGetLastError()) == hipSuccess)
        e = hipFuncSetAttribute((const void*)k_init_hypotheses, hipFuncAttributeMaxDynamicSharedMemorySize, HY_LDS);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_init_hypotheses, dim3((unsigned)((size_t)P * tiles), 2), dim3(64), HY_LDS, st, h, tiles);
        e = hipGetLastError();
    }
    if (e == hipSuccess && score) {
        a.kps = d_kps;
        a.counts = d_counts;
        a.pair_f1 = d_pair_f1;
        a.pair_f2 = d_pair_f2;
        a.matches12 = d_matches12;
        a.M21[0] = h.H21;
        a.M21[1] = h.F21;
        a.H12 = h.H12;
        a.inliers[0] = o.inliers_h;
        a.inliers[1] = o.inliers_f;
        a.n_matches = o.n_matches;
        a.cap = cap;
        a.P = P;
        a.n_hyp = n_hyp;
        a.inv_sigma2 = 1.0f / (sigma * sigma);  // Initializer.cc:333, 409
        r = launch(a, st);
        if (r == ORB_OK && (o.best_H21 || o.best_F21 || o.RH || o.use_h)) {
            ResultArgs ra{h.H21, h.F21, {a.best[0], a.best[1]}, {a.best_score[0], a.best_score[1]},
                          o.best_H21, o.best_F21, o.RH, o.use_h, P, n_hyp};
            hipLaunchKernelGGL(k_init_result, dim3((P + 63) / 64), dim3(64), 0, st, ra);
            e = hipGetLastError();
        }
    }
    if (owned) (void)hipFreeAsync(owned, st);
    if (r) return r;
    if (e != hipSuccess) return fail(ORB_EDEVICE, std::string("initializer: ") + hipGetErrorString(e));
    return ORB_OK;
}

// The host forms: the pair as a 2-frame batch with one pair (0, 1), staged like orb_initializer_check.
// Their outputs are the chain's, as host arrays, with the two halves of `norm` apart.
struct HostOut : ChainOut {
    float *T1, *T2;
};

int host_run(const char* who, const orb_keypoint_t* kps1, int n1, const orb_keypoint_t* kps2, int n2,
             const int32_t* matches12, float sigma, int n_hyp, const int32_t* sets, const int32_t* rand31, bool score,
             const HostOut& o, int device) {
    const std::string w = std::string(who) + ": ";
    if (n1 < 0 || n2 < 0 || (n1 && (!kps1 || !matches12)) || (n2 && !kps2)) return fail(ORB_EINVAL, w + "bad arguments");
    if ((sets == nullptr) == (rand31 == nullptr)) return fail(ORB_EINVAL, w + "exactly one of sets and rand31 is given");
    const int cap = std::max(std::max(n1, n2), 1);
    if (cap > IN_MAX_CAP) return fail(ORB_ENOTSUP, w + "more than 8192 keypoints per frame");
    if (n_hyp < 1 || n_hyp > IN_MAX_HYP)
        return fail(ORB_EINVAL, w + "n_hyp must be in [1, 1024] (got " + std::to_string(n_hyp) + ")");
    int N;
    if (int r = check_matches(w, matches12, n1, n2, &N)) return r;
    for (int k = 0; k < n_hyp * 8; ++k) {
        if (rand31 && rand31[k] < 0)
            return fail(ORB_EINVAL, w + "rand31[" + std::to_string(k) + "] = " + std::to_string(rand31[k]) + " is negative");
        if (sets && N >= 8 && (sets[k] < 0 || sets[k] >= N))
            return fail(ORB_EINVAL, w + "sets[" + std::to_string(k) + "] = " + std::to_string(sets[k]) +
                                        " is outside [0, N = " + std::to_string(N) + ")");
    }
    const size_t nh = (size_t)n_hyp;
    OrbStagePlan P;
    const PairStage pair(P, cap, 4);
    const auto rD = P.in<int32_t>(nh * 8);
    OrbRegion<float> rHyp[5];  // H21 H12 F21 Hn Fn
    for (auto& r : rHyp) r = P.out<float>(nh * 9);
    const auto rSet = P.out<int32_t>(nh * 8);
    const auto rN = P.out<float>(2 * HY_NORM);  // T1 ..., T2 ...
    const auto rS = P.out<float>(2 * nh);       // scores_h | scores_f
    const auto rB = P.out<int32_t>(7);          // best 2 | best_score 2 (floats) | n_matches | RH (float) | use_h
    const auto rBH = P.out<float>(18);          // best_H21 | best_F21
    const auto rI = P.out<uint8_t>(2 * (size_t)cap);  // inliers_h | inliers_f
    HypArgs h0{};  // the chain's scratch at its most, as if no optional output were given
    InitArgs a0{};
    const auto rX = P.scratch<uint8_t>(
        orb_layout_size([&](OrbLayout& L) { chain_regions(L, ChainOut{}, score, cap, 1, n_hyp, h0, a0); }));
    OrbHostCall call(P, device);
    if (call.err) return call.err;
    pair.fill(call, kps1, n1, kps2, n2, matches12);
    const int32_t *dc = call.dev(pair.hdr), *dd = call.send(rD, sets ? sets : rand31);
    if (int r = call.upload()) return r;
    ChainOut co{};
    co.H21 = call.dev(rHyp[0]);
    co.H12 = call.dev(rHyp[1]);
    co.F21 = call.dev(rHyp[2]);
    co.Hn = call.dev(rHyp[3]);
    co.Fn = call.dev(rHyp[4]);
    co.sets_out = call.dev(rSet);
    co.norm = call.dev(rN);
    int32_t* const db = call.dev(rB);
    co.n_matches = db + 4;
    if (score) {
        co.scores_h = call.dev(rS);
        co.scores_f = co.scores_h + n_hyp;
        co.best_h = db;
        co.best_f = db + 1;
        co.best_score_h = (float*)(db + 2);
        co.best_score_f = co.best_score_h + 1;
        co.RH = (float*)(db + 5);
        co.use_h = db + 6;
        co.best_H21 = call.dev(rBH);
        co.best_F21 = co.best_H21 + 9;
        co.inliers_h = call.dev(rI);
        co.inliers_f = co.inliers_h + cap;
    }
    const int r = run_chain(call.dev(pair.kps), dc, cap, 1, dc + 2, dc + 3, call.dev(pair.matches), sigma, n_hyp,
                            rand31 ? dd : nullptr, sets ? dd : nullptr, score, co, call.dev(rX), rX.count, call.stream());
    if (int rf = call.finish(r, hipSuccess, w)) return rf;
    float* const ho[5] = {o.H21, o.H12, o.F21, o.Hn, o.Fn};
    for (int k = 0; k < 5; ++k) call.get(rHyp[k], ho[k]);
    call.get(rSet, o.sets_out);
    call.get(rN, o.T1, 9);
    call.get(rN, o.T2, 9, HY_NORM);
    const int32_t* hb = call.host(rB);
    const float* hbs = (const float*)(hb + 2);
    const size_t nm = (size_t)hb[4];  // the inliers are n_matches long, not cap
    if (o.n_matches) *o.n_matches = hb[4];
    if (!score) return ORB_OK;
    call.get(rS, o.scores_h, nh);
    call.get(rS, o.scores_f, nh, nh);
    if (o.best_h) *o.best_h = hb[0];
    if (o.best_f) *o.best_f = hb[1];
    if (o.best_score_h) *o.best_score_h = hbs[0];
    if (o.best_score_f) *o.best_score_f = hbs[1];
    call.get(rI, o.inliers_h, nm);
    call.get(rI, o.inliers_f, nm, cap);
    if (o.RH) std::memcpy(o.RH, hb + 5, 4);
    if (o.use_h) *o.use_h = hb[6];
    call.get(rBH, o.best_H21, 9);
    call.get(rBH, o.best_F21, 9, 9);
    return ORB_OK;
}

}  // namespace

extern "C" {

int orb_initializer_compute_hypotheses(const orb_keypoint_t* kps1, int n1, const orb_keypoint_t* kps2, int n2,
                                       const int32_t* matches12, int n_hyp, const int32_t* sets, const int32_t* rand31,
                                       float* H21, float* H12, float* F21, float* Hn, float* Fn, float* T1, float* T2,
                                       int32_t* sets_out, int* n_matches, int device) {
    HostOut o{};
    o.H21 = H21;
    o.H12 = H12;
    o.F21 = F21;
    o.Hn = Hn;
    o.Fn = Fn;
    o.T1 = T1;
    o.T2 = T2;
    o.sets_out = sets_out;
    o.n_matches = n_matches;
    return host_run("initializer hypotheses", kps1, n1, kps2, n2, matches12, 1.0f, n_hyp, sets, rand31, false, o, device);
}

int orb_initializer_ransac(const orb_keypoint_t* kps1, int n1, const orb_keypoint_t* kps2, int n2,
                           const int32_t* matches12, float sigma, int n_hyp, const int32_t* rand31, float* H21,
                           float* H12, float* F21, int32_t* sets_out, float* scores_h, float* scores_f, int32_t* best_h,
                           float* best_score_h, uint8_t* inliers_h, int32_t* best_f, float* best_score_f,
                           uint8_t* inliers_f, float* best_H21, float* best_F21, float* RH, int32_t* use_h,
                           int* n_matches, int device) {
    HostOut o{};
    o.H21 = H21;
    o.H12 = H12;
    o.F21 = F21;
    o.sets_out = sets_out;
    o.scores_h = scores_h;
    o.scores_f = scores_f;
    o.best_h = best_h;
    o.best_score_h = best_score_h;
    o.inliers_h = inliers_h;
    o.best_f = best_f;
    o.best_score_f = best_score_f;
    o.inliers_f = inliers_f;
    o.best_H21 = best_H21;
    o.best_F21 = best_F21;
    o.RH = RH;
    o.use_h = use_h;
    o.n_matches = n_matches;
    if (!rand31) return fail(ORB_EINVAL, "initializer ransac: rand31 is NULL");
    return host_run("initializer ransac", kps1, n1, kps2, n2, matches12, sigma, n_hyp, nullptr, rand31, true, o, device);
}

int orb_initializer_ransac_batch_device(const orb_keypoint_t* d_kps, const int32_t* d_counts, int cap, int P,
                                        const int32_t* d_pair_f1, const int32_t* d_pair_f2,
                                        const int32_t* d_matches12, float sigma, int n_hyp, const int32_t* d_rand31,
                                        float* d_H21, float* d_H12, float* d_F21, int32_t* d_sets_out,
                                        float* d_scores_h, float* d_scores_f, int32_t* d_best_h, float* d_best_score_h,
                                        uint8_t* d_inliers_h, int32_t* d_best_f, float* d_best_score_f,
                                        uint8_t* d_inliers_f, int32_t* d_n_matches, float* d_best_H21,
                                        float* d_best_F21, float* d_RH, int32_t* d_use_h, void* stream) {
    if (P < 0 || cap <= 0) return fail(ORB_EINVAL, "initializer ransac: bad arguments");
    if (int r = check_limits(cap, n_hyp, true, true)) return r;
    if (P == 0) return ORB_OK;
    if (P > 65535) return fail(ORB_ENOTSUP, "initializer ransac: more than 65535 pairs per call");
    if (!d_kps || !d_counts || !d_pair_f1 || !d_pair_f2 || !d_matches12 || !d_rand31)
        return fail(ORB_EINVAL, "initializer ransac: bad arguments");
    ChainOut o{};
    o.H21 = d_H21;
    o.H12 = d_H12;
    o.F21 = d_F21;
    o.sets_out = d_sets_out;
    o.scores_h = d_scores_h;
    o.scores_f = d_scores_f;
    o.best_h = d_best_h;
    o.best_score_h = d_best_score_h;
    o.inliers_h = d_inliers_h;
    o.best_f = d_best_f;
    o.best_score_f = d_best_score_f;
    o.inliers_f = d_inliers_f;
    o.n_matches = d_n_matches;
    o.best_H21 = d_best_H21;
    o.best_F21 = d_best_F21;
    o.RH = d_RH;
    o.use_h = d_use_h;
    return run_chain(d_kps, d_counts, cap, P, d_pair_f1, d_pair_f2, d_matches12, sigma, n_hyp, d_rand31, nullptr, true, o,
                     nullptr, 0, (hipStream_t)stream);
}

}  // extern "C"

// ---- the reconstruction: ReconstructF / ReconstructH, CheckRT, Triangulate, DecomposeE ----------
//
// What Initializer::Initialize does with the winning model (Initializer.cc:113-116, 468-745,
// 796-927); the CPU statement of the same reading is
// tests/native/initializer_reconstruct_model.cpp, which shares no text with this file.  IEEE f32 /
// f64 operations, the reference build's five fused multiply-adds written out, one libm call (acosf).
//
//   k_init_motion   one workgroup per pair: the matches in index order (frame-1 index of every
//                   ordinal, N), the count of set mask entries, and on thread 0 the 4 (DecomposeE) or
//                   8 (Faugeras) motion hypotheses of the model that use_h names.
//   k_init_checkrt  one lane per (pair, hypothesis, match ordinal), workgroups of one wave:
//                   Triangulate's 4 x 4 decomposition on the lane's column of LDS ([element][lane],
//                   hy_jacobi of §16 on the transposed matrix, only vt.row(3) read) and every gate of
//                   CheckRT; writes the counted / vbGood flags and the cosine.
//   k_init_stat     one workgroup per (pair, hypothesis): nGood and sorted[min(50, nGood - 1)] of
//                   the counted cosines by rank counting in LDS (a NaN ranks after every number),
//                   then the parallax.
//   k_init_select   one workgroup per pair: the acceptance rule on thread 0, then R21, t21 and the
//                   winner's vP3D / vbTriangulated rows, its points recomputed with the same function.
namespace {

constexpr int RC_THREADS = 256;
constexpr double RC_PI = 3.1415926535897932384626433832795;  // CV_PI

struct RecArgs {
    const orb_keypoint_t* kps;
    const int32_t* counts;
    const int32_t* pair_f1;
    const int32_t* pair_f2;
    const int32_t* matches12;
    const float* H21;          // P x 9 each: the winners
    const float* F21;
    const int32_t* use_h;      // P
    const uint8_t* inl_h;      // P x cap, by match ordinal
    const uint8_t* inl_f;
    const int32_t* n_matches;  // P, or NULL: every match is walked
    float fx, fy, cx, cy, th2, min_parallax;
    int min_triangulated;
    int32_t* ord_i;            // P x cap (scratch)
    int32_t* nwalk;            // P (scratch)
    uint8_t* flags;            // P x 8 x cap (scratch): bit 0 counted, bit 1 vbGood
    float* cosv;               // P x 8 x cap (scratch)
    int32_t* n_motion;         // P; none of the following is NULL in the kernels
    float* motion_R;           // P x 72
    float* motion_t;           // P x 24
    int32_t* n_good;           // P x 8
    float* cos_sel;            // P x 8
    float* parallax;           // P x 8
    int32_t* n_inliers;        // P
    int32_t* best;             // P
    int32_t* ok;               // P; this and the following may be NULL
    float* R21;                // P x 9
    float* t21;                // P x 3
    float* P3D;                // P x cap x 3
    uint8_t* triangulated;     // P x cap
    int cap, P;
};

__device__ __forceinline__ PairView rec_view(const RecArgs& a, int p) {
    InitArgs ia{};
    ia.kps = a.kps;
    ia.counts = a.counts;
    ia.pair_f1 = a.pair_f1;
    ia.pair_f2 = a.pair_f2;
    ia.matches12 = a.matches12;
    ia.cap = a.cap;
    return pair_view(ia, p);
}

// U * tp (3 x 3 by 3 x 1, the short path), then t / cv::norm(t)
__device__ __forceinline__ void rc_unit_Ut(const M3& U, const float* tp, float* out) {
    float t[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) t[r] = U.m[3 * r] * tp[0] + U.m[3 * r + 1] * tp[1] + U.m[3 * r + 2] * tp[2];
    scale3(t, 1. / norm3(t), out);
}

// SVD::compute of a 3 x 3 on column 0 of the given LDS regions (the transpose path of §16)
__device__ void rc_svd3(const M3& S, float* A3, float* Vq, double* W, M3* u, M3* vt, float* w) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) A3[(i * 3 + k) * 64] = S.m[k * 3 + i];
    hy_jacobi<3, 3, 3, true>(A3, Vq, W);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            u->m[r * 3 + c] = A3[(c * 3 + r) * 64];
            vt->m[r * 3 + c] = Vq[(r * 3 + c) * 64];
        }
#pragma unroll
    for (int i = 0; i < 3; ++i) w[i] = (float)W[i * 64];
}

__device__ __forceinline__ void rc_store_motion(const RecArgs& a, int p, int k, const M3& R, const float* t) {
#pragma unroll
    for (int e = 0; e < 9; ++e) a.motion_R[(size_t)p * 72 + k * 9 + e] = R.m[e];
#pragma unroll
    for (int e = 0; e < 3; ++e) a.motion_t[(size_t)p * 24 + k * 3 + e] = t[e];
}

__global__ void __launch_bounds__(RC_THREADS) k_init_motion(RecArgs a) {
    __shared__ int s_wtot[RC_THREADS / 64];
    __shared__ int s_cnt;
    __shared__ float s_a[9 * 64], s_v[9 * 64];
    __shared__ double s_w[3 * 64];
    const int p = blockIdx.x, tid = threadIdx.x;
    const PairView v = rec_view(a, p);
    const bool use_h = a.use_h[p] != 0;
    if (tid == 0) s_cnt = 0;
    int32_t* ord = a.ord_i + (size_t)p * a.cap;
    const int N = compact_matches<RC_THREADS>(v, s_wtot, [&](int o, int i, int) { ord[o] = i; });
    const int Nw = a.n_matches ? min(N, max(a.n_matches[p], 0)) : N;
    const uint8_t* mask = (use_h ? a.inl_h : a.inl_f) + (size_t)p * a.cap;
    int c = 0;
    for (int o = tid; o < Nw; o += RC_THREADS) c += mask[o] != 0;
    if (c) atomicAdd(&s_cnt, c);
    __syncthreads();
    if (tid != 0) return;
    a.nwalk[p] = Nw;
    a.n_inliers[p] = s_cnt;
    for (int e = 0; e < 72; ++e) a.motion_R[(size_t)p * 72 + e] = 0.0f;
    for (int e = 0; e < 24; ++e) a.motion_t[(size_t)p * 24 + e] = 0.0f;
    M3 K, M;
    {
        const float k[9] = {a.fx, 0.0f, a.cx, 0.0f, a.fy, a.cy, 0.0f, 0.0f, 1.0f};
        const float* src = (use_h ? a.H21 : a.F21) + (size_t)p * 9;
#pragma unroll
        for (int e = 0; e < 9; ++e) {
            K.m[e] = k[e];
            M.m[e] = src[e];
        }
    }
    M3 U, Vt;
    float w[3];
    if (!use_h) {
        // ReconstructF: E21 = K.t()*F21*K (the first product carries GEMM_1_T), DecomposeE
        const M3 E = mul3(gemm3<true, false>(K, M, 1.0), K);
        rc_svd3(E, s_a, s_v, s_w, &U, &Vt, w);
        const float col[3] = {U.m[2], U.m[5], U.m[8]};
        float t1[3], t2[3];
        scale3(col, 1. / norm3(col), t1);  // t = t/cv::norm(t)
        M3 W;
        {
            const float wm[9] = {0.0f, -1.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f};
#pragma unroll
            for (int e = 0; e < 9; ++e) W.m[e] = wm[e];
        }
        M3 R1 = mul3(mul3(U, W), Vt);
        if (det3(R1) < 0) R1 = neg3x3(R1);
        M3 R2 = mul3(gemm3<false, true>(U, W, 1.0), Vt);  // u*W.t()*vt: GEMM_2_T
        if (det3(R2) < 0) R2 = neg3x3(R2);
#pragma unroll
        for (int e = 0; e < 3; ++e) t2[e] = 0.0f - t1[e];
        rc_store_motion(a, p, 0, R1, t1);
        rc_store_motion(a, p, 1, R2, t1);
        rc_store_motion(a, p, 2, R1, t2);
        rc_store_motion(a, p, 3, R2, t2);
        a.n_motion[p] = 4;
        return;
    }
    // ReconstructH (Faugeras); vn is computed by the reference and never read: skipped
    const M3 A = mul3(mul3(inv3(K), M), K);
    rc_svd3(A, s_a, s_v, s_w, &U, &Vt, w);
    const float s = (float)(det3(U) * det3(Vt));
    const float d1 = w[0], d2 = w[1], d3 = w[2];
    if ((double)(d1 / d2) < 1.00001 || (double)(d2 / d3) < 1.00001) {
        a.n_motion[p] = 0;
        return;
    }
    const float d22 = d2 * d2, d33 = d3 * d3, d13 = d1 * d3;
    const float n12 = __builtin_fmaf(d1, d1, -d22), n13 = __builtin_fmaf(d1, d1, -d33), n23 = d22 - d33;
    const float aux1 = __builtin_sqrtf(n12 / n13);
    const float aux3 = __builtin_sqrtf(n23 / n13);
    const float root = __builtin_sqrtf(n12 * n23);
    const float aux_stheta = root / ((d1 + d3) * d2);
    const float ctheta = (d22 + d13) / ((d1 + d3) * d2);
    const float aux_sphi = root / ((d1 - d3) * d2);
    const float cphi = (d13 - d22) / ((d1 - d3) * d2);
#pragma unroll 1
    for (int i = 0; i < 4; ++i) {
        const float x1 = i < 2 ? aux1 : -aux1;
        const float x3 = (i & 1) ? -aux3 : aux3;
        const float st = (i == 0 || i == 3) ? aux_stheta : -aux_stheta;
        const float sp = (i == 0 || i == 3) ? aux_sphi : -aux_sphi;
        M3 Rp;
        float tp[3], t[3];
        {
            const float r[9] = {ctheta, 0.0f, -st, 0.0f, 1.0f, 0.0f, st, 0.0f, ctheta};
#pragma unroll
            for (int e = 0; e < 9; ++e) Rp.m[e] = r[e];
        }
        tp[0] = x1, tp[1] = 0.0f, tp[2] = -x3;
        scale3(tp, (double)(d1 - d3), tp);  // tp *= d1-d3
        rc_unit_Ut(U, tp, t);
        rc_store_motion(a, p, i, mul3(mul3_alpha(U, Rp, (double)s), Vt), t);  // s*U*Rp*Vt
        {
            const float r[9] = {cphi, 0.0f, sp, 0.0f, -1.0f, 0.0f, sp, 0.0f, -cphi};
#pragma unroll
            for (int e = 0; e < 9; ++e) Rp.m[e] = r[e];
        }
        tp[0] = x1, tp[1] = 0.0f, tp[2] = x3;
        scale3(tp, (double)(d1 + d3), tp);  // tp *= d1+d3
        rc_unit_Ut(U, tp, t);
        rc_store_motion(a, p, 4 + i, mul3(mul3_alpha(U, Rp, (double)s), Vt), t);
    }
    a.n_motion[p] = 8;
}

// What CheckRT prepares once per call: P2 = K*[R|t] and O2 = -R.t()*t
struct RcPose {
    float R[9], t[3], P2[12], O2[3];
};

__device__ __forceinline__ RcPose rc_pose(const RecArgs& a, int p, int h) {
    RcPose q;
#pragma unroll
    for (int e = 0; e < 9; ++e) q.R[e] = a.motion_R[(size_t)p * 72 + h * 9 + e];
#pragma unroll
    for (int e = 0; e < 3; ++e) q.t[e] = a.motion_t[(size_t)p * 24 + h * 3 + e];
    const float K[9] = {a.fx, 0.0f, a.cx, 0.0f, a.fy, a.cy, 0.0f, 0.0f, 1.0f};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {  // the short path, 3 x 3 by 3 x 4; K's zeros are not skipped (0 * inf)
            const float b0 = j < 3 ? q.R[j] : q.t[0], b1 = j < 3 ? q.R[3 + j] : q.t[1], b2 = j < 3 ? q.R[6 + j] : q.t[2];
            q.P2[i * 4 + j] = K[3 * i] * b0 + K[3 * i + 1] * b1 + K[3 * i + 2] * b2;
        }
    orb_cv::camera_centre(q.R, q.t, q.O2);
    return q;
}

// One match of CheckRT (Initializer.cc:830-891) on the lane's LDS column.  Returns bit 0: counted
// (nGood, vCosParallax, vP3D), bit 1: vbGood.
__device__ int rc_check_one(const RecArgs& a, const RcPose& q, float x1, float y1, float x2, float y2,
                            const TriColumn& col, float* cosp, float* pt) {
    // Triangulate with P1 = K[I|0] and P2
    const float P1[12] = {a.fx, 0.0f, a.cx, 0.0f, 0.0f, a.fy, a.cy, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f};
    const float xs[4] = {x1, y1, x2, y2};
    float vr[4];
    triangulate_vt3(P1, q.P2, xs, col, vr);
    float p3[3];
    scale3(vr, 1. / (double)vr[3], p3);  // rowRange(0,3)/x3D.at<float>(3): a MatExpr scale
    if (!__builtin_isfinite(p3[0]) || !__builtin_isfinite(p3[1]) || !__builtin_isfinite(p3[2])) return 0;
    const float O1[3] = {0.0f, 0.0f, 0.0f};
    float n1[3], n2[3];
    orb_cv::sub3(p3, O1, n1);
    orb_cv::sub3(p3, q.O2, n2);
    const float dist1 = (float)norm3(n1);
    const float dist2 = (float)norm3(n2);
    const float cosParallax = (float)(orb_cv::dot3(n1, n2) / (double)(dist1 * dist2));
    const bool low = (double)cosParallax < 0.99998;
    if (p3[2] <= 0.0f && low) return 0;
    float p2[3];
    orb_cv::gemm3_add(q.R, p3, q.t, p2);  // R*p3dC1+t
    if (p2[2] <= 0.0f && low) return 0;
    const float invZ1 = (float)(1.0 / (double)p3[2]);
    const float im1x = __builtin_fmaf(a.fx * p3[0], invZ1, a.cx);
    const float im1y = __builtin_fmaf(a.fy * p3[1], invZ1, a.cy);
    const float e1 = __builtin_fmaf(im1x - x1, im1x - x1, (im1y - y1) * (im1y - y1));
    if (e1 > a.th2) return 0;
    const float invZ2 = (float)(1.0 / (double)p2[2]);
    const float im2x = __builtin_fmaf(a.fx * p2[0], invZ2, a.cx);
    const float im2y = __builtin_fmaf(a.fy * p2[1], invZ2, a.cy);
    const float e2 = __builtin_fmaf(im2x - x2, im2x - x2, (im2y - y2) * (im2y - y2));
    if (e2 > a.th2) return 0;
    *cosp = cosParallax;
    pt[0] = p3[0], pt[1] = p3[1], pt[2] = p3[2];
    return low ? 3 : 1;
}

__global__ void __launch_bounds__(64) k_init_checkrt(RecArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t smem[TRI_WAVE_BYTES];
    const int p = blockIdx.z, h = blockIdx.y, lane = threadIdx.x;
    const int o = blockIdx.x * 64 + lane;
    if (h >= a.n_motion[p] || o >= a.nwalk[p]) return;  // (no barrier below: every lane works on its own column)
    const size_t row = ((size_t)p * 8 + h) * a.cap;
    const uint8_t* mask = (a.use_h[p] != 0 ? a.inl_h : a.inl_f) + (size_t)p * a.cap;
    int fl = 0;
    float cs = 0.0f;
    if (mask[o] != 0) {
        const PairView v = rec_view(a, p);
        const int i = a.ord_i[(size_t)p * a.cap + o];
        const int m = v.m12[i];
        const RcPose q = rc_pose(a, p, h);
        float pt[3];
        fl = rc_check_one(a, q, v.k1[i].x, v.k1[i].y, v.k2[m].x, v.k2[m].y, TriColumn(smem, lane), &cs, pt);
    }
    a.flags[row + o] = (uint8_t)fl;
    a.cosv[row + o] = cs;
}

__global__ void __launch_bounds__(RC_THREADS) k_init_stat(RecArgs a) {
    __shared__ float s_c[IN_MAX_CAP];
    __shared__ int s_n;
    const int h = blockIdx.x, p = blockIdx.y, tid = threadIdx.x;
    const size_t g = (size_t)p * 8 + h;
    if (h >= a.n_motion[p]) {
        if (tid == 0) {
            a.n_good[g] = 0;
            a.cos_sel[g] = __builtin_nanf("");
            a.parallax[g] = 0.0f;
        }
        return;
    }
    if (tid == 0) s_n = 0;
    __syncthreads();
    const int Nw = a.nwalk[p];
    for (int o = tid; o < Nw; o += RC_THREADS)
        if (a.flags[g * a.cap + o] & 1) s_c[atomicAdd(&s_n, 1)] = a.cosv[g * a.cap + o];
    __syncthreads();
    const int nGood = s_n;
    if (nGood == 0) {
        if (tid == 0) {
            a.n_good[g] = 0;
            a.cos_sel[g] = __builtin_nanf("");
            a.parallax[g] = 0.0f;
        }
        return;
    }
    // sorted[min(50, size - 1)]: the element with exactly that many before it, where "before" is a
    // smaller value, a number before a NaN, or an equal value in a lower slot
    const int idx = min(50, nGood - 1);
    for (int e = tid; e < nGood; e += RC_THREADS) {
        const float ce = s_c[e];
        const bool en = ce != ce;
        int rank = 0;
        for (int j = 0; j < nGood; ++j) {
            const float cj = s_c[j];
            const bool jn = cj != cj;
            const bool before = cj < ce || (en && !jn) || ((cj == ce || (en && jn)) && j < e);
            rank += before;
        }
        if (rank == idx) {
            a.n_good[g] = nGood;
            a.cos_sel[g] = ce;
            // acos(float) is acosf; * 180 in float; / CV_PI in double; narrowed
            a.parallax[g] = (float)((double)(acosf(ce) * 180.0f) / RC_PI);
        }
    }
}

__global__ void __launch_bounds__(RC_THREADS) k_init_select(RecArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t smem[(RC_THREADS / 64) * TRI_WAVE_BYTES];
    __shared__ int s_best;
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nm = a.n_motion[p];
    if (tid == 0) {
        const int32_t* ng = a.n_good + (size_t)p * 8;
        const float* par = a.parallax + (size_t)p * 8;
        const int N = a.n_inliers[p];
        int b = -1;
        if (nm == 4) {  // ReconstructF (Initializer.cc:497-567)
            const int maxGood = max(ng[0], max(ng[1], max(ng[2], ng[3])));
            const int nMinGood = max((int)(0.9 * (double)N), a.min_triangulated);
            int nsimilar = 0;
            for (int k = 0; k < 4; ++k) nsimilar += (double)ng[k] > 0.7 * (double)maxGood;
            if (!(maxGood < nMinGood || nsimilar > 1))
                for (int k = 0; k < 4; ++k)
                    if (ng[k] == maxGood) {  // the else-if chain: the first one decides alone
                        if (par[k] > a.min_parallax) b = k;
                        break;
                    }
        } else if (nm == 8) {  // ReconstructH (687-729)
            int bestGood = 0, secondBestGood = 0, bestIdx = -1;
            float bestParallax = -1.0f;
            for (int k = 0; k < 8; ++k) {
                if (ng[k] > bestGood) {
                    secondBestGood = bestGood;
                    bestGood = ng[k];
                    bestIdx = k;
                    bestParallax = par[k];
                } else if (ng[k] > secondBestGood)
                    secondBestGood = ng[k];
            }
            if ((double)secondBestGood < 0.75 * (double)bestGood && bestParallax >= a.min_parallax &&
                bestGood > a.min_triangulated && (double)bestGood > 0.9 * (double)N)
                b = bestIdx;
        }
        s_best = b;
        a.best[p] = b;
        if (a.ok) a.ok[p] = b >= 0;
        if (a.R21)
            for (int e = 0; e < 9; ++e) a.R21[(size_t)p * 9 + e] = b >= 0 ? a.motion_R[(size_t)p * 72 + b * 9 + e] : 0.0f;
        if (a.t21)
            for (int e = 0; e < 3; ++e) a.t21[(size_t)p * 3 + e] = b >= 0 ? a.motion_t[(size_t)p * 24 + b * 3 + e] : 0.0f;
    }
    float* P3D = a.P3D ? a.P3D + (size_t)p * a.cap * 3 : nullptr;
    uint8_t* tri = a.triangulated ? a.triangulated + (size_t)p * a.cap : nullptr;
    for (int i = tid; i < a.cap; i += RC_THREADS) {
        if (P3D) P3D[3 * i] = P3D[3 * i + 1] = P3D[3 * i + 2] = 0.0f;
        if (tri) tri[i] = 0;
    }
    __syncthreads();
    const int b = s_best;
    if (b < 0 || (!P3D && !tri)) return;
    // vP3D / vbTriangulated of the winner, indexed by the frame-1 keypoint: the counted ordinals'
    // points again, by the function that counted them
    const PairView v = rec_view(a, p);
    const RcPose q = rc_pose(a, p, b);
    const uint8_t* fl = a.flags + ((size_t)p * 8 + b) * a.cap;
    const TriColumn col(smem + wave * TRI_WAVE_BYTES, lane);
    const int Nw = a.nwalk[p];
    for (int o = tid; o < Nw; o += RC_THREADS) {
        if (!(fl[o] & 1)) continue;
        const int i = a.ord_i[(size_t)p * a.cap + o];
        const int m = v.m12[i];
        float cs, pt[3] = {0.0f, 0.0f, 0.0f};
        const int f = rc_check_one(a, q, v.k1[i].x, v.k1[i].y, v.k2[m].x, v.k2[m].y, col, &cs, pt);
        if (P3D) P3D[3 * i] = pt[0], P3D[3 * i + 1] = pt[1], P3D[3 * i + 2] = pt[2];
        if (tri) tri[i] = (f & 2) ? 1 : 0;
    }
}

int check_rec_params(const std::string& w, const float* K4, float sigma, float min_parallax, int min_triangulated) {
    if (!K4) return fail(ORB_EINVAL, w + "K4 is NULL");
    if (int r = orb_check_camera(w.substr(0, w.size() - 2).c_str(), "", K4)) return r;
    if (!std::isfinite(sigma) || sigma == 0.0f)
        return fail(ORB_EINVAL, w + "sigma = " + std::to_string(sigma) + " must be finite and not 0");
    if (!std::isfinite(min_parallax))
        return fail(ORB_EINVAL, w + "min_parallax = " + std::to_string(min_parallax) + " must be finite");
    if (min_triangulated < 0)
        return fail(ORB_EINVAL, w + "min_triangulated = " + std::to_string(min_triangulated) + " is negative");
    return ORB_OK;
}

// k_init_motion -> k_init_checkrt -> k_init_stat -> k_init_select, enqueued on `st`.  `scratch`:
// `scratch_bytes` of device memory for rec_regions(), or NULL for a stream-ordered allocation freed
// after the last kernel.
int run_reconstruct(const orb_keypoint_t* d_kps, const int32_t* d_counts, int cap, int P, const int32_t* d_pair_f1,
                    const int32_t* d_pair_f2, const int32_t* d_matches12, const float* d_H21, const float* d_F21,
                    const int32_t* d_use_h, const uint8_t* d_inl_h, const uint8_t* d_inl_f, const int32_t* d_n_matches,
                    const float* K4, float sigma, float min_parallax, int min_triangulated, const RecOut& o,
                    uint8_t* scratch, size_t scratch_bytes, hipStream_t st) {
    RecArgs a{};
    void* owned = nullptr;
    if (scratch) {
        OrbLayout L(scratch);
        rec_regions(L, o, cap, P, a);
        assert(L.end <= scratch_bytes);
    } else if (int r = orb_scratch_alloc(&owned, st, "initializer reconstruct: scratch: ",
                                         [&](OrbLayout& L) { rec_regions(L, o, cap, P, a); }))
        return r;
    a.kps = d_kps;
    a.counts = d_counts;
    a.pair_f1 = d_pair_f1;
    a.pair_f2 = d_pair_f2;
    a.matches12 = d_matches12;
    a.H21 = d_H21;
    a.F21 = d_F21;
    a.use_h = d_use_h;
    a.inl_h = d_inl_h;
    a.inl_f = d_inl_f;
    a.n_matches = d_n_matches;
    a.fx = K4[0];
    a.fy = K4[1];
    a.cx = K4[2];
    a.cy = K4[3];
    const float sigma2 = sigma * sigma;  // mSigma2
    a.th2 = (float)(4.0 * (double)sigma2);  // 4.0*mSigma2, narrowed at the call
    a.min_parallax = min_parallax;
    a.min_triangulated = min_triangulated;
    a.ok = o.ok;
    a.R21 = o.R21;
    a.t21 = o.t21;
    a.P3D = o.P3D;
    a.triangulated = o.triangulated;
    a.cap = cap;
    a.P = P;
    hipError_t e = hipSuccess;
    hipLaunchKernelGGL(k_init_motion, dim3(P), dim3(RC_THREADS), 0, st, a);
    if ((e = hipGetLastError()) == hipSuccess) {
        hipLaunchKernelGGL(k_init_checkrt, dim3((cap + 63) / 64, 8, P), dim3(64), 0, st, a);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_init_stat, dim3(8, P), dim3(RC_THREADS), 0, st, a);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_init_select, dim3(P), dim3(RC_THREADS), 0, st, a);
        e = hipGetLastError();
    }
    if (owned) (void)hipFreeAsync(owned, st);
    if (e != hipSuccess) return fail(ORB_EDEVICE, std::string("initializer reconstruct: ") + hipGetErrorString(e));
    return ORB_OK;
}

int check_batch_args(const std::string& w, int cap, int P) {
    if (P < 0 || cap <= 0) return fail(ORB_EINVAL, w + "bad arguments");
    if (cap > IN_MAX_CAP) return fail(ORB_ENOTSUP, w + "more than 8192 keypoints per frame");
    if (P > 65535) return fail(ORB_ENOTSUP, w + "more than 65535 pairs per call");
    return ORB_OK;
}

}  // namespace

extern "C" {

int orb_initializer_reconstruct_batch_device(const orb_keypoint_t* d_kps, const int32_t* d_counts, int cap, int P,
                                             const int32_t* d_pair_f1, const int32_t* d_pair_f2,
                                             const int32_t* d_matches12, const float* d_best_H21,
                                             const float* d_best_F21, const int32_t* d_use_h,
                                             const uint8_t* d_inliers_h, const uint8_t* d_inliers_f,
                                             const int32_t* d_n_matches, const float* K4, float sigma,
                                             float min_parallax, int min_triangulated, int32_t* d_ok, float* d_R21,
                                             float* d_t21, float* d_P3D, uint8_t* d_triangulated, int32_t* d_n_motion,
                                             float* d_motion_R, float* d_motion_t, int32_t* d_n_good,
                                             float* d_cos_parallax, float* d_parallax_deg, int32_t* d_best,
                                             int32_t* d_n_inliers, void* stream) {
    const std::string w = "initializer reconstruct: ";
    if (int r = check_batch_args(w, cap, P)) return r;
    if (int r = check_rec_params(w, K4, sigma, min_parallax, min_triangulated)) return r;
    if (P == 0) return ORB_OK;
    if (!d_kps || !d_counts || !d_pair_f1 || !d_pair_f2 || !d_matches12 || !d_best_H21 || !d_best_F21 || !d_use_h ||
        !d_inliers_h || !d_inliers_f)
        return fail(ORB_EINVAL, w + "bad arguments");
    const RecOut o{d_ok, d_R21, d_t21, d_P3D, d_triangulated, d_n_motion, d_motion_R, d_motion_t,
                   d_n_good, d_cos_parallax, d_parallax_deg, d_best, d_n_inliers};
    return run_reconstruct(d_kps, d_counts, cap, P, d_pair_f1, d_pair_f2, d_matches12, d_best_H21, d_best_F21, d_use_h,
                           d_inliers_h, d_inliers_f, d_n_matches, K4, sigma, min_parallax, min_triangulated, o, nullptr,
                           0, (hipStream_t)stream);
}

int orb_initializer_reconstruct(const orb_keypoint_t* kps1, int n1, const orb_keypoint_t* kps2, int n2,
                                const int32_t* matches12, const float* M21, int use_h, const uint8_t* inliers,
                                const float* K4, float sigma, float min_parallax, int min_triangulated, int32_t* ok,
                                float* R21, float* t21, float* P3D, uint8_t* triangulated, int32_t* n_motion,
                                float* motion_R, float* motion_t, int32_t* n_good, float* cos_parallax,
                                float* parallax_deg, int32_t* best, int32_t* n_inliers, int device) {
    const std::string w = "initializer reconstruct: ";
    if (n1 < 0 || n2 < 0 || (n1 && (!kps1 || !matches12)) || (n2 && !kps2)) return fail(ORB_EINVAL, w + "bad arguments");
    if (!M21) return fail(ORB_EINVAL, w + "M21 is NULL");
    if (use_h != 0 && use_h != 1) return fail(ORB_EINVAL, w + "use_h = " + std::to_string(use_h) + " is not 0 or 1");
    const int cap = std::max(std::max(n1, n2), 1);
    if (cap > IN_MAX_CAP) return fail(ORB_ENOTSUP, w + "more than 8192 keypoints per frame");
    if (int r = check_rec_params(w, K4, sigma, min_parallax, min_triangulated)) return r;
    int N;
    if (int r = check_matches(w, matches12, n1, n2, &N)) return r;
    if (N && !inliers) return fail(ORB_EINVAL, w + "inliers is NULL");
    for (int k = 0; k < N; ++k)
        if (inliers[k] > 1)
            return fail(ORB_EINVAL, w + "inliers[" + std::to_string(k) + "] = " + std::to_string((int)inliers[k]) +
                                        " is not 0 or 1");
    OrbStagePlan P;
    const PairStage pair(P, cap, 5);  // the header ends with use_h
    const auto rMod = P.in<float>(9);
    const auto rI = P.in<uint8_t>(cap);
    const auto rS = P.out<int32_t>(4);  // ok, best, n_motion, n_inliers
    const auto rR = P.out<float>(12);   // R21 9, t21 3
    const auto rMR = P.out<float>(72), rMT = P.out<float>(24);
    const auto rG = P.out<int32_t>(8);
    const auto rCs = P.out<float>(8), rPa = P.out<float>(8), rP = P.out<float>((size_t)cap * 3);
    const auto rT = P.out<uint8_t>(cap);
    RecArgs a0{};  // the chain's scratch at its most, as if no optional output were given
    const auto rX = P.scratch<uint8_t>(orb_layout_size([&](OrbLayout& L) { rec_regions(L, RecOut{}, cap, 1, a0); }));
    OrbHostCall call(P, device);
    if (call.err) return call.err;
    pair.fill(call, kps1, n1, kps2, n2, matches12, use_h);
    const float* d_model = call.send(rMod, M21);
    call.put(rI, inliers, N);
    if (int r = call.upload()) return r;
    const int32_t* dc = call.dev(pair.hdr);
    int32_t* ds = call.dev(rS);
    const RecOut o{ds, call.dev(rR), call.dev(rR) + 9, call.dev(rP), call.dev(rT), ds + 2, call.dev(rMR),
                   call.dev(rMT), call.dev(rG), call.dev(rCs), call.dev(rPa), ds + 1, ds + 3};
    // the one model and the one mask serve whichever use_h names
    const int r = run_reconstruct(call.dev(pair.kps), dc, cap, 1, dc + 2, dc + 3, call.dev(pair.matches), d_model,
                                  d_model, dc + 4, call.dev(rI), call.dev(rI), nullptr, K4, sigma, min_parallax,
                                  min_triangulated, o, call.dev(rX), rX.count, call.stream());
    if (int rf = call.finish(r, hipSuccess, w)) return rf;
    call.get(rS, ok, 1, 0);
    call.get(rS, best, 1, 1);
    call.get(rS, n_motion, 1, 2);
    call.get(rS, n_inliers, 1, 3);
    call.get(rR, R21, 9);
    call.get(rR, t21, 3, 9);
    call.get(rMR, motion_R);
    call.get(rMT, motion_t);
    call.get(rG, n_good);
    call.get(rCs, cos_parallax);
    call.get(rPa, parallax_deg);
    call.get(rP, P3D, (size_t)n1 * 3);
    call.get(rT, triangulated, (size_t)n1);
    return ORB_OK;
}

int orb_initializer_initialize(const orb_keypoint_t* kps1, int n1, const orb_keypoint_t* kps2, int n2,
                               const int32_t* matches12, float sigma, int n_hyp, const int32_t* rand31, const float* K4,
                               float min_parallax, int min_triangulated, float* H21, float* H12, float* F21,
                               int32_t* sets_out, float* scores_h, float* scores_f, int32_t* best_h,
                               float* best_score_h, uint8_t* inliers_h, int32_t* best_f, float* best_score_f,
                               uint8_t* inliers_f, float* best_H21, float* best_F21, float* RH, int32_t* use_h,
                               int* n_matches, int32_t* ok, float* R21, float* t21, float* P3D, uint8_t* triangulated,
                               int32_t* n_motion, float* motion_R, float* motion_t, int32_t* n_good,
                               float* cos_parallax, float* parallax_deg, int32_t* best, int32_t* n_inliers,
                               int device) {
    if (int r = check_rec_params("initializer initialize: ", K4, sigma, min_parallax, min_triangulated)) return r;
    // the model, the mask and use_h pass through the host between the two chains (the batch form
    // keeps them on the device)
    std::vector<uint8_t> ih, jf;
    float bH[9], bF[9];
    int32_t uh = 0;
    if (!inliers_h) {
        ih.resize((size_t)std::max(n1, 1));
        inliers_h = ih.data();
    }
    if (!inliers_f) {
        jf.resize((size_t)std::max(n1, 1));
        inliers_f = jf.data();
    }
    if (int r = orb_initializer_ransac(kps1, n1, kps2, n2, matches12, sigma, n_hyp, rand31, H21, H12, F21, sets_out,
                                       scores_h, scores_f, best_h, best_score_h, inliers_h, best_f, best_score_f,
                                       inliers_f, bH, bF, RH, &uh, n_matches, device))
        return r;
    if (best_H21) std::memcpy(best_H21, bH, 36);
    if (best_F21) std::memcpy(best_F21, bF, 36);
    if (use_h) *use_h = uh;
    return orb_initializer_reconstruct(kps1, n1, kps2, n2, matches12, uh ? bH : bF, uh, uh ? inliers_h : inliers_f, K4,
                                       sigma, min_parallax, min_triangulated, ok, R21, t21, P3D, triangulated, n_motion,
                                       motion_R, motion_t, n_good, cos_parallax, parallax_deg, best, n_inliers, device);
}

int orb_initializer_initialize_batch_device(
    const orb_keypoint_t* d_kps, const int32_t* d_counts, int cap, int P, const int32_t* d_pair_f1,
    const int32_t* d_pair_f2, const int32_t* d_matches12, float sigma, int n_hyp, const int32_t* d_rand31,
    const float* K4, float min_parallax, int min_triangulated, float* d_H21, float* d_H12, float* d_F21,
    int32_t* d_sets_out, float* d_scores_h, float* d_scores_f, int32_t* d_best_h, float* d_best_score_h,
    uint8_t* d_inliers_h, int32_t* d_best_f, float* d_best_score_f, uint8_t* d_inliers_f, int32_t* d_n_matches,
    float* d_best_H21, float* d_best_F21, float* d_RH, int32_t* d_use_h, int32_t* d_ok, float* d_R21, float* d_t21,
    float* d_P3D, uint8_t* d_triangulated, int32_t* d_n_motion, float* d_motion_R, float* d_motion_t,
    int32_t* d_n_good, float* d_cos_parallax, float* d_parallax_deg, int32_t* d_best, int32_t* d_n_inliers,
    void* stream) {
    const std::string w = "initializer initialize: ";
    if (int r = check_batch_args(w, cap, P)) return r;
    if (int r = check_limits(cap, n_hyp, true, true)) return r;
    if (int r = check_rec_params(w, K4, sigma, min_parallax, min_triangulated)) return r;
    if (P == 0) return ORB_OK;
    if (!d_kps || !d_counts || !d_pair_f1 || !d_pair_f2 || !d_matches12 || !d_rand31)
        return fail(ORB_EINVAL, w + "bad arguments");
    hipStream_t st = (hipStream_t)stream;
    // what passes from the first chain to the second and the caller did not ask for
    const size_t p = (size_t)P;
    ChainOut o{};
    o.H21 = d_H21;
    o.H12 = d_H12;
    o.F21 = d_F21;
    o.sets_out = d_sets_out;
    o.scores_h = d_scores_h;
    o.scores_f = d_scores_f;
    o.best_h = d_best_h;
    o.best_score_h = d_best_score_h;
    o.best_f = d_best_f;
    o.best_score_f = d_best_score_f;
    o.RH = d_RH;
    void* link = nullptr;
    if (int r = orb_scratch_alloc(&link, st, w + "scratch: ", [&](OrbLayout& L) {
            o.inliers_h = L.given_or_take(d_inliers_h, p * cap);
            o.inliers_f = L.given_or_take(d_inliers_f, p * cap);
            o.n_matches = L.given_or_take(d_n_matches, p);
            o.best_H21 = L.given_or_take(d_best_H21, p * 9);
            o.best_F21 = L.given_or_take(d_best_F21, p * 9);
            o.use_h = L.given_or_take(d_use_h, p);
        }))
        return r;
    int r = run_chain(d_kps, d_counts, cap, P, d_pair_f1, d_pair_f2, d_matches12, sigma, n_hyp, d_rand31, nullptr, true, o,
                      nullptr, 0, st);
    if (r == ORB_OK) {
        const RecOut ro{d_ok, d_R21, d_t21, d_P3D, d_triangulated, d_n_motion, d_motion_R, d_motion_t,
                        d_n_good, d_cos_parallax, d_parallax_deg, d_best, d_n_inliers};
        r = run_reconstruct(d_kps, d_counts, cap, P, d_pair_f1, d_pair_f2, d_matches12, o.best_H21, o.best_F21, o.use_h,
                            o.inliers_h, o.inliers_f, o.n_matches, K4, sigma, min_parallax, min_triangulated, ro, nullptr,
                            0, st);
    }
    if (link) (void)hipFreeAsync(link, st);
    return r;
}

}  // extern "C"
