// orb_solvers.hip — the RANSAC consensus of PnPsolver and Sim3Solver on the GPU (part of liborb_hip.so).
//
// PnPsolver::CheckInliers (reference src/PnPsolver.cc:280-311) and Sim3Solver::CheckInliers
// (src/Sim3Solver.cc:335-359, with Project 377-398) for every hypothesis of a solver at once, the
// per-correspondence set-up of the two constructors (PnPsolver.cc:40-82, 126-128;
// Sim3Solver.cc:37-112) and the keep-the-best rules of the two iterate() loops (PnPsolver.cc:181-196,
// Sim3Solver.cc:183-200).  The hypotheses themselves (EPnP compute_pose, Horn's computeT) and the
// random minimal sets are the caller's.
//
// Arithmetic: the TU is built -ffp-contract=off and the fused multiply-adds that g++ -O3
// -march=native makes of the reference's own translation units are written out
// (scripts/contraction_check_solvers.sh prints the disassembly they are read from):
//   PnP   r0*X + r1*Y + r2*Z + t (double)  ->  fma(r2, Z, fma(r0, X, r1*Y)) + t
//         1/(row 2)                        ->  a double divide, narrowed to float
//         uc + fu*Xc*invZc                 ->  fma(fu*(double)Xc, (double)invZc, uc)
//         distX*distX + distY*distY        ->  fmaf(distX, distX, distY*distY)
//   Sim3  1/z, X*invz                      ->  float divide, float multiply
//         fx*x + cx                        ->  fmaf(fx, x, cx)
// Sim3's cv::Mat arithmetic is OpenCV's binary and is not contracted: Rcw*X + tcw is a float row
// sum taken left to right and then (float)((double)sum + (double)t); a - b is a float subtraction;
// d.dot(d) is a double accumulation narrowed to float.  Its bound is the reference's
// std::vector<size_t> entry: (size_t)(9.210 * sigma2), converted to float by the compare.
// The result of a consensus is an integer count and a bit mask, so nothing here depends on an
// order of additions.
//
//   k_cons_prepare<M>  one workgroup per solver: compacts the match row in index order (ballot +
//                      popcount prefix, wave totals through LDS) and writes the per-correspondence
//                      values as SoA scratch, n and the index list; zeroes the solver's counts.
//   k_cons_score<M>    grid (solver, tile of 64 hypotheses, groups of 4 mask words), 4 waves.  A
//                      wave owns 64 correspondences, lane = correspondence with its values in
//                      registers; it loops over the tile's hypotheses, whose coefficients are
//                      wave-uniform loads.  One __ballot per hypothesis is the mask word (one lane
//                      stores it); the popcounts are summed per hypothesis in LDS and added to
//                      `counts` with one integer atomic per (workgroup, hypothesis).
//   k_cons_select<M>   one workgroup per solver: prefix maxima over the <= 1024 counts give the
//                      running best, its holder after every iteration and the first qualifying /
//                      accepted iteration.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <string>

#include "../../include/orb_abi.h"
#include "orb_internal.h"

namespace {

int fail(int code, const std::string& msg) { return orb_internal_set_error(code, msg); }
constexpr auto al = orb_align256;  // (a short name for the layout lines)

constexpr int CS_MAX_CAP = 8192;
constexpr int CS_MAX_HYP = 1024;
constexpr int CS_TILE = 64;            // hypotheses per workgroup = lanes that carry a count
constexpr int CS_WAVES = 4;            // mask words (64 correspondences each) per workgroup
constexpr int CS_THREADS = 64 * CS_WAVES;
constexpr int CS_PREP_THREADS = 256;
constexpr int CS_SEL_THREADS = CS_MAX_HYP;
constexpr int PNP = 0, SIM3 = 1;
constexpr int NV_PNP = 6;    // X Y Z px py maxErr
constexpr int NV_SIM3 = 12;  // X3Dc1 (3) X3Dc2 (3) P1im1 (2) P2im2 (2) bound1 bound2

struct ConsArgs {
    // source, batch form: extractor records, one match row per solver, MapPoint attributes
    const orb_keypoint_t* kps;
    const int32_t* kcounts;
    const int32_t* pair_a;
    const int32_t* pair_b;
    const int32_t* match;
    const float* mp_pos;
    const uint8_t* mp_bad;
    const float* pose;
    // source, one solver already compact (the host entry points): n_direct >= 0 and
    // PnP  c0 = p3d (n x 3), c1 = p2d (n x 2), c2 = sigma2
    // Sim3 c0 = x3dc1, c1 = x3dc2 (n x 3), c2 = sigma2_1, c3 = sigma2_2
    const float* c0;
    const float* c1;
    const float* c2;
    const float* c3;
    int n_direct;
    float level_sigma2[ORB_MAX_VIEW_LEVELS];
    int nlevels;
    float th2;
    float K1[4], K2[4];
    double fu, fv, uc, vc;
    const int32_t* best_in;
    int min_inliers;
    // scratch and outputs (masks, index, best_at, first may be NULL)
    float* soa;  // S x NV x cap
    int32_t* n;
    int32_t* index;
    int32_t* counts;
    uint64_t* masks;
    int32_t* best_at;
    int32_t* first;
    int cap, S, n_hyp, W;
};

// cv::Mat A(3x3) * x + t as OpenCV 2.4's gemm evaluates it: A row-major with `stride` floats per
// row, t at A-relative `t` with `tstride`.
__device__ __forceinline__ void gemm3_add(const float* A, int stride, const float* t, int tstride, float x0, float x1,
                                          float x2, float* out) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        float s = A[i * stride] * x0;
        s = s + A[i * stride + 1] * x1;
        s = s + A[i * stride + 2] * x2;
        out[i] = (float)((double)s + (double)t[i * tstride]);
    }
}

// Project / FromCameraToImage (Sim3Solver.cc:392-396, 412-416)
__device__ __forceinline__ void to_image(float X, float Y, float Z, const float* K, float* u, float* v) {
    const float invz = 1.0f / Z;
    const float x = X * invz;
    const float y = Y * invz;
    *u = __builtin_fmaf(K[0], x, K[2]);
    *v = __builtin_fmaf(K[1], y, K[3]);
}

// (a - b).dot(a - b) of two 2x1 CV_32F
__device__ __forceinline__ float diff_dot2(float a0, float a1, float b0, float b1) {
    const float d0 = a0 - b0, d1 = a1 - b1;
    double r = 0;
    r += (double)d0 * (double)d0;
    r += (double)d1 * (double)d1;
    return (float)r;
}

__device__ __forceinline__ double pnp_row(const double* r, double t, float X, float Y, float Z) {
    return __builtin_fma(r[2], (double)Z, __builtin_fma(r[0], (double)X, r[1] * (double)Y)) + t;
}

__device__ __forceinline__ int clamp_level(const ConsArgs& a, int octave) {
    return min(max(octave, 0), a.nlevels - 1);
}

// The values of correspondence `o` of solver `s` from the compact inputs' element `i` (direct) or
// from the batch (first-side index i, second-side index m).
template <int MODEL>
__device__ __forceinline__ void emit(const ConsArgs& a, int s, int o, int i, int m) {
    float* q = a.soa + (size_t)s * (MODEL == PNP ? NV_PNP : NV_SIM3) * a.cap + o;
    const int cap = a.cap;
    const bool direct = a.n_direct >= 0;
    if (MODEL == PNP) {
        // batch: i = the frame's keypoint (pair_b), m = the keyframe's keypoint (pair_a) and its MapPoint
        float X, Y, Z, px, py, s2;
        if (direct) {
            X = a.c0[3 * i], Y = a.c0[3 * i + 1], Z = a.c0[3 * i + 2];
            px = a.c1[2 * i], py = a.c1[2 * i + 1];
            s2 = a.c2[i];
        } else {
            const size_t kf = (size_t)a.pair_a[s] * cap + m;
            const orb_keypoint_t& kp = a.kps[(size_t)a.pair_b[s] * cap + i];
            X = a.mp_pos[3 * kf], Y = a.mp_pos[3 * kf + 1], Z = a.mp_pos[3 * kf + 2];
            px = kp.x, py = kp.y;
            s2 = a.level_sigma2[clamp_level(a, kp.octave)];
        }
        q[0] = X, q[cap] = Y, q[2 * cap] = Z, q[3 * cap] = px, q[4 * cap] = py;
        q[5 * cap] = s2 * a.th2;  // mvMaxError (PnPsolver.cc:128)
    } else {
        float X1[3], X2[3], s1, s2;
        if (direct) {
#pragma unroll
            for (int k = 0; k < 3; ++k) X1[k] = a.c0[3 * i + k], X2[k] = a.c1[3 * i + k];
            s1 = a.c2[i], s2 = a.c3[i];
        } else {
            const int fa = a.pair_a[s], fb = a.pair_b[s];
            const size_t k1 = (size_t)fa * cap + i, k2 = (size_t)fb * cap + m;
            const float* Ta = a.pose + (size_t)fa * 12;
            const float* Tb = a.pose + (size_t)fb * 12;
            gemm3_add(Ta, 3, Ta + 9, 1, a.mp_pos[3 * k1], a.mp_pos[3 * k1 + 1], a.mp_pos[3 * k1 + 2], X1);
            gemm3_add(Tb, 3, Tb + 9, 1, a.mp_pos[3 * k2], a.mp_pos[3 * k2 + 1], a.mp_pos[3 * k2 + 2], X2);
            s1 = a.level_sigma2[clamp_level(a, a.kps[k1].octave)];
            s2 = a.level_sigma2[clamp_level(a, a.kps[k2].octave)];
        }
        float u1, v1, u2, v2;
        to_image(X1[0], X1[1], X1[2], a.K1, &u1, &v1);  // mvP1im1
        to_image(X2[0], X2[1], X2[2], a.K2, &u2, &v2);  // mvP2im2
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k * cap] = X1[k], q[(3 + k) * cap] = X2[k];
        q[6 * cap] = u1, q[7 * cap] = v1, q[8 * cap] = u2, q[9 * cap] = v2;
        // mvnMaxError1/2 are std::vector<size_t> (Sim3Solver.h:79-80, Sim3Solver.cc:87-88): the
        // double product truncated; err < bound then converts the integer to float
        q[10 * cap] = (float)(unsigned long long)(9.210 * (double)s1);
        q[11 * cap] = (float)(unsigned long long)(9.210 * (double)s2);
    }
}

template <int MODEL>
__global__ void __launch_bounds__(CS_PREP_THREADS) k_cons_prepare(ConsArgs a) {
    __shared__ int s_wtot[CS_PREP_THREADS / 64];
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int h = tid; h < a.n_hyp; h += CS_PREP_THREADS) a.counts[(size_t)s * a.n_hyp + h] = 0;
    if (a.n_direct >= 0) {
        for (int i = tid; i < a.n_direct; i += CS_PREP_THREADS) {
            emit<MODEL>(a, s, i, i, i);
            if (a.index) a.index[i] = i;
        }
        if (tid == 0) a.n[s] = a.n_direct;
        return;
    }
    // The row is indexed by the frame's keypoints for PnP (entry = keyframe keypoint, frame =
    // pair_b, keyframe = pair_a) and by keyframe a's for Sim3 (entry = keyframe b's).  An entry is
    // a match only inside both counts, so no read leaves the batch arrays.
    const int fa = a.pair_a[s], fb = a.pair_b[s];
    const int na = min(max(a.kcounts[fa], 0), a.cap), nb = min(max(a.kcounts[fb], 0), a.cap);
    const int n_row = MODEL == PNP ? nb : na;    // indices of the row
    const int n_ent = MODEL == PNP ? na : nb;    // range of its entries
    const int f_row = MODEL == PNP ? fb : fa, f_ent = MODEL == PNP ? fa : fb;
    const int32_t* row = a.match + (size_t)s * a.cap;
    int base = 0;
    for (int i0 = 0; i0 < n_row; i0 += CS_PREP_THREADS) {
        const int i = i0 + tid;
        const int m = i < n_row ? row[i] : -1;
        bool ok = (unsigned)m < (unsigned)n_ent;
        if (ok && a.mp_bad) {
            ok = !a.mp_bad[(size_t)f_ent * a.cap + m];
            if (MODEL == SIM3) ok = ok && !a.mp_bad[(size_t)f_row * a.cap + i];
        }
        const unsigned long long bal = __ballot(ok);
        if (lane == 0) s_wtot[wave] = __popcll(bal);
        __syncthreads();
        int off = base, tot = 0;
#pragma unroll
        for (int w = 0; w < CS_PREP_THREADS / 64; ++w) {
            const int t = s_wtot[w];
            if (w < wave) off += t;
            tot += t;
        }
        if (ok) {
            const int o = off + __popcll(bal & ((1ull << lane) - 1ull));
            emit<MODEL>(a, s, o, i, m);
            if (a.index) a.index[(size_t)s * a.cap + o] = i;
        }
        base += tot;
        __syncthreads();
    }
    // the index list past n reads -1
    if (a.index)
        for (int i = base + tid; i < a.cap; i += CS_PREP_THREADS) a.index[(size_t)s * a.cap + i] = -1;
    if (tid == 0) a.n[s] = base;
}

// HR / HT: the hypotheses of all solvers (PnP: R n_hyp x 9 and t n_hyp x 3 doubles; Sim3: T12 and
// T21, n_hyp x 12 floats), read at wave-uniform addresses.
template <int MODEL, class HT>
__global__ void __launch_bounds__(CS_THREADS) k_cons_score(ConsArgs a, const HT* __restrict__ HA,
                                                           const HT* __restrict__ HB) {
    __shared__ int s_cnt[CS_TILE];
    const int s = blockIdx.x, tile = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int word = blockIdx.z * CS_WAVES + wave;
    const int n = a.n[s], cap = a.cap;
    const int h0 = tile * CS_TILE, h1 = min(h0 + CS_TILE, a.n_hyp);
    if (tid < CS_TILE) s_cnt[tid] = 0;
    __syncthreads();
    uint64_t* masks = a.masks ? a.masks + (size_t)s * a.n_hyp * a.W : nullptr;
    const int i = word * 64 + lane;
    const bool valid = i < n;
    int cnt = 0;
    if (word < a.W && word * 64 >= n) {
        // past the solver's correspondences: the mask words are zero (lane = hypothesis)
        if (masks && h0 + lane < h1) masks[(size_t)(h0 + lane) * a.W + word] = 0;
    } else if (word < a.W) {
        constexpr int NV = MODEL == PNP ? NV_PNP : NV_SIM3;
        const float* q = a.soa + (size_t)s * NV * cap + i;
        float v[NV];
#pragma unroll
        for (int k = 0; k < NV; ++k) v[k] = valid ? q[(size_t)k * cap] : 0.0f;
        for (int h = h0; h < h1; ++h) {
            const size_t g = (size_t)s * a.n_hyp + h;
            bool in;
            if (MODEL == PNP) {
                const double* R = (const double*)HA + g * 9;
                const double* t = (const double*)HB + g * 3;
                const float Xc = (float)pnp_row(R, t[0], v[0], v[1], v[2]);
                const float Yc = (float)pnp_row(R + 3, t[1], v[0], v[1], v[2]);
                const float invZc = (float)(1.0 / pnp_row(R + 6, t[2], v[0], v[1], v[2]));
                const double ue = __builtin_fma(a.fu * (double)Xc, (double)invZc, a.uc);
                const double ve = __builtin_fma(a.fv * (double)Yc, (double)invZc, a.vc);
                const float distX = (float)((double)v[3] - ue);
                const float distY = (float)((double)v[4] - ve);
                const float error2 = __builtin_fmaf(distX, distX, distY * distY);
                in = error2 < v[5];
            } else {
                const float* T12 = (const float*)HA + g * 12;
                const float* T21 = (const float*)HB + g * 12;
                float P[3], u, w, e1, e2;
                gemm3_add(T12, 4, T12 + 3, 4, v[3], v[4], v[5], P);  // vP2im1: X3Dc2 through T12, K1
                to_image(P[0], P[1], P[2], a.K1, &u, &w);
                e1 = diff_dot2(v[6], v[7], u, w);                    // mvP1im1 - vP2im1
                gemm3_add(T21, 4, T21 + 3, 4, v[0], v[1], v[2], P);  // vP1im2: X3Dc1 through T21, K2
                to_image(P[0], P[1], P[2], a.K2, &u, &w);
                e2 = diff_dot2(u, w, v[8], v[9]);                    // vP1im2 - mvP2im2
                in = e1 < v[10] && e2 < v[11];
            }
            const unsigned long long bal = __ballot(valid && in);
            if (masks && lane == 0) masks[(size_t)h * a.W + word] = bal;
            cnt += lane == h - h0 ? __popcll(bal) : 0;
        }
        if (cnt) atomicAdd(&s_cnt[lane], cnt);
    }
    __syncthreads();
    if (tid < CS_TILE && h0 + tid < h1) {
        const int c = s_cnt[tid];
        if (c) atomicAdd(&a.counts[(size_t)s * a.n_hyp + h0 + tid], c);
    }
}

// Inclusive prefix maximum over CS_SEL_THREADS values (every thread calls it).
__device__ __forceinline__ int scan_max(int* s_a, int v) {
    const int tid = threadIdx.x;
    s_a[tid] = v;
    __syncthreads();
    for (int d = 1; d < CS_SEL_THREADS; d <<= 1) {
        int x = s_a[tid];
        if (tid >= d) x = max(x, s_a[tid - d]);
        __syncthreads();
        s_a[tid] = x;
        __syncthreads();
    }
    return s_a[tid];
}

template <int MODEL>
__global__ void __launch_bounds__(CS_SEL_THREADS) k_cons_select(ConsArgs a) {
    __shared__ int s_a[CS_SEL_THREADS];
    __shared__ int s_first;
    const int s = blockIdx.x, h = threadIdx.x;
    const bool live = h < a.n_hyp;
    const int best_in = a.best_in ? a.best_in[s] : 0;
    const int c = live ? a.counts[(size_t)s * a.n_hyp + h] : INT_MIN;
    if (h == 0) s_first = INT_MAX;
    // running best before iteration h: best_in and the counts that could have replaced it
    const bool qualifies = MODEL == PNP ? c >= a.min_inliers : true;  // PnPsolver.cc:181
    scan_max(s_a, max(h == 0 ? best_in : INT_MIN, live && qualifies ? c : INT_MIN));
    const int before = h == 0 ? best_in : s_a[h - 1];
    // PnP replaces on a strict > (PnPsolver.cc:184), Sim3 on >= (Sim3Solver.cc:183)
    const bool upd = live && qualifies && (MODEL == PNP ? c > before : c >= before);
    const bool hit = MODEL == PNP ? live && qualifies : upd && c > a.min_inliers;  // Sim3Solver.cc:192
    __syncthreads();
    const int holder = scan_max(s_a, upd ? h : (best_in > 0 ? -2 : -1));
    if (hit) atomicMin(&s_first, h);
    __syncthreads();
    if (live && a.best_at) a.best_at[(size_t)s * a.n_hyp + h] = holder;
    if (h == 0 && a.first) a.first[s] = s_first == INT_MAX ? -1 : s_first;
}

template <int MODEL, class HT>
int launch(const ConsArgs& a, const HT* HA, const HT* HB, hipStream_t st) {
    hipLaunchKernelGGL((k_cons_prepare<MODEL>), dim3(a.S), dim3(CS_PREP_THREADS), 0, st, a);
    ORB_HIPCHK(hipGetLastError());
    const int tiles = (a.n_hyp + CS_TILE - 1) / CS_TILE;
    const int zg = (std::max(a.W, 1) + CS_WAVES - 1) / CS_WAVES;
    hipLaunchKernelGGL((k_cons_score<MODEL, HT>), dim3(a.S, tiles, zg), dim3(CS_THREADS), 0, st, a, HA, HB);
    ORB_HIPCHK(hipGetLastError());
    hipLaunchKernelGGL((k_cons_select<MODEL>), dim3(a.S), dim3(CS_SEL_THREADS), 0, st, a);
    ORB_HIPCHK(hipGetLastError());
    return ORB_OK;
}

int check_limits(const char* who, int cap, int n_hyp) {
    if (cap > CS_MAX_CAP) return fail(ORB_ENOTSUP, std::string(who) + ": more than 8192 correspondences or keypoints");
    if (n_hyp < 1 || n_hyp > CS_MAX_HYP)
        return fail(ORB_EINVAL, std::string(who) + ": n_hyp must be in [1, 1024] (got " + std::to_string(n_hyp) + ")");
    return ORB_OK;
}

// sigma2 must be a finite value >= 0; for Sim3 its bound 9.210 * sigma2 must also fit the
// reference's size_t without the wrap of an out-of-range conversion.
int check_sigma2(const char* who, const float* s2, int n, bool sim3) {
    for (int i = 0; i < n; ++i) {
        const double b = 9.210 * (double)s2[i];
        if (!std::isfinite(s2[i]) || s2[i] < 0.0f || (sim3 && !(b < 9223372036854775808.0)))
            return fail(ORB_EINVAL, std::string(who) + ": sigma2[" + std::to_string(i) + "] = " +
                                        std::to_string(s2[i]) + " is not a finite value >= 0" +
                                        (sim3 ? " with 9.21 * sigma2 below 2^63" : ""));
    }
    return ORB_OK;
}

// One solver from compact host arrays: the common part of the two host entry points.  in[k]: the
// k-th input array with in_bytes[k] bytes (4 correspondence arrays, then the 2 hypothesis arrays).
template <int MODEL, class HT>
int run_host(ConsArgs a, const void* const* in, const size_t* in_bytes, int n, int32_t* counts, uint64_t* masks,
             int32_t* best_at, int32_t* first, int best_in, int device) {
    int ndev = 0;
    ORB_HIPCHK(hipGetDeviceCount(&ndev));
    if (device < 0) ORB_HIPCHK(hipGetDevice(&device));
    OrbHostCtx* C = device < ndev ? orb_internal_thread_ctx(device) : nullptr;
    if (!C) return fail(ORB_EINVAL, "device ordinal out of range");
    ORB_HIPCHK(hipSetDevice(device));
    const int n_hyp = a.n_hyp, W = (n + 63) / 64, cap = std::max(n, 1);
    constexpr int NV = MODEL == PNP ? NV_PNP : NV_SIM3;
    // staging: in  [c0 | c1 | c2 | c3 | HA | HB | best_in]
    //          out [counts | best_at | first, n | masks]      then the SoA scratch (device only)
    size_t o_in[7], off = 0;
    for (int k = 0; k < 6; ++k) {
        o_in[k] = off;
        off = al(off + in_bytes[k]);
    }
    o_in[6] = off;
    const size_t in_end = al(off + 4);
    const size_t oC = in_end, oB = al(oC + (size_t)n_hyp * 4), oF = al(oB + (size_t)n_hyp * 4), oM = al(oF + 8),
                 out_end = al(oM + (size_t)n_hyp * W * 8), total = al(out_end + (size_t)NV * cap * 4);
    if (int r = C->reserve(total, out_end)) return r;
    uint8_t* hp = C->pinned;
    for (int k = 0; k < 6; ++k)
        if (in_bytes[k]) std::memcpy(hp + o_in[k], in[k], in_bytes[k]);
    std::memcpy(hp + o_in[6], &best_in, 4);
    ORB_HIPCHK(hipMemcpyAsync(C->buf, hp, in_end, hipMemcpyHostToDevice, C->stream));
    uint8_t* d = C->buf;
    a.c0 = (const float*)(d + o_in[0]);
    a.c1 = (const float*)(d + o_in[1]);
    a.c2 = (const float*)(d + o_in[2]);
    a.c3 = (const float*)(d + o_in[3]);
    a.n_direct = n;
    a.best_in = (const int32_t*)(d + o_in[6]);
    a.soa = (float*)(d + out_end);
    a.counts = (int32_t*)(d + oC);
    a.best_at = (int32_t*)(d + oB);
    a.first = (int32_t*)(d + oF);
    a.n = a.first + 1;
    a.index = nullptr;
    a.masks = W ? (uint64_t*)(d + oM) : nullptr;
    a.cap = cap;
    a.S = 1;
    a.W = W;
    const int r = launch<MODEL, HT>(a, (const HT*)(d + o_in[4]), (const HT*)(d + o_in[5]), C->stream);
    hipError_t e = hipSuccess;
    if (r == ORB_OK) e = hipMemcpyAsync(hp + oC, d + oC, out_end - oC, hipMemcpyDeviceToHost, C->stream);
    const hipError_t es = hipStreamSynchronize(C->stream);  // the staging is reused by the next call
    if (r) return r;
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(ORB_EDEVICE, std::string("solvers: ") + hipGetErrorString(e));
    if (counts) std::memcpy(counts, hp + oC, (size_t)n_hyp * 4);
    if (best_at) std::memcpy(best_at, hp + oB, (size_t)n_hyp * 4);
    if (first) std::memcpy(first, hp + oF, 4);
    if (masks && W) std::memcpy(masks, hp + oM, (size_t)n_hyp * W * 8);
    return ORB_OK;
}

// The common part of the two batch entry points: scratch, launch, release.
template <int MODEL, class HT>
int run_batch(ConsArgs a, const HT* HA, const HT* HB, hipStream_t st) {
    constexpr int NV = MODEL == PNP ? NV_PNP : NV_SIM3;
    // stream-ordered scratch: the SoA values, then n and counts where the caller does not want them
    const size_t b_soa = al((size_t)a.S * NV * a.cap * 4), b_n = al((size_t)a.S * 4),
                 b_c = al((size_t)a.S * a.n_hyp * 4);
    void* tmp = nullptr;
    hipError_t e = hipMallocAsync(&tmp, b_soa + b_n + b_c, st);
    if (e != hipSuccess) return fail(ORB_ENOMEM, std::string("solvers: scratch: ") + hipGetErrorString(e));
    a.soa = (float*)tmp;
    if (!a.n) a.n = (int32_t*)((uint8_t*)tmp + b_soa);
    if (!a.counts) a.counts = (int32_t*)((uint8_t*)tmp + b_soa + b_n);
    const int r = launch<MODEL, HT>(a, HA, HB, st);
    (void)hipFreeAsync(tmp, st);
    return r;
}

int fill_batch(ConsArgs& a, const char* who, const orb_keypoint_t* d_kps, const int32_t* d_counts, int cap, int S,
               const int32_t* d_pair_a, const int32_t* d_pair_b, const int32_t* d_match, const float* d_mp_pos,
               const uint8_t* d_mp_bad, const float* level_sigma2, int nlevels, int n_hyp, bool sim3) {
    if (S < 0 || cap <= 0) return fail(ORB_EINVAL, std::string(who) + ": bad arguments");
    if (int r = check_limits(who, cap, n_hyp)) return r;
    if (S > 65535) return fail(ORB_ENOTSUP, std::string(who) + ": more than 65535 solvers per call");
    if (!level_sigma2 || nlevels < 1 || nlevels > ORB_MAX_VIEW_LEVELS)
        return fail(ORB_EINVAL, std::string(who) + ": nlevels must be in [1, 16]");
    if (int r = check_sigma2(who, level_sigma2, nlevels, sim3)) return r;
    if (S && (!d_kps || !d_counts || !d_pair_a || !d_pair_b || !d_match || !d_mp_pos))
        return fail(ORB_EINVAL, std::string(who) + ": bad arguments");
    a.kps = d_kps;
    a.kcounts = d_counts;
    a.pair_a = d_pair_a;
    a.pair_b = d_pair_b;
    a.match = d_match;
    a.mp_pos = d_mp_pos;
    a.mp_bad = d_mp_bad;
    a.n_direct = -1;
    std::memcpy(a.level_sigma2, level_sigma2, (size_t)nlevels * 4);
    a.nlevels = nlevels;
    a.cap = cap;
    a.S = S;
    a.n_hyp = n_hyp;
    a.W = (cap + 63) / 64;
    return ORB_OK;
}

}  // namespace

extern "C" {

int orb_pnp_check_inliers(int n, const float* p3d, const float* p2d, const float* sigma2, float th2, double fu,
                          double fv, double uc, double vc, int n_hyp, const double* R, const double* t,
                          int min_inliers, int best_in, int32_t* counts, uint64_t* masks, int32_t* best_at,
                          int32_t* first_ok, int device) {
    if (n < 0 || (n && (!p3d || !p2d || !sigma2))) return fail(ORB_EINVAL, "pnp_check_inliers: bad arguments");
    if (int r = check_limits("pnp_check_inliers", n, n_hyp)) return r;
    if (!R || !t) return fail(ORB_EINVAL, "pnp_check_inliers: no hypotheses given");
    if (int r = check_sigma2("pnp_check_inliers", sigma2, n, false)) return r;
    ConsArgs a{};
    a.th2 = th2;
    a.fu = fu, a.fv = fv, a.uc = uc, a.vc = vc;
    a.n_hyp = n_hyp;
    a.min_inliers = min_inliers;
    const void* in[6] = {p3d, p2d, sigma2, nullptr, R, t};
    const size_t nb[6] = {(size_t)n * 12, (size_t)n * 8, (size_t)n * 4, 0, (size_t)n_hyp * 72, (size_t)n_hyp * 24};
    return run_host<PNP, double>(a, in, nb, n, counts, masks, best_at, first_ok, best_in, device);
}

int orb_sim3_check_inliers(int n, const float* x3dc1, const float* x3dc2, const float* sigma2_1,
                           const float* sigma2_2, const float* K1, const float* K2, int n_hyp, const float* T12,
                           const float* T21, int min_inliers, int best_in, int32_t* counts, uint64_t* masks,
                           int32_t* best_at, int32_t* first_accept, int device) {
    if (n < 0 || (n && (!x3dc1 || !x3dc2 || !sigma2_1 || !sigma2_2)) || !K1 || !K2)
        return fail(ORB_EINVAL, "sim3_check_inliers: bad arguments");
    if (int r = check_limits("sim3_check_inliers", n, n_hyp)) return r;
    if (!T12 || !T21) return fail(ORB_EINVAL, "sim3_check_inliers: no hypotheses given");
    if (int r = check_sigma2("sim3_check_inliers", sigma2_1, n, true)) return r;
    if (int r = check_sigma2("sim3_check_inliers", sigma2_2, n, true)) return r;
    ConsArgs a{};
    std::memcpy(a.K1, K1, 16);
    std::memcpy(a.K2, K2, 16);
    a.n_hyp = n_hyp;
    a.min_inliers = min_inliers;
    const void* in[6] = {x3dc1, x3dc2, sigma2_1, sigma2_2, T12, T21};
    const size_t nb[6] = {(size_t)n * 12, (size_t)n * 12, (size_t)n * 4, (size_t)n * 4, (size_t)n_hyp * 48,
                          (size_t)n_hyp * 48};
    return run_host<SIM3, float>(a, in, nb, n, counts, masks, best_at, first_accept, best_in, device);
}

int orb_pnp_check_inliers_batch_device(const orb_keypoint_t* d_kps, const int32_t* d_counts, int cap, int S,
                                       const int32_t* d_pair_a, const int32_t* d_pair_b, const int32_t* d_match,
                                       const float* d_mp_pos, const uint8_t* d_mp_bad, const float* level_sigma2,
                                       int nlevels, float th2, double fu, double fv, double uc, double vc, int n_hyp,
                                       const double* d_R, const double* d_t, int min_inliers,
                                       const int32_t* d_best_in, int32_t* d_n, int32_t* d_index,
                                       int32_t* d_counts_out, uint64_t* d_masks, int32_t* d_best_at,
                                       int32_t* d_first_ok, void* stream) {
    ConsArgs a{};
    if (int r = fill_batch(a, "pnp_check_inliers_batch", d_kps, d_counts, cap, S, d_pair_a, d_pair_b, d_match,
                           d_mp_pos, d_mp_bad, level_sigma2, nlevels, n_hyp, false))
        return r;
    if (S == 0) return ORB_OK;
    if (!d_R || !d_t) return fail(ORB_EINVAL, "pnp_check_inliers_batch: no hypotheses given");
    a.th2 = th2;
    a.fu = fu, a.fv = fv, a.uc = uc, a.vc = vc;
    a.min_inliers = min_inliers;
    a.best_in = d_best_in;
    a.n = d_n;
    a.index = d_index;
    a.counts = d_counts_out;
    a.masks = d_masks;
    a.best_at = d_best_at;
    a.first = d_first_ok;
    return run_batch<PNP, double>(a, d_R, d_t, (hipStream_t)stream);
}

int orb_sim3_check_inliers_batch_device(const orb_keypoint_t* d_kps, const int32_t* d_counts, int cap, int S,
                                        const int32_t* d_pair_a, const int32_t* d_pair_b, const int32_t* d_match,
                                        const float* d_mp_pos, const uint8_t* d_mp_bad, const float* d_pose,
                                        const float* level_sigma2, int nlevels, const float* K, int n_hyp,
                                        const float* d_T12, const float* d_T21, int min_inliers,
                                        const int32_t* d_best_in, int32_t* d_n, int32_t* d_index,
                                        int32_t* d_counts_out, uint64_t* d_masks, int32_t* d_best_at,
                                        int32_t* d_first_accept, void* stream) {
    ConsArgs a{};
    if (int r = fill_batch(a, "sim3_check_inliers_batch", d_kps, d_counts, cap, S, d_pair_a, d_pair_b, d_match,
                           d_mp_pos, d_mp_bad, level_sigma2, nlevels, n_hyp, true))
        return r;
    if (S == 0) return ORB_OK;
    if (!d_pose || !K) return fail(ORB_EINVAL, "sim3_check_inliers_batch: bad arguments");
    if (!d_T12 || !d_T21) return fail(ORB_EINVAL, "sim3_check_inliers_batch: no hypotheses given");
    a.pose = d_pose;
    std::memcpy(a.K1, K, 16);
    std::memcpy(a.K2, K, 16);
    a.min_inliers = min_inliers;
    a.best_in = d_best_in;
    a.n = d_n;
    a.index = d_index;
    a.counts = d_counts_out;
    a.masks = d_masks;
    a.best_at = d_best_at;
    a.first = d_first_accept;
    return run_batch<SIM3, float>(a, d_T12, d_T21, (hipStream_t)stream);
}

}  // extern "C"
