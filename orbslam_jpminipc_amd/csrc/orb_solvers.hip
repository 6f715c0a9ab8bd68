// orb_solvers.hip — the RANSAC consensus of PnPsolver and Sim3Solver on the GPU (part of liborb_hip.so).
//
// PnPsolver::CheckInliers (reference src/PnPsolver.cc:280-311) and Sim3Solver::CheckInliers
// (src/Sim3Solver.cc:335-359, with Project 377-398) for every hypothesis of a solver at once, the
// per-correspondence set-up of the two constructors (PnPsolver.cc:40-82, 126-128;
// Sim3Solver.cc:37-112) and the keep-the-best rules of the two iterate() loops (PnPsolver.cc:181-196,
// Sim3Solver.cc:183-200).  In the check_inliers entry points the hypotheses are the caller's; in the
// ransac ones they are made here from the caller's rand() values: the minimal sets of
// Sim3Solver::iterate (Sim3Solver.cc:163-177) and Horn's closed form, Sim3Solver::computeT (215-332),
// DESIGN.md §15; the minimal sets of PnPsolver::iterate (PnPsolver.cc:160-173), EPnP's compute_pose
// (449-497, csrc/orb_epnp_math.h) and Refine (232-277), DESIGN.md §17.
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
// d.dot(d) is a double accumulation narrowed to float (these and computeT's are
// csrc/orb_cv_math.h's).  Its bound is the reference's std::vector<size_t> entry:
// (size_t)(9.210 * sigma2), converted to float by the compare.
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
//   k_sim3_hypotheses  one lane per (solver, hypothesis), between prepare and score: the three
//                      draws mapped to indices, the three correspondences gathered from the SoA
//                      scratch, computeT in registers (cv::eigen as JacobiImpl_<float> with every
//                      array index a compile-time constant: no scratch memory), T12 / T21 written.
//   k_sim3_accepted    one workgroup per solver: the Sim3 and mask row of the accepted hypothesis.
//   k_pnp_hypotheses   one lane per (solver, hypothesis), between prepare and score: the four draws
//                      mapped to indices, compute_pose with n = 4, the 12 x 12 work matrix of its
//                      Jacobi SVD in LDS laid out [element][lane]; R / t written as doubles.
//   k_pnp_refine       one workgroup per (solver, iteration that replaced the best): compute_pose on
//                      the correspondences of the iteration's mask (one lane, every sum a single
//                      chain); its poses are scored by k_cons_score<PNP> again.
//   k_pnp_select       one workgroup per solver: the first replacing iteration whose refined count
//                      is > min_inliers, and the pose, mask and count that iterate returns.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <string>

#include "../../include/orb_abi.h"
#include "orb_cv_math.h"
#include "orb_epnp_math.h"
#include "orb_internal.h"

namespace {

int fail(int code, const std::string& msg) { return orb_internal_set_error(code, msg); }

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

// cv::Mat arithmetic on 3-vectors and 3 x 3 matrices: csrc/orb_cv_math.h
using orb_cv::gemm3_add;
using orb_cv::gemm_out;

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

// ---- Sim3Solver: the hypotheses (Sim3Solver.cc:163-177, 215-332) -----------------------
struct HypArgs {
    const int32_t* rand31;  // S x n_hyp x 3 values of rand(), or
    const int32_t* sets;    // S x n_hyp x 3 indices: exactly one of the two
    float* T12;             // outputs, each may be NULL
    float* T21;
    float* sim3;
    float* quat;
    int32_t* sets_out;
};

// The symmetric 4x4 of cv::eigen in registers: U the upper triangle (0,1) (0,2) (0,3) (1,2) (1,3)
// (2,3), W the diagonal, V the eigenvectors as rows, indR / indC JacobiImpl_'s pivot indices.  Every
// array index is a constant after unrolling; a runtime index is a chain of selects.
struct Jac4 {
    float U[6], W[4], V[16];
    int indR[3], indC[4];
};
__host__ __device__ constexpr int jac_up(int i, int j) { return i == 0 ? j - 1 : (i == 1 ? j + 1 : 5); }
// A[r][c], r < c, at a runtime index: the six candidates masked by the index and OR-ed.  (A chain of
// selects over J.U[] is folded by the compiler into one load at a selected address, which keeps U in
// scratch memory.)
__device__ __forceinline__ unsigned jac_pick(int p, int P, float v) { return p == P ? __float_as_uint(v) : 0u; }
__device__ __forceinline__ float jac_get(const Jac4& J, int r, int c) {
    const int p = r == 0 ? c - 1 : (r == 1 ? c + 1 : 5);
    return __uint_as_float(jac_pick(p, 0, J.U[0]) | jac_pick(p, 1, J.U[1]) | jac_pick(p, 2, J.U[2]) |
                           jac_pick(p, 3, J.U[3]) | jac_pick(p, 4, J.U[4]) | jac_pick(p, 5, J.U[5]));
}
// indR[IDX] = the first largest |A[IDX][i]|, i > IDX; indC[IDX] = the first largest |A[i][IDX]|, i < IDX.
// The loops of JacobiImpl_ are written out through templates so that every index is a constant
// before the first scalar-replacement pass: a loop-indexed J.U[] would keep J in scratch memory.
template <int IDX, int I>
__device__ __forceinline__ void jac_scan_row(const Jac4& J, float& mv, int& m) {
    if constexpr (I >= IDX + 2 && I < 4) {
        const float val = fabsf(J.U[jac_up(IDX, I)]);
        if (mv < val) mv = val, m = I;
    }
}
template <int IDX, int I>
__device__ __forceinline__ void jac_scan_col(const Jac4& J, float& mv, int& m) {
    if constexpr (I >= 1 && I < IDX) {
        const float val = fabsf(J.U[jac_up(I, IDX)]);
        if (mv < val) mv = val, m = I;
    }
}
template <int IDX>
__device__ __forceinline__ void jac_scan(Jac4& J) {
    if constexpr (IDX < 3) {
        int m = IDX + 1;
        float mv = fabsf(J.U[jac_up(IDX, IDX + 1)]);
        jac_scan_row<IDX, 2>(J, mv, m);
        jac_scan_row<IDX, 3>(J, mv, m);
        J.indR[IDX] = m;
    }
    if constexpr (IDX > 0) {
        int m = 0;
        float mv = fabsf(J.U[jac_up(0, IDX)]);
        jac_scan_col<IDX, 1>(J, mv, m);
        jac_scan_col<IDX, 2>(J, mv, m);
        J.indC[IDX] = m;
    }
}
__device__ __forceinline__ void jac_rot(float& v0, float& v1, float c, float s) {
    const float a0 = v0, b0 = v1;
    v0 = a0 * c - b0 * s;
    v1 = a0 * s + b0 * c;
}
// rows and columns K and L at index I (i < k, k < i < l, l < i in JacobiImpl_'s three loops)
template <int K, int L, int I>
__device__ __forceinline__ void jac_rot_at(Jac4& J, float c, float s) {
    if constexpr (I < K) jac_rot(J.U[jac_up(I, K)], J.U[jac_up(I, L)], c, s);
    else if constexpr (I > K && I < L) jac_rot(J.U[jac_up(K, I)], J.U[jac_up(I, L)], c, s);
    else if constexpr (I > L) jac_rot(J.U[jac_up(K, I)], J.U[jac_up(L, I)], c, s);
}
// one rotation on the pivot p = A[K][L]
template <int K, int L>
__device__ __forceinline__ void jac_rotate(Jac4& J, float p) {
    const float y = (float)((double)(J.W[L] - J.W[K]) * 0.5);
    float t = fabsf(y) + orb_cv::cv_hypot(p, y);  // lapack.cpp's own hypot, in float
    float s = orb_cv::cv_hypot(p, t);
    const float c = t / s;
    s = p / s;
    t = (p / t) * p;
    if (y < 0) s = -s, t = -t;
    J.U[jac_up(K, L)] = 0;
    J.W[K] -= t;
    J.W[L] += t;
    jac_rot_at<K, L, 0>(J, c, s);
    jac_rot_at<K, L, 1>(J, c, s);
    jac_rot_at<K, L, 2>(J, c, s);
    jac_rot_at<K, L, 3>(J, c, s);
    jac_rot(J.V[4 * K], J.V[4 * L], c, s);
    jac_rot(J.V[4 * K + 1], J.V[4 * L + 1], c, s);
    jac_rot(J.V[4 * K + 2], J.V[4 * L + 2], c, s);
    jac_rot(J.V[4 * K + 3], J.V[4 * L + 3], c, s);
    jac_scan<K>(J);
    jac_scan<L>(J);
}
__device__ __forceinline__ float sel4(int m, float v0, float v1, float v2, float v3) {
    float v = v0;
    v = m == 1 ? v1 : v;
    v = m == 2 ? v2 : v;
    v = m == 3 ? v3 : v;
    return v;
}
// the second half of the pivot search: column I's largest entry against the best so far
template <int I>
__device__ __forceinline__ void jac_pivot_col(const Jac4& J, float& mv, int& k, int& l) {
    const float val = fabsf(jac_get(J, J.indC[I], I));
    if (mv < val) mv = val, k = J.indC[I], l = I;
}

// cv::eigen(N, eval, evec) of the symmetric 4x4 CV_32F whose upper triangle and diagonal are in J:
// q = row 0 of evec.  The descending sort swaps rows 0 and m, the first largest eigenvalue; the later
// swaps leave row 0 alone, so row 0 is row m before the sort.
__device__ __forceinline__ void jac_eigen_row0(Jac4& J, float* q) {
    J.V[0] = 1, J.V[1] = 0, J.V[2] = 0, J.V[3] = 0;
    J.V[4] = 0, J.V[5] = 1, J.V[6] = 0, J.V[7] = 0;
    J.V[8] = 0, J.V[9] = 0, J.V[10] = 1, J.V[11] = 0;
    J.V[12] = 0, J.V[13] = 0, J.V[14] = 0, J.V[15] = 1;
    J.indC[0] = 0;
    jac_scan<0>(J);
    jac_scan<1>(J);
    jac_scan<2>(J);
    jac_scan<3>(J);
    for (int iters = 0; iters < 4 * 4 * 30; ++iters) {
        int k = 0;
        float mv = fabsf(jac_get(J, 0, J.indR[0]));
        float val = fabsf(jac_get(J, 1, J.indR[1]));
        if (mv < val) mv = val, k = 1;
        val = fabsf(J.U[5]);  // indR[2] is 3
        if (mv < val) mv = val, k = 2;
        int l = k == 0 ? J.indR[0] : (k == 1 ? J.indR[1] : 3);
        jac_pivot_col<1>(J, mv, k, l);
        jac_pivot_col<2>(J, mv, k, l);
        jac_pivot_col<3>(J, mv, k, l);
        const float p = jac_get(J, k, l);
        if (fabsf(p) <= 1.1920928955078125e-7f) break;  // FLT_EPSILON
        switch (4 * k + l) {
            case 1: jac_rotate<0, 1>(J, p); break;
            case 2: jac_rotate<0, 2>(J, p); break;
            case 3: jac_rotate<0, 3>(J, p); break;
            case 6: jac_rotate<1, 2>(J, p); break;
            case 7: jac_rotate<1, 3>(J, p); break;
            default: jac_rotate<2, 3>(J, p); break;
        }
    }
    int m = 0;
    float wm = J.W[0];
    if (wm < J.W[1]) wm = J.W[1], m = 1;
    if (wm < J.W[2]) wm = J.W[2], m = 2;
    if (wm < J.W[3]) wm = J.W[3], m = 3;
    q[0] = sel4(m, J.V[0], J.V[4], J.V[8], J.V[12]);
    q[1] = sel4(m, J.V[1], J.V[5], J.V[9], J.V[13]);
    q[2] = sel4(m, J.V[2], J.V[6], J.V[10], J.V[14]);
    q[3] = sel4(m, J.V[3], J.V[7], J.V[11], J.V[15]);
}

// Sim3Solver::centroid of a 3x3 (row-major, a correspondence per column)
__device__ __forceinline__ void centroid3(const float* P, float* Pr, float* C) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        float a0 = P[3 * r], a1 = P[3 * r + 1];  // cv::reduce: (s0 + s2) + s1
        a0 = a0 + P[3 * r + 2];
        a0 = a0 + a1;
        C[r] = orb_cv::scale(a0, 1. / (double)3);
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) Pr[k] = P[k] - C[k / 3];
}
// (DUtils::Random::RandomInt and the minimal sets of both solvers: orb_epnp::minimal_set<K>)

// One lane per (solver, hypothesis), after k_cons_prepare<SIM3>.
__global__ void __launch_bounds__(64) k_sim3_hypotheses(ConsArgs a, HypArgs y) {
    const int s = blockIdx.y, h = blockIdx.x * 64 + threadIdx.x;
    if (h >= a.n_hyp) return;
    const size_t g = (size_t)s * a.n_hyp + h;
    const int n = a.n[s], cap = a.cap;
    float T12[12], T21[12], R[9], t12[3], q[4], ms12i = 0;
    int idx[3] = {0, 0, 0};
#pragma unroll
    for (int k = 0; k < 12; ++k) T12[k] = T21[k] = 0;
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = 0;
    t12[0] = t12[1] = t12[2] = q[0] = q[1] = q[2] = q[3] = 0;
    // N < mRansacMinInliers: bNoMore, nothing is generated (Sim3Solver.cc:146-150); n >= 3 otherwise
    if (n >= a.min_inliers && n >= (y.sets ? 1 : 3)) {
        if (y.sets) {
#pragma unroll
            for (int i = 0; i < 3; ++i) idx[i] = min(max(y.sets[3 * g + i], 0), n - 1);
        } else {
            // vAvailableIndices, [idx] = back(), pop_back() with idx the value drawn (Sim3Solver.cc:175-176):
            // the mapping PnPsolver shares
            orb_epnp::minimal_set<3>(y.rand31 + 3 * g, n, idx);
        }
        const float* x = a.soa + (size_t)s * NV_SIM3 * cap;
        float P1[9], P2[9], Pr1[9], Pr2[9], O1[3], O2[3];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                P1[3 * r + i] = x[(size_t)r * cap + idx[i]];
                P2[3 * r + i] = x[(size_t)(3 + r) * cap + idx[i]];
            }
        centroid3(P1, Pr1, O1);
        centroid3(P2, Pr2, O2);
        // M = Pr2*Pr1.t() (GEMM_2_T: GEMMSingleMul<float, double>)
        const orb_cv::M3 Mm = orb_cv::gemm3<false, true>(orb_cv::load3x3(Pr2), orb_cv::load3x3(Pr1), 1.0);
        const float* M = Mm.m;
        Jac4 J;
        J.W[0] = M[0] + M[4] + M[8];    // N11
        J.U[0] = M[5] - M[7];           // N12
        J.U[1] = M[6] - M[2];           // N13
        J.U[2] = M[1] - M[3];           // N14
        J.W[1] = M[0] - M[4] - M[8];    // N22
        J.U[3] = M[1] + M[3];           // N23
        J.U[4] = M[6] + M[2];           // N24
        J.W[2] = -M[0] + M[4] - M[8];   // N33
        J.U[5] = M[5] + M[7];           // N34
        J.W[3] = -M[0] - M[4] + M[8];   // N44
        jac_eigen_row0(J, q);
        float vec[3] = {q[1], q[2], q[3]};
        const double nrm = orb_cv::norm3(vec);
        const double ang = atan2(nrm, (double)q[0]);
        orb_cv::scale3(vec, (2 * ang) * (1. / nrm), vec);  // 2*ang*vec/norm(vec)
        {  // cvRodrigues2
            double rx = vec[0], ry = vec[1], rz = vec[2];
            const double theta = sqrt(rx * rx + ry * ry + rz * rz);
            if (theta < 2.2204460492503131e-16) {  // DBL_EPSILON
#pragma unroll
                for (int k = 0; k < 9; ++k) R[k] = k % 4 == 0 ? 1.0f : 0.0f;
            } else {
                const double c = cos(theta), sn = sin(theta), c1 = 1. - c;
                const double itheta = theta ? 1. / theta : 0.;
                rx *= itheta, ry *= itheta, rz *= itheta;
                const double rrt[9] = {rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz};
                const double r_x[9] = {0, -rz, ry, rz, 0, -rx, -ry, rx, 0};
#pragma unroll
                for (int k = 0; k < 9; ++k) R[k] = (float)(c * (k % 4 == 0 ? 1.0 : 0.0) + c1 * rrt[k] + sn * r_x[k]);
            }
        }
        // P3 = mR12i*Pr2, nom = Pr1.dot(P3) (unrolled by 4), den = the double sum of P3's float squares
        float P3[9];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const float t = R[3 * i] * Pr2[j] + R[3 * i + 1] * Pr2[3 + j] + R[3 * i + 2] * Pr2[6 + j];
                P3[3 * i + j] = gemm_out(t, 1.0, 0.0f, 0.0);
            }
        double nom = 0;
        nom += (double)Pr1[0] * P3[0] + (double)Pr1[1] * P3[1] + (double)Pr1[2] * P3[2] + (double)Pr1[3] * P3[3];
        nom += (double)Pr1[4] * P3[4] + (double)Pr1[5] * P3[5] + (double)Pr1[6] * P3[6] + (double)Pr1[7] * P3[7];
        nom += (double)Pr1[8] * P3[8];
        double den = 0;
#pragma unroll
        for (int k = 0; k < 9; ++k) den += (double)(P3[k] * P3[k]);
        ms12i = (float)(nom / den);
        // mt12i = O1 - ms12i*mR12i*O2: one gemm, alpha = -ms12i, C = O1, beta = 1
        gemm3_add(R, 3, O1, 1, O2[0], O2[1], O2[2], t12, -(double)ms12i, 1.0);
        // sR = ms12i*mR12i; sRinv = (1.0/ms12i)*mR12i.t(); tinv = -sRinv*mt12i
        const double inv_s = 1.0 / (double)ms12i;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                T12[4 * i + j] = orb_cv::scale(R[3 * i + j], (double)ms12i);
                T21[4 * i + j] = orb_cv::scale(R[3 * j + i], inv_s);
            }
            T12[4 * i + 3] = t12[i];
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const float t = T21[4 * i] * t12[0] + T21[4 * i + 1] * t12[1] + T21[4 * i + 2] * t12[2];
            T21[4 * i + 3] = gemm_out(t, -1.0, 0.0f, 0.0);
        }
    }
    if (y.T12) {
#pragma unroll
        for (int k = 0; k < 12; ++k) y.T12[g * 12 + k] = T12[k];
    }
    if (y.T21) {
#pragma unroll
        for (int k = 0; k < 12; ++k) y.T21[g * 12 + k] = T21[k];
    }
    if (y.sim3) {
#pragma unroll
        for (int k = 0; k < 9; ++k) y.sim3[g * 13 + k] = R[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) y.sim3[g * 13 + 9 + k] = t12[k];
        y.sim3[g * 13 + 12] = ms12i;
    }
    if (y.quat) {
#pragma unroll
        for (int k = 0; k < 4; ++k) y.quat[g * 4 + k] = q[k];
    }
    if (y.sets_out) {
#pragma unroll
        for (int k = 0; k < 3; ++k) y.sets_out[g * 3 + k] = idx[k];
    }
}

// What iterate returns per solver: the Sim3 (13 floats) and the mask row of hypothesis first_accept,
// or of best_at[n_hyp - 1] (mBestT12) when nothing was accepted; NaN and a zero row when the best is
// still the earlier calls' (best_at < 0).
__global__ void __launch_bounds__(64) k_sim3_accepted(ConsArgs a, const float* sim3, float* accepted,
                                                      uint64_t* accepted_mask) {
    const int s = blockIdx.x, tid = threadIdx.x;
    const int f = a.first[s];
    const int h = f >= 0 ? f : a.best_at[(size_t)s * a.n_hyp + a.n_hyp - 1];
    if (accepted && tid < 13)
        accepted[(size_t)s * 13 + tid] = h >= 0 ? sim3[((size_t)s * a.n_hyp + h) * 13 + tid] : __builtin_nanf("");
    if (accepted_mask)
        for (int w = tid; w < a.W; w += 64)
            accepted_mask[(size_t)s * a.W + w] = h >= 0 ? a.masks[((size_t)s * a.n_hyp + h) * a.W + w] : 0ull;
}

// ---- PnPsolver: the hypotheses and Refine (PnPsolver.cc:137-277, 314-922) ----------------
constexpr int PNP_LDS = orb_epnp::WK_DOUBLES * 64 * 8;  // 79 872 bytes: [element][lane], two workgroups per CU

struct PnpArgs {
    const int32_t* rand31;  // S x n_hyp x 4 values of rand(), or
    const int32_t* sets;    // S x n_hyp x 4 indices: exactly one of the two
    double* R;              // S x n_hyp x 9, S x n_hyp x 3: the score kernel's input
    double* t;
    double* rep;            // may be NULL
    int32_t* sets_out;      // may be NULL
    // Refine and the result of the call
    double* rR;
    double* rt;
    int32_t* rcounts;
    uint64_t* rmasks;
    const int32_t* sel;     // the stand-alone n-point pose: n_sel indices in place of a mask row
    int n_sel;
    int32_t* first_refined;
    float* pose;
    uint64_t* pose_mask;
    int32_t* pose_inliers;
};

// The four correspondences of a minimal set, and alphas / pcs, in the lane's registers.
struct Pts4 {
    static constexpr bool STORED = true;
    double pws[12], us[8], al[16], pcs[12];
    __device__ __forceinline__ int size() const { return 4; }
    __device__ __forceinline__ double pw(int i, int j) const { return pws[3 * i + j]; }
    __device__ __forceinline__ double u(int i, int j) const { return us[2 * i + j]; }
    __device__ __forceinline__ double& alpha(int i, int c) { return al[4 * i + c]; }
    __device__ __forceinline__ double& pc(int i, int j) { return pcs[3 * i + j]; }
};

// The n correspondences of an index list, read from the SoA scratch where they are used; alphas and
// pcs are recomputed where they are read (no per-correspondence storage).
struct PtsList {
    static constexpr bool STORED = false;
    const float* q;
    int cap, n;
    const uint16_t* list;
    __device__ __forceinline__ int size() const { return n; }
    __device__ __forceinline__ double pw(int i, int j) const { return (double)q[(size_t)j * cap + list[i]]; }
    __device__ __forceinline__ double u(int i, int j) const { return (double)q[(size_t)(3 + j) * cap + list[i]]; }
};

// One lane per (solver, hypothesis), after k_cons_prepare<PNP>: the set from the draws, compute_pose
// with n = 4, the 12 x 12 and the small decompositions' work arrays in the lane's column of LDS.
__global__ void __launch_bounds__(64) k_pnp_hypotheses(ConsArgs a, PnpArgs y) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int s = blockIdx.y, h = blockIdx.x * 64 + threadIdx.x;
    if (h >= a.n_hyp) return;
    const size_t g = (size_t)s * a.n_hyp + h;
    const int n = a.n[s], cap = a.cap;
    double R[9], t[3], rep = 0;
    int idx[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = 0;
    t[0] = t[1] = t[2] = 0;
    // N < mRansacMinInliers: bNoMore, nothing is generated (PnPsolver.cc:145-149); n >= 4 otherwise
    if (n >= a.min_inliers && n >= (y.sets ? 1 : 4)) {
        if (y.sets) {
#pragma unroll
            for (int i = 0; i < 4; ++i) idx[i] = min(max(y.sets[4 * g + i], 0), n - 1);
        } else
            orb_epnp::minimal_set<4>(y.rand31 + 4 * g, n, idx);
        orb_epnp::Epnp<orb_epnp::Mat<64>, Pts4> e;
        e.wk = orb_epnp::Mat<64>{(double*)smem + threadIdx.x};
        const float* q = a.soa + (size_t)s * NV_PNP * cap;
#pragma unroll
        for (int i = 0; i < 4; ++i) {  // add_correspondence: float to double
#pragma unroll
            for (int j = 0; j < 3; ++j) e.pt.pws[3 * i + j] = (double)q[(size_t)j * cap + idx[i]];
            e.pt.us[2 * i] = (double)q[(size_t)3 * cap + idx[i]];
            e.pt.us[2 * i + 1] = (double)q[(size_t)4 * cap + idx[i]];
        }
        e.fu = a.fu, e.fv = a.fv, e.uc = a.uc, e.vc = a.vc;
        e.br = 0;
        rep = orb_epnp::compute_pose(e, R, t);
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) y.R[g * 9 + k] = R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) y.t[g * 3 + k] = t[k];
    if (y.rep) y.rep[g] = rep;
    if (y.sets_out) {
#pragma unroll
        for (int k = 0; k < 4; ++k) y.sets_out[g * 4 + k] = idx[k];
    }
}

// Refine's compute_pose (PnPsolver.cc:234-256), one workgroup per (solver, iteration): only the
// iterations that replaced the best have a new mask to refine (best_at[h] == h), the
// others leave a NaN pose and a count of -1.  Lane 0 runs compute_pose on the correspondences of the
// iteration's mask in index order; every sum over them is the single chain of the reference.  With
// y.sel the list is given instead (the stand-alone n-point pose).
__global__ void __launch_bounds__(64) k_pnp_refine(ConsArgs a, PnpArgs y) {
    __shared__ uint16_t s_list[CS_MAX_CAP];
    __shared__ double s_wk[orb_epnp::WK_DOUBLES];
    __shared__ int s_n;
    const int s = blockIdx.y, h = blockIdx.x, tid = threadIdx.x;
    const size_t g = (size_t)s * a.n_hyp + h;
    const bool live = y.sel || a.best_at[g] == h;
    if (tid == 0 && y.rcounts) y.rcounts[g] = live ? 0 : -1;
    if (!live) {
        if (tid < 9) y.rR[g * 9 + tid] = __builtin_nan("");
        if (tid < 3) y.rt[g * 3 + tid] = __builtin_nan("");
        return;
    }
    if (y.sel) {
        for (int i = tid; i < y.n_sel; i += 64) s_list[i] = (uint16_t)y.sel[i];
        if (tid == 0) s_n = y.n_sel;
    } else if (tid == 0) {
        int k = 0;
        for (int w = 0; w < a.W; ++w) {
            unsigned long long bits = a.masks[g * a.W + w];  // only bits below n are ever set
            while (bits) {
                s_list[k++] = (uint16_t)(w * 64 + __builtin_ctzll(bits));
                bits &= bits - 1;
            }
        }
        s_n = k;
    }
    __syncthreads();
    if (tid != 0) return;
    orb_epnp::Epnp<orb_epnp::Mat<1>, PtsList> e;
    e.wk = orb_epnp::Mat<1>{s_wk};
    e.pt.q = a.soa + (size_t)s * NV_PNP * a.cap;
    e.pt.cap = a.cap;
    e.pt.n = s_n;
    e.pt.list = s_list;
    e.fu = a.fu, e.fv = a.fv, e.uc = a.uc, e.vc = a.vc;
    e.br = 0;
    double R[9], t[3];
    const double rep = orb_epnp::compute_pose(e, R, t);
    for (int k = 0; k < 9; ++k) y.rR[g * 9 + k] = R[k];
    for (int k = 0; k < 3; ++k) y.rt[g * 3 + k] = t[k];
    if (y.rep && y.sel) y.rep[g] = rep;
}

// What iterate returns per solver: the refined pose, mask and count of the first replacing iteration
// whose Refine counted more than min_inliers (PnPsolver.cc:198-208, 264), else the best ones
// (213-226); NaN and a zero row when there is nothing, or when the best is still the earlier calls'.
// The pose is Rcw row-major then tcw, double narrowed to float (mBestTcw / mRefinedTcw).
__global__ void __launch_bounds__(64) k_pnp_select(ConsArgs a, PnpArgs y) {
    __shared__ int s_f;
    const int s = blockIdx.x, tid = threadIdx.x;
    const size_t g0 = (size_t)s * a.n_hyp;
    if (tid == 0) s_f = INT_MAX;
    __syncthreads();
    for (int h = tid; h < a.n_hyp; h += 64)
        if (a.best_at[g0 + h] == h && y.rcounts[g0 + h] > a.min_inliers) atomicMin(&s_f, h);
    __syncthreads();
    const int f = s_f == INT_MAX ? -1 : s_f;
    const int hb = a.best_at[g0 + a.n_hyp - 1];
    const int best_in = a.best_in ? a.best_in[s] : 0;
    if (tid == 0) {
        if (y.first_refined) y.first_refined[s] = f;
        if (y.pose_inliers)
            y.pose_inliers[s] = f >= 0 ? y.rcounts[g0 + f]
                                       : (hb >= 0 ? a.counts[g0 + hb] : (hb == -2 && best_in >= a.min_inliers ? best_in : 0));
    }
    if (y.pose && tid < 12) {
        const double* Rs = f >= 0 ? y.rR + (g0 + f) * 9 : (hb >= 0 ? y.R + (g0 + hb) * 9 : nullptr);
        const double* ts = f >= 0 ? y.rt + (g0 + f) * 3 : (hb >= 0 ? y.t + (g0 + hb) * 3 : nullptr);
        y.pose[(size_t)s * 12 + tid] = Rs ? (float)(tid < 9 ? Rs[tid] : ts[tid - 9]) : __builtin_nanf("");
    }
    if (y.pose_mask)
        for (int w = tid; w < a.W; w += 64)
            y.pose_mask[(size_t)s * a.W + w] =
                f >= 0 ? y.rmasks[(g0 + f) * a.W + w] : (hb >= 0 ? a.masks[(g0 + hb) * a.W + w] : 0ull);
}

template <int MODEL, class HT>
int launch(const ConsArgs& a, const HT* HA, const HT* HB, hipStream_t st, const HypArgs* hyp = nullptr) {
    hipLaunchKernelGGL((k_cons_prepare<MODEL>), dim3(a.S), dim3(CS_PREP_THREADS), 0, st, a);
    ORB_HIPCHK(hipGetLastError());
    if (hyp) {
        hipLaunchKernelGGL(k_sim3_hypotheses, dim3((a.n_hyp + 63) / 64, a.S), dim3(64), 0, st, a, *hyp);
        ORB_HIPCHK(hipGetLastError());
    }
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

// What the consensus reads and writes in every host form: best_in, declared as the last input, and
// counts | best_at | first, n as the first outputs.  The masks (`rM`, n_hyp x W words) and the SoA
// scratch are declared by the caller, after its own outputs.
struct ConsStage {
    OrbRegion<int32_t> best_in, counts, best_at, first_n;
    ConsStage(OrbStagePlan& P, size_t nh)
        : best_in(P.in<int32_t>(1)), counts(P.out<int32_t>(nh)), best_at(P.out<int32_t>(nh)), first_n(P.out<int32_t>(2)) {}
    void args(const OrbHostCall& c, ConsArgs& a, int n, int best, OrbRegion<uint64_t> rM, OrbRegion<float> rSoa) const {
        a.n_direct = n;
        a.best_in = c.send(best_in, &best);
        a.soa = c.dev(rSoa);
        a.counts = c.dev(counts);
        a.best_at = c.dev(best_at);
        a.first = c.dev(first_n);
        a.n = a.first + 1;
        a.index = nullptr;
        a.W = (n + 63) / 64;
        a.masks = a.W ? c.dev(rM) : nullptr;  // no pointer to an empty region
        a.cap = std::max(n, 1);
        a.S = 1;
    }
    void results(const OrbHostCall& c, OrbRegion<uint64_t> rM, int32_t* counts_out, int32_t* best_at_out, int32_t* first,
                 uint64_t* masks) const {
        c.get(counts, counts_out);
        c.get(best_at, best_at_out);
        c.get(first_n, first, 1);
        c.get(rM, masks);
    }
};

// One solver from compact host arrays: the common part of the two host entry points.  in[k]: the
// k-th input array with in_bytes[k] bytes (4 correspondence arrays, then the 2 hypothesis arrays).
template <int MODEL, class HT>
int run_host(ConsArgs a, const void* const* in, const size_t* in_bytes, int n, int32_t* counts, uint64_t* masks,
             int32_t* best_at, int32_t* first, int best_in, int device) {
    const int n_hyp = a.n_hyp, W = (n + 63) / 64, cap = std::max(n, 1);
    const size_t nh = (size_t)n_hyp;
    constexpr int NV = MODEL == PNP ? NV_PNP : NV_SIM3;
    OrbStagePlan P;
    OrbRegion<uint8_t> rIn[6];
    for (int k = 0; k < 6; ++k) rIn[k] = P.in<uint8_t>(in_bytes[k]);
    const ConsStage cs(P, nh);
    const auto rM = P.out<uint64_t>(nh * W);
    const auto rSoa = P.scratch<float>((size_t)NV * cap);
    OrbHostCall call(P, device);
    if (call.err) return call.err;
    const void* d_in[6];
    for (int k = 0; k < 6; ++k) d_in[k] = call.send(rIn[k], (const uint8_t*)in[k]);
    a.c0 = (const float*)d_in[0];
    a.c1 = (const float*)d_in[1];
    a.c2 = (const float*)d_in[2];
    a.c3 = (const float*)d_in[3];
    cs.args(call, a, n, best_in, rM, rSoa);
    if (int r = call.upload()) return r;
    const int r = launch<MODEL, HT>(a, (const HT*)d_in[4], (const HT*)d_in[5], call.stream());
    if (int rf = call.finish(r, hipSuccess, "solvers: ")) return rf;
    cs.results(call, rM, counts, best_at, first, masks);
    return ORB_OK;
}

// The common part of the two batch entry points: scratch, launch, release.
template <int MODEL, class HT>
int run_batch(ConsArgs a, const HT* HA, const HT* HB, hipStream_t st) {
    constexpr int NV = MODEL == PNP ? NV_PNP : NV_SIM3;
    // stream-ordered scratch: the SoA values, then n and counts where the caller does not want them
    int32_t *const d_n = a.n, *const d_counts = a.counts;
    void* tmp = nullptr;
    if (int r = orb_scratch_alloc(&tmp, st, "solvers: scratch: ", [&](OrbLayout& L) {
            a.soa = L.take<float>((size_t)a.S * NV * a.cap);
            a.n = L.given_or_take(d_n, (size_t)a.S);
            a.counts = L.given_or_take(d_counts, (size_t)a.S * a.n_hyp);
        }))
        return r;
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

// Exactly one of sets / rand31 (n_hyp x K), every value in range (the host forms).  PnP (K = 4) takes
// n = 0 and then leaves the sets unread; Sim3 (K = 3) refuses every set of an empty problem.
int check_draws(const char* who, int K, int n, int n_hyp, const int32_t* sets, const int32_t* rand31) {
    if ((sets != nullptr) == (rand31 != nullptr))
        return fail(ORB_EINVAL, std::string(who) + ": exactly one of sets and rand31 must be given");
    const int32_t* v = sets ? sets : rand31;
    for (size_t k = 0; k < (size_t)n_hyp * K; ++k) {
        if (sets && (K == 3 || n > 0) && (v[k] < 0 || v[k] >= n))
            return fail(ORB_EINVAL, std::string(who) + ": sets[" + std::to_string(k) + "] = " + std::to_string(v[k]) +
                                        " is outside [0, n)");
        if (rand31 && v[k] < 0)
            return fail(ORB_EINVAL, std::string(who) + ": rand31[" + std::to_string(k) + "] = " + std::to_string(v[k]) +
                                        " is outside [0, 2^31)");
    }
    return ORB_OK;
}

// A consensus below the size K of a minimal set accepts hypotheses that nothing supports.
int check_min_inliers(const char* who, int K, int min_inliers) {
    if (min_inliers < K)
        return fail(ORB_EINVAL, std::string(who) + ": min_inliers must be at least " + std::to_string(K) +
                                    ", the size of a minimal set (got " + std::to_string(min_inliers) + ")");
    return ORB_OK;
}

struct HypHost {  // the host outputs of the generation, each may be NULL
    float* T12;
    float* T21;
    float* sim3;
    float* quat;
    int32_t* sets_out;
    float* accepted;
};

// One Sim3Solver from compact host arrays: the hypotheses and, with `score`, the consensus on them in
// one stream-ordered chain.  Without `score` the sigma2 arrays may be NULL (zeros are staged).
int run_host_sim3(ConsArgs a, bool score, int n, const float* x1, const float* x2, const float* s1, const float* s2,
                  const int32_t* sets, const int32_t* rand31, const HypHost& o, int32_t* counts, uint64_t* masks,
                  int32_t* best_at, int32_t* first, int best_in, int device) {
    const int n_hyp = a.n_hyp, W = (n + 63) / 64, cap = std::max(n, 1);
    const size_t N = (size_t)n, nh = (size_t)n_hyp;
    OrbStagePlan P;
    const auto r1 = P.in<float>(N * 3), r2 = P.in<float>(N * 3), r3 = P.in<float>(N), r4 = P.in<float>(N);
    const auto rD = P.in<int32_t>(nh * 3);
    const ConsStage cs(P, nh);
    const auto rT12 = P.out<float>(nh * 12), rT21 = P.out<float>(nh * 12), rS = P.out<float>(nh * 13),
               rQ = P.out<float>(nh * 4);
    const auto rSet = P.out<int32_t>(nh * 3);
    const auto rA = P.out<float>(13);
    const auto rM = P.out<uint64_t>(nh * W);
    const auto rSoa = P.scratch<float>((size_t)NV_SIM3 * cap);
    OrbHostCall call(P, device);
    if (call.err) return call.err;
    a.c0 = call.send(r1, x1);
    a.c1 = call.send(r2, x2);
    a.c2 = call.send(r3, s1);
    a.c3 = call.send(r4, s2);
    cs.args(call, a, n, best_in, rM, rSoa);
    HypArgs y{};
    (sets ? y.sets : y.rand31) = call.send(rD, sets ? sets : rand31);
    y.T12 = call.dev(rT12);
    y.T21 = call.dev(rT21);
    y.sim3 = call.dev(rS);
    y.quat = call.dev(rQ);
    y.sets_out = call.dev(rSet);
    if (int r = call.upload()) return r;
    int r = ORB_OK;
    hipError_t e = hipSuccess;
    if (score) {
        r = launch<SIM3, float>(a, y.T12, y.T21, call.stream(), &y);
        if (r == ORB_OK) {
            hipLaunchKernelGGL(k_sim3_accepted, dim3(1), dim3(64), 0, call.stream(), a, y.sim3, call.dev(rA),
                               (uint64_t*)nullptr);
            e = hipGetLastError();
        }
    } else {
        hipLaunchKernelGGL((k_cons_prepare<SIM3>), dim3(1), dim3(CS_PREP_THREADS), 0, call.stream(), a);
        e = hipGetLastError();
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_sim3_hypotheses, dim3((n_hyp + 63) / 64, 1), dim3(64), 0, call.stream(), a, y);
            e = hipGetLastError();
        }
    }
    if (int rf = call.finish(r, e, "solvers: ")) return rf;
    if (score) {
        cs.results(call, rM, counts, best_at, first, masks);
        call.get(rA, o.accepted);
    }
    call.get(rT12, o.T12);
    call.get(rT21, o.T21);
    call.get(rS, o.sim3);
    call.get(rQ, o.quat);
    call.get(rSet, o.sets_out);
    return ORB_OK;
}

// The PnP chain on a filled ConsArgs / PnpArgs: prepare, hypotheses and, with `score`, the consensus on
// them, Refine at the replacing iterations, the consensus on the refined poses and the result.
int launch_pnp(const ConsArgs& a, const PnpArgs& y, bool score, hipStream_t st) {
    hipError_t e = hipFuncSetAttribute((const void*)k_pnp_hypotheses, hipFuncAttributeMaxDynamicSharedMemorySize, PNP_LDS);
    if (e != hipSuccess) return fail(ORB_EDEVICE, std::string("solvers: ") + hipGetErrorString(e));
    hipLaunchKernelGGL((k_cons_prepare<PNP>), dim3(a.S), dim3(CS_PREP_THREADS), 0, st, a);
    ORB_HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_pnp_hypotheses, dim3((a.n_hyp + 63) / 64, a.S), dim3(64), PNP_LDS, st, a, y);
    ORB_HIPCHK(hipGetLastError());
    if (!score) return ORB_OK;
    const dim3 sg(a.S, (a.n_hyp + CS_TILE - 1) / CS_TILE, (std::max(a.W, 1) + CS_WAVES - 1) / CS_WAVES);
    hipLaunchKernelGGL((k_cons_score<PNP, double>), sg, dim3(CS_THREADS), 0, st, a, (const double*)y.R, (const double*)y.t);
    ORB_HIPCHK(hipGetLastError());
    hipLaunchKernelGGL((k_cons_select<PNP>), dim3(a.S), dim3(CS_SEL_THREADS), 0, st, a);
    ORB_HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_pnp_refine, dim3(a.n_hyp, a.S), dim3(64), 0, st, a, y);
    ORB_HIPCHK(hipGetLastError());
    ConsArgs b = a;
    b.counts = y.rcounts;
    b.masks = y.rmasks;
    hipLaunchKernelGGL((k_cons_score<PNP, double>), sg, dim3(CS_THREADS), 0, st, b, (const double*)y.rR, (const double*)y.rt);
    ORB_HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_pnp_select, dim3(a.S), dim3(64), 0, st, a, y);
    ORB_HIPCHK(hipGetLastError());
    return ORB_OK;
}

struct PnpHost {  // the host outputs, each may be NULL
    double* R;
    double* t;
    double* rep;
    int32_t* sets_out;
    int32_t* refined_counts;
    int32_t* first_refined;
    float* pose;
    uint64_t* pose_mask;
    int32_t* pose_inliers;
};

enum { PNP_HYP = 0, PNP_RANSAC = 1, PNP_POSE_N = 2 };

// One PnPsolver from compact host arrays in one stream-ordered chain: the hypotheses (PNP_HYP), the
// whole iterate (PNP_RANSAC) or compute_pose on the n_sel correspondences `sel` (PNP_POSE_N, n_hyp = 1).
// Without the consensus sigma2 may be NULL (zeros are staged).
int run_host_pnp(ConsArgs a, int mode, int n, const float* p3d, const float* p2d, const float* sigma2,
                 const int32_t* sets, const int32_t* rand31, const int32_t* sel, int n_sel, const PnpHost& o,
                 int32_t* counts, uint64_t* masks, int32_t* best_at, int32_t* first, int best_in, int device) {
    const int n_hyp = a.n_hyp, W = (n + 63) / 64, cap = std::max(n, 1);
    const size_t N = (size_t)n, nh = (size_t)n_hyp;
    OrbStagePlan P;
    const auto r1 = P.in<float>(N * 3), r2 = P.in<float>(N * 2), r3 = P.in<float>(N);
    const auto rD = P.in<int32_t>(nh * 4), rL = P.in<int32_t>(n_sel);
    const ConsStage cs(P, nh);
    const auto rR = P.out<double>(nh * 9), rT = P.out<double>(nh * 3), rE = P.out<double>(nh);
    const auto rSet = P.out<int32_t>(nh * 4), rRC = P.out<int32_t>(nh), rFR = P.out<int32_t>(2);  // first_refined, inliers
    const auto rP = P.out<float>(12);
    const auto rPM = P.out<uint64_t>(W), rM = P.out<uint64_t>(nh * W);
    const auto rRR = P.scratch<double>(nh * 9), rRT = P.scratch<double>(nh * 3);  // the refined poses and masks
    const auto rRM = P.scratch<uint64_t>(nh * W);
    const auto rSoa = P.scratch<float>((size_t)NV_PNP * cap);
    OrbHostCall call(P, device);
    if (call.err) return call.err;
    a.c0 = call.send(r1, p3d);
    a.c1 = call.send(r2, p2d);
    a.c2 = call.send(r3, sigma2);
    call.put(rL, sel);
    cs.args(call, a, n, best_in, rM, rSoa);
    PnpArgs y{};
    if (mode != PNP_POSE_N) (sets ? y.sets : y.rand31) = call.send(rD, sets ? sets : rand31);
    y.R = call.dev(rR);
    y.t = call.dev(rT);
    y.rep = call.dev(rE);
    y.sets_out = call.dev(rSet);
    y.rR = call.dev(rRR);
    y.rt = call.dev(rRT);
    y.rcounts = call.dev(rRC);
    y.rmasks = W ? call.dev(rRM) : nullptr;  // no pointer to an empty region
    y.first_refined = call.dev(rFR);
    y.pose_inliers = y.first_refined + 1;
    y.pose = call.dev(rP);
    y.pose_mask = call.dev(rPM);
    if (int r = call.upload()) return r;
    int r = ORB_OK;
    hipError_t e = hipSuccess;
    if (mode == PNP_POSE_N) {
        y.sel = call.dev(rL);
        y.n_sel = n_sel;
        y.rR = y.R, y.rt = y.t;  // the pose goes where the caller reads R and t
        y.rcounts = nullptr;
        hipLaunchKernelGGL((k_cons_prepare<PNP>), dim3(1), dim3(CS_PREP_THREADS), 0, call.stream(), a);
        e = hipGetLastError();
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_pnp_refine, dim3(1, 1), dim3(64), 0, call.stream(), a, y);
            e = hipGetLastError();
        }
    } else
        r = launch_pnp(a, y, mode == PNP_RANSAC, call.stream());
    if (int rf = call.finish(r, e, "solvers: ")) return rf;
    if (mode == PNP_RANSAC) {
        cs.results(call, rM, counts, best_at, first, masks);
        call.get(rRC, o.refined_counts);
        call.get(rFR, o.first_refined, 1);
        call.get(rFR, o.pose_inliers, 1, 1);
        call.get(rP, o.pose);
        call.get(rPM, o.pose_mask);
    }
    call.get(rR, o.R);
    call.get(rT, o.t);
    call.get(rE, o.rep);
    if (mode != PNP_POSE_N) call.get(rSet, o.sets_out);
    return ORB_OK;
}

}  // namespace

extern "C" {

int orb_sim3_compute_hypotheses(int n, const float* x3dc1, const float* x3dc2, int n_hyp, const int32_t* sets,
                                const int32_t* rand31, float* T12, float* T21, float* sim3, float* quat,
                                int32_t* sets_out, int device) {
    const char* who = "sim3_compute_hypotheses";
    if (n < 1 || !x3dc1 || !x3dc2) return fail(ORB_EINVAL, std::string(who) + ": bad arguments");
    if (int r = check_limits(who, n, n_hyp)) return r;
    if (int r = check_draws(who, 3, n, n_hyp, sets, rand31)) return r;
    if (rand31 && n < 3) return fail(ORB_EINVAL, std::string(who) + ": a minimal set is drawn from n >= 3 correspondences");
    ConsArgs a{};
    a.K1[0] = a.K1[1] = a.K2[0] = a.K2[1] = 1.0f;
    a.n_hyp = n_hyp;
    a.min_inliers = 0;
    const HypHost o{T12, T21, sim3, quat, sets_out, nullptr};
    return run_host_sim3(a, false, n, x3dc1, x3dc2, nullptr, nullptr, sets, rand31, o, nullptr, nullptr, nullptr, nullptr, 0,
                         device);
}

int orb_sim3_ransac(int n, const float* x3dc1, const float* x3dc2, const float* sigma2_1, const float* sigma2_2,
                    const float* K1, const float* K2, int n_hyp, const int32_t* sets, const int32_t* rand31,
                    int min_inliers, int best_in, int32_t* counts, uint64_t* masks, int32_t* best_at,
                    int32_t* first_accept, float* T12, float* T21, float* sim3, int32_t* sets_out, float* accepted,
                    int device) {
    const char* who = "sim3_ransac";
    if (n < 0 || (n && (!x3dc1 || !x3dc2 || !sigma2_1 || !sigma2_2)) || !K1 || !K2)
        return fail(ORB_EINVAL, std::string(who) + ": bad arguments");
    if (int r = check_limits(who, n, n_hyp)) return r;
    if (int r = check_min_inliers(who, 3, min_inliers)) return r;
    if (int r = check_draws(who, 3, n, n_hyp, sets, rand31)) return r;
    if (int r = check_sigma2(who, sigma2_1, n, true)) return r;
    if (int r = check_sigma2(who, sigma2_2, n, true)) return r;
    ConsArgs a{};
    std::memcpy(a.K1, K1, 16);
    std::memcpy(a.K2, K2, 16);
    a.n_hyp = n_hyp;
    a.min_inliers = min_inliers;
    const HypHost o{T12, T21, sim3, nullptr, sets_out, accepted};
    return run_host_sim3(a, true, n, x3dc1, x3dc2, sigma2_1, sigma2_2, sets, rand31, o, counts, masks, best_at,
                         first_accept, best_in, device);
}

int orb_sim3_ransac_batch_device(const orb_keypoint_t* d_kps, const int32_t* d_counts, int cap, int S,
                                 const int32_t* d_pair_a, const int32_t* d_pair_b, const int32_t* d_match,
                                 const float* d_mp_pos, const uint8_t* d_mp_bad, const float* d_pose,
                                 const float* level_sigma2, int nlevels, const float* K, int n_hyp,
                                 const int32_t* d_rand31, int min_inliers, const int32_t* d_best_in, int32_t* d_n,
                                 int32_t* d_index, int32_t* d_counts_out, uint64_t* d_masks, int32_t* d_best_at,
                                 int32_t* d_first_accept, float* d_T12, float* d_T21, float* d_sim3,
                                 int32_t* d_sets_out, float* d_accepted, uint64_t* d_accepted_mask, void* stream) {
    const char* who = "sim3_ransac_batch";
    ConsArgs a{};
    if (int r = fill_batch(a, who, d_kps, d_counts, cap, S, d_pair_a, d_pair_b, d_match, d_mp_pos, d_mp_bad,
                           level_sigma2, nlevels, n_hyp, true))
        return r;
    if (int r = check_min_inliers(who, 3, min_inliers)) return r;
    if (S == 0) return ORB_OK;
    if (!d_pose || !K) return fail(ORB_EINVAL, std::string(who) + ": bad arguments");
    if (!d_rand31) return fail(ORB_EINVAL, std::string(who) + ": no rand31 values given");
    hipStream_t st = (hipStream_t)stream;
    a.pose = d_pose;
    std::memcpy(a.K1, K, 16);
    std::memcpy(a.K2, K, 16);
    a.min_inliers = min_inliers;
    a.best_in = d_best_in;
    a.index = d_index;
    // stream-ordered scratch for the SoA values and for every array the chain needs and the caller
    // did not ask for
    const size_t SH = (size_t)S * n_hyp;
    const bool want_acc = d_accepted || d_accepted_mask;
    HypArgs y{};
    y.rand31 = d_rand31;
    y.sets_out = d_sets_out;
    void* tmp = nullptr;
    if (int r = orb_scratch_alloc(&tmp, st, "solvers: scratch: ", [&](OrbLayout& L) {
            a.soa = L.take<float>((size_t)S * NV_SIM3 * cap);
            a.n = L.given_or_take(d_n, (size_t)S);
            a.counts = L.given_or_take(d_counts_out, SH);
            y.T12 = L.given_or_take(d_T12, SH * 12);
            y.T21 = L.given_or_take(d_T21, SH * 12);
            // (NULL where the caller gave none and the accepted hypothesis, which reads them, is not wanted)
            y.sim3 = d_sim3 ? d_sim3 : d_accepted ? L.take<float>(SH * 13) : nullptr;
            a.best_at = d_best_at ? d_best_at : want_acc ? L.take<int32_t>(SH) : nullptr;
            a.first = d_first_accept ? d_first_accept : want_acc ? L.take<int32_t>((size_t)S) : nullptr;
            a.masks = d_masks ? d_masks : d_accepted_mask ? L.take<uint64_t>(SH * a.W) : nullptr;
        }))
        return r;
    int r = launch<SIM3, float>(a, y.T12, y.T21, st, &y);
    if (r == ORB_OK && want_acc) {
        hipLaunchKernelGGL(k_sim3_accepted, dim3(S), dim3(64), 0, st, a, y.sim3, d_accepted, d_accepted_mask);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) r = fail(ORB_EDEVICE, std::string("solvers: ") + hipGetErrorString(e));
    }
    (void)hipFreeAsync(tmp, st);
    return r;
}

int orb_pnp_compute_hypotheses(int n, const float* p3d, const float* p2d, double fu, double fv, double uc, double vc,
                               int n_hyp, const int32_t* sets, const int32_t* rand31, double* R, double* t,
                               double* rep_error, int32_t* sets_out, int device) {
    const char* who = "pnp_compute_hypotheses";
    if (n < 1 || !p3d || !p2d) return fail(ORB_EINVAL, std::string(who) + ": bad arguments");
    if (int r = check_limits(who, n, n_hyp)) return r;
    if (int r = check_draws(who, 4, n, n_hyp, sets, rand31)) return r;
    if (rand31 && n < 4) return fail(ORB_EINVAL, std::string(who) + ": a minimal set is drawn from n >= 4 correspondences");
    ConsArgs a{};
    a.fu = fu, a.fv = fv, a.uc = uc, a.vc = vc;
    a.n_hyp = n_hyp;
    a.min_inliers = 0;
    const PnpHost o{R, t, rep_error, sets_out, nullptr, nullptr, nullptr, nullptr, nullptr};
    return run_host_pnp(a, PNP_HYP, n, p3d, p2d, nullptr, sets, rand31, nullptr, 0, o, nullptr, nullptr, nullptr, nullptr,
                        0, device);
}

int orb_pnp_compute_pose_n(int n, const float* p3d, const float* p2d, double fu, double fv, double uc, double vc,
                           int n_sel, const int32_t* sel, double* R, double* t, double* rep_error, int device) {
    const char* who = "pnp_compute_pose_n";
    if (n < 1 || !p3d || !p2d || !sel) return fail(ORB_EINVAL, std::string(who) + ": bad arguments");
    if (int r = check_limits(who, n, 1)) return r;
    if (n_sel < 1 || n_sel > CS_MAX_CAP)
        return fail(ORB_EINVAL, std::string(who) + ": n_sel must be in [1, 8192] (got " + std::to_string(n_sel) + ")");
    for (int k = 0; k < n_sel; ++k)
        if (sel[k] < 0 || sel[k] >= n)
            return fail(ORB_EINVAL, std::string(who) + ": sel[" + std::to_string(k) + "] = " + std::to_string(sel[k]) +
                                        " is outside [0, n)");
    ConsArgs a{};
    a.fu = fu, a.fv = fv, a.uc = uc, a.vc = vc;
    a.n_hyp = 1;
    const PnpHost o{R, t, rep_error, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    return run_host_pnp(a, PNP_POSE_N, n, p3d, p2d, nullptr, nullptr, nullptr, sel, n_sel, o, nullptr, nullptr, nullptr,
                        nullptr, 0, device);
}

int orb_pnp_ransac(int n, const float* p3d, const float* p2d, const float* sigma2, float th2, double fu, double fv,
                   double uc, double vc, int n_hyp, const int32_t* sets, const int32_t* rand31, int min_inliers,
                   int best_in, int32_t* counts, uint64_t* masks, int32_t* best_at, int32_t* first_ok, double* R,
                   double* t, int32_t* sets_out, int32_t* refined_counts, int32_t* first_refined, float* pose,
                   uint64_t* pose_mask, int32_t* pose_inliers, int device) {
    const char* who = "pnp_ransac";
    if (n < 0 || (n && (!p3d || !p2d || !sigma2))) return fail(ORB_EINVAL, std::string(who) + ": bad arguments");
    if (int r = check_limits(who, n, n_hyp)) return r;
    if (int r = check_min_inliers(who, 4, min_inliers)) return r;
    if (int r = check_draws(who, 4, n, n_hyp, sets, rand31)) return r;
    if (int r = check_sigma2(who, sigma2, n, false)) return r;
    ConsArgs a{};
    a.th2 = th2;
    a.fu = fu, a.fv = fv, a.uc = uc, a.vc = vc;
    a.n_hyp = n_hyp;
    a.min_inliers = min_inliers;
    const PnpHost o{R, t, nullptr, sets_out, refined_counts, first_refined, pose, pose_mask, pose_inliers};
    return run_host_pnp(a, PNP_RANSAC, n, p3d, p2d, sigma2, sets, rand31, nullptr, 0, o, counts, masks, best_at, first_ok,
                        best_in, device);
}

int orb_pnp_ransac_batch_device(const orb_keypoint_t* d_kps, const int32_t* d_counts, int cap, int S,
                                const int32_t* d_pair_a, const int32_t* d_pair_b, const int32_t* d_match,
                                const float* d_mp_pos, const uint8_t* d_mp_bad, const float* level_sigma2, int nlevels,
                                float th2, double fu, double fv, double uc, double vc, int n_hyp,
                                const int32_t* d_rand31, int min_inliers, const int32_t* d_best_in, int32_t* d_n,
                                int32_t* d_index, int32_t* d_counts_out, uint64_t* d_masks, int32_t* d_best_at,
                                int32_t* d_first_ok, double* d_R, double* d_t, int32_t* d_sets_out,
                                int32_t* d_refined_counts, int32_t* d_first_refined, float* d_pose,
                                uint64_t* d_pose_mask, int32_t* d_pose_inliers, void* stream) {
    const char* who = "pnp_ransac_batch";
    ConsArgs a{};
    if (int r = fill_batch(a, who, d_kps, d_counts, cap, S, d_pair_a, d_pair_b, d_match, d_mp_pos, d_mp_bad,
                           level_sigma2, nlevels, n_hyp, false))
        return r;
    if (int r = check_min_inliers(who, 4, min_inliers)) return r;
    if (S == 0) return ORB_OK;
    if (!d_rand31) return fail(ORB_EINVAL, std::string(who) + ": no rand31 values given");
    hipStream_t st = (hipStream_t)stream;
    a.th2 = th2;
    a.fu = fu, a.fv = fv, a.uc = uc, a.vc = vc;
    a.min_inliers = min_inliers;
    a.best_in = d_best_in;
    a.index = d_index;
    // stream-ordered scratch for the SoA values, the refined poses and masks, and for every array the
    // chain needs and the caller did not ask for
    const size_t SH = (size_t)S * n_hyp;
    PnpArgs y{};
    y.rand31 = d_rand31;
    y.sets_out = d_sets_out;
    a.first = d_first_ok;
    y.first_refined = d_first_refined;
    y.pose = d_pose;
    y.pose_mask = d_pose_mask;
    y.pose_inliers = d_pose_inliers;
    void* tmp = nullptr;
    if (int r = orb_scratch_alloc(&tmp, st, "solvers: scratch: ", [&](OrbLayout& L) {
            a.soa = L.take<float>((size_t)S * NV_PNP * cap);
            a.n = L.given_or_take(d_n, (size_t)S);
            a.counts = L.given_or_take(d_counts_out, SH);
            y.R = L.given_or_take(d_R, SH * 9);
            y.t = L.given_or_take(d_t, SH * 3);
            a.best_at = L.given_or_take(d_best_at, SH);
            a.masks = L.given_or_take(d_masks, SH * a.W);
            y.rcounts = L.given_or_take(d_refined_counts, SH);
            y.rR = L.take<double>(SH * 9);
            y.rt = L.take<double>(SH * 3);
            y.rmasks = L.take<uint64_t>(SH * a.W);
        }))
        return r;
    const int r = launch_pnp(a, y, true, st);
    (void)hipFreeAsync(tmp, st);
    return r;
}

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
