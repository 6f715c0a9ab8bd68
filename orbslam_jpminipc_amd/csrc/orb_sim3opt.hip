// orb_sim3opt.hip — Optimizer::OptimizeSim3 on the GPU (part of liborb_hip.so).
//
// The 7-DoF optimisation that LoopClosing::ComputeSim3 runs per loop candidate between SearchBySim3
// and SearchByProjection (reference src/Optimizer.cc:1721-1917; LoopClosing.cc:340), with the parts of
// g2o it runs restated in double:
//   set-up          Optimizer.cc:1733-1853: per usable slot the fixed points P3D1c / P3D2c, the edges
//                   e12 (obs kpUn1, point P3D2c, information invSigma2(octave1) I) and e21 (obs kpUn2,
//                   point P3D1c, information sigma2(octave2) I: GetSigma2, line 1842), Huber delta
//                   (double)(float)sqrt(th2)
//   state           g2o::Sim3 (sim3.h:41-292): quaternion (never normalised), t, s; Sim3(R, t, s) 64-67,
//                   map 144-146, inverse 233-236, operator* 266-272, Sim3(update) 70-142
//   edges           computeError of EdgeSim3ProjectXYZ / EdgeInverseSim3ProjectXYZ
//                   (types_seven_dof_expmap.h:138-145, 160-167); oplusImpl 60-69
//   Jacobian        BaseBinaryEdge::linearizeOplus, numeric (base_binary_edge.hpp:131-205): central
//                   differences at 1e-9 through oplus, restated literally
//   quadratic form  base_binary_edge.hpp:91-113 with RobustKernelHuber, as §13
//   Levenberg       optimization_algorithm_levenberg.cpp:61-189, dense solver linear_solver_dense.h:104-112
//   schedule        Optimizer.cc:1857-1916
// The quaternion and rotation helpers, the Huber kernel, ldlt<7>, the Levenberg bookkeeping, the
// workgroup sum, the compaction step and the Sim3 state with its map, inverse, product and exponential are
// those of csrc/orb_g2o_math.h, shared with the other optimizer units; this unit holds the two edges and
// the schedule.
//
// Arithmetic: all f64, the TU built -ffp-contract=off; inputs are widened from f32 once, in the
// prepare step (the batch form's camera-frame points are the float row sums of §12 first, gemm3_add of
// csrc/orb_cv_math.h).  Sums
// over edges are taken in a fixed order (thread-strided partial sums, e12 before e21 of a pair, an
// xor butterfly across the wave, the four waves in order): a call gives the same bits on every run.
// There is no floating-point atomic.
//
//   k_s3_prepare  one workgroup per problem: compacts the usable slots in index order (ballot +
//                 popcount prefix, wave totals through LDS) to SoA doubles X1c X2c obs1 obs2 info1
//                 info2 and the index list; writes the kept row / the copy of the match row.
//   k_s3_solve    one workgroup per problem runs the whole schedule.  Thread t owns the pairs t,
//                 t + 256, ...  Per build the 15 estimates of the numeric Jacobian (the estimate and
//                 its 14 perturbations) and their inverses are computed once, by 15 threads, into
//                 LDS; an edge then costs 15 map-and-project evaluations.  A build pass reduces the
//                 28 + 7 + 1 values of H, b and the robust chi2, a trial pass one value.  After a
//                 reduction every thread holds the same bits, so the 7 x 7 solve, the update and every
//                 decision of the schedule are taken redundantly by all threads: no broadcast, and
//                 branches are uniform.  Every loop has a static bound (2 rounds, 5 and <= 10
//                 iterations, 10 trials, ceil(n / 256) pairs).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <string>

#include "../../include/orb_abi.h"
#include "orb_cv_math.h"
#include "orb_g2o_math.h"
#include "orb_internal.h"

namespace {

int fail(int code, const std::string& msg) { return orb_internal_set_error(code, msg); }

constexpr int S3_MAX_CAP = 8192;
constexpr int S3_THREADS = 256;
constexpr int S3_WAVES = S3_THREADS / 64;
static_assert(S3_WAVES == G2O_WAVES, "block_sum and compact_slot are written for this many waves");
constexpr int S3_NV = 14;    // X1c(3) X2c(3) obs1(2) obs2(2) info1 info2 | chi2 of e12, e21 at their last evaluation
constexpr int S3_NACC = 36;  // 28 of H (upper triangle), 7 of b, the robust chi2
constexpr int S3_NST = 15;   // the estimate and its 14 perturbations

struct S3Args {
    // batch form: records of keyframes pair_a[s] / pair_b[s], row s of match, positions and poses per keyframe
    const orb_keypoint_t* kps;
    const int32_t* kcounts;
    const int32_t* pair_a;
    const int32_t* pair_b;
    const int32_t* match;
    const float* mp_pos;
    const uint8_t* mp_bad;
    const float* pose;
    int32_t* match_out;
    float level_sigma2[ORB_MAX_VIEW_LEVELS], inv_level_sigma2[ORB_MAX_VIEW_LEVELS];
    int nlevels;
    // host form (n_direct >= 0): one problem, the per-slot values given directly
    const float *x1, *x2, *obs1, *obs2, *w1, *w2;
    const uint8_t* usable;
    uint8_t* kept;
    int n_direct;
    double K1[4], K2[4];
    double delta;  // the Huber delta, (double)(float)sqrt(th2) (Optimizer.cc:1770)
    double th2;    // (double)th2, what chi2() is compared with
    const float* sim3_in;
    float* sim3_out;
    double* sim3_out64;
    int32_t* n_inliers;
    orb_sim3_opt_info_t* info;
    // scratch
    double* soa;     // S x S3_NV x cap
    int32_t* index;  // S x cap
    int32_t* n;      // S
    int cap, S;
};

__global__ void __launch_bounds__(S3_THREADS) k_s3_prepare(S3Args a) {
    __shared__ int s_wtot[S3_WAVES];
    const int s = blockIdx.x, tid = threadIdx.x;
    const bool direct = a.n_direct >= 0;
    const int cap = a.cap;
    int fa = 0, fb = 0, n_row, nb = 0;
    if (direct) {
        n_row = a.n_direct;
    } else {
        // an entry is a match only inside both counts, so no read leaves the batch arrays
        fa = a.pair_a[s], fb = a.pair_b[s];
        n_row = min(max(a.kcounts[fa], 0), cap);
        nb = min(max(a.kcounts[fb], 0), cap);
    }
    const int32_t* row = direct ? nullptr : a.match + (size_t)s * cap;
    double* q = a.soa + (size_t)s * S3_NV * cap;
    int32_t* index = a.index + (size_t)s * cap;
    const int n_all = direct ? a.n_direct : cap;
    int base = 0;
    for (int i0 = 0; i0 < n_all; i0 += S3_THREADS) {
        const int i = i0 + tid;
        int m = -1;
        bool ok = false;
        if (i < n_all) {
            if (direct) {
                ok = a.usable ? a.usable[i] != 0 : true;
                a.kept[i] = ok ? 1 : 0;
            } else {
                const int e = row[i];
                if (a.match_out) a.match_out[(size_t)s * cap + i] = e;
                m = e;
                ok = i < n_row && (unsigned)m < (unsigned)nb;
                if (ok && a.mp_bad) ok = !a.mp_bad[(size_t)fa * cap + i] && !a.mp_bad[(size_t)fb * cap + m];
            }
        }
        const int o = compact_slot(ok, s_wtot, base);
        if (o >= 0) {
            float X1[3], X2[3], o1[2], o2[2], w1, w2;
            if (direct) {
#pragma unroll
                for (int k = 0; k < 3; ++k) X1[k] = a.x1[3 * i + k], X2[k] = a.x2[3 * i + k];
#pragma unroll
                for (int k = 0; k < 2; ++k) o1[k] = a.obs1[2 * i + k], o2[k] = a.obs2[2 * i + k];
                w1 = a.w1[i], w2 = a.w2[i];
            } else {
                const size_t k1 = (size_t)fa * cap + i, k2 = (size_t)fb * cap + m;
                // cv::Mat Rcw * X + tcw as §12 states it (csrc/orb_cv_math.h)
                const float* Ta = a.pose + (size_t)fa * 12;
                const float* Tb = a.pose + (size_t)fb * 12;
                orb_cv::gemm3_add(Ta, a.mp_pos + 3 * k1, Ta + 9, X1);
                orb_cv::gemm3_add(Tb, a.mp_pos + 3 * k2, Tb + 9, X2);
                const orb_keypoint_t& kp1 = a.kps[k1];
                const orb_keypoint_t& kp2 = a.kps[k2];
                o1[0] = kp1.x, o1[1] = kp1.y, o2[0] = kp2.x, o2[1] = kp2.y;
                w1 = a.inv_level_sigma2[min(max(kp1.octave, 0), a.nlevels - 1)];
                w2 = a.level_sigma2[min(max(kp2.octave, 0), a.nlevels - 1)];  // GetSigma2 (Optimizer.cc:1842)
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) q[(size_t)k * cap + o] = (double)X1[k], q[(size_t)(3 + k) * cap + o] = (double)X2[k];
#pragma unroll
            for (int k = 0; k < 2; ++k) q[(size_t)(6 + k) * cap + o] = (double)o1[k], q[(size_t)(8 + k) * cap + o] = (double)o2[k];
            q[(size_t)10 * cap + o] = (double)w1, q[(size_t)11 * cap + o] = (double)w2;
            index[o] = i;
        }
    }
    if (tid == 0) a.n[s] = base;
}

// struct Sim3, sim3_map, sim3_inverse, the product and the exponential are csrc/orb_g2o_math.h's
__device__ __forceinline__ Sim3 oplus(const double* u, const Sim3& T) { return sim3_oplus(u, T); }

// obs - cam_map(project(M.map(X))); project does not look at the depth
__device__ __forceinline__ void edge_error(const Sim3& M, const double* K, const double* X, const double* obs,
                                           double* e) {
    double P[3];
    sim3_map(M, X, P);
    e[0] = obs[0] - ((P[0] / P[2]) * K[0] + K[2]);
    e[1] = obs[1] - ((P[1] / P[2]) * K[1] + K[3]);
}

// One edge's share of a build pass: error at M[0], the numeric Jacobian over M[1..14]
// (base_binary_edge.hpp:131-205), the robust quadratic form (91-113) added to acc; returns its chi2.
__device__ __forceinline__ double edge_build(const Sim3* M, const double* K, const double* X, const double* obs,
                                             double w, double delta, double dsqr, double* acc) {
    double e[2], J[14];
    edge_error(M[0], K, X, obs, e);
    const double scalar = 1.0 / (2 * 1e-9);
#pragma unroll
    for (int d = 0; d < 7; ++d) {
        double ep[2], em[2];
        edge_error(M[1 + 2 * d], K, X, obs, ep);
        edge_error(M[2 + 2 * d], K, X, obs, em);
        J[d] = scalar * (ep[0] - em[0]);
        J[7 + d] = scalar * (ep[1] - em[1]);
        // An empty statement that pins the column: the 14 evaluations are independent, and scheduled
        // side by side (their LDS reads first) they spilled 964 B per lane; one after the other the
        // kernel has no scratch.  The arithmetic is the same either way.
        __asm__ volatile("" : "+v"(J[d]), "+v"(J[7 + d]));
    }
    const double c2 = e[0] * (w * e[0]) + e[1] * (w * e[1]);
    double rho0, rho1;
    huber(c2, delta, dsqr, &rho0, &rho1);
    const double wo = w * rho1;  // weightedOmega = rho[1] * omega
    const double r0 = (-(w * e[0])) * rho1, r1 = (-(w * e[1])) * rho1;
    int c = 0;
#pragma unroll
    for (int j = 0; j < 7; ++j)
#pragma unroll
        for (int k = j; k < 7; ++k) acc[c++] += (J[j] * wo) * J[k] + (J[7 + j] * wo) * J[7 + k];
#pragma unroll
    for (int j = 0; j < 7; ++j) acc[28 + j] += J[j] * r0 + J[7 + j] * r1;
    acc[35] += rho0;
    return c2;
}

__global__ void __launch_bounds__(S3_THREADS) k_s3_solve(S3Args a) {
    __shared__ double s_red[S3_WAVES][S3_NACC];
    __shared__ Sim3 s_fwd[S3_NST], s_inv[S3_NST];
    __shared__ uint8_t s_off[S3_MAX_CAP];  // the pair was removed by the first classification
    __shared__ int s_cnt[1];
    const int s = blockIdx.x, tid = threadIdx.x, cap = a.cap;
    const int n = min(max(a.n[s], 0), min(cap, S3_MAX_CAP));
    double* q = a.soa + (size_t)s * S3_NV * cap;
    double* chi12 = q + (size_t)12 * cap;
    double* chi21 = q + (size_t)13 * cap;
    const double delta = a.delta, dsqr = delta * delta, th = a.th2;
    const double K1[4] = {a.K1[0], a.K1[1], a.K1[2], a.K1[3]};
    const double K2[4] = {a.K2[0], a.K2[1], a.K2[2], a.K2[3]};
    for (int e = tid; e < n; e += S3_THREADS) s_off[e] = 0;
    if (tid == 0) s_cnt[0] = 0;
    Sim3 S0;
    {  // Sim3(Matrix3d R, t, s): the quaternion of the widened R, not normalised
        const float* p = a.sim3_in + (size_t)s * 13;
        double R[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = (double)p[k];
        quat_from_matrix(R, S0.q);
#pragma unroll
        for (int k = 0; k < 3; ++k) S0.t[k] = (double)p[9 + k];
        S0.s = (double)p[12];
    }
    Sim3 T = S0;
    __syncthreads();
    int iters[2] = {0, 0};
    int trials = 0, n_bad = 0, more = 0, n_in = 0;
    bool copy_out = false;
    double lambda = -1., ni = 2., last_chi = 0.;
    double x[7] = {0, 0, 0, 0, 0, 0, 0};
    #pragma unroll 1
    for (int r = 0; r < 2; ++r) {
        const int its = r == 0 ? 5 : more;
        int bad_steps = 0;
        bool stop = n <= 0;
        #pragma unroll 1
        for (int it = 0; it < 10; ++it) {
            if (stop || it >= its) break;
            ++iters[r];
            // the estimates of the numeric Jacobian and their inverses, once per build
            __syncthreads();  // the readers of the last trial's states are done
            if (tid < S3_NST) {
                Sim3 P = T;
                if (tid > 0) {
                    double u[7] = {0, 0, 0, 0, 0, 0, 0};
                    const int d = (tid - 1) >> 1;
                    const double h = (tid & 1) ? 1e-9 : -1e-9;
#pragma unroll
                    for (int k = 0; k < 7; ++k) u[k] = k == d ? h : 0.0;
                    P = oplus(u, T);
                }
                s_fwd[tid] = P;
                s_inv[tid] = sim3_inverse(P);
            }
            __syncthreads();
            // computeActiveErrors + activeRobustChi2 + buildSystem at T
            double acc[S3_NACC];
#pragma unroll
            for (int k = 0; k < S3_NACC; ++k) acc[k] = 0.;
            #pragma unroll 1
            for (int e = tid; e < n; e += S3_THREADS) {
                if (s_off[e]) continue;
                const double X1[3] = {q[e], q[(size_t)cap + e], q[(size_t)2 * cap + e]};
                const double X2[3] = {q[(size_t)3 * cap + e], q[(size_t)4 * cap + e], q[(size_t)5 * cap + e]};
                const double o1[2] = {q[(size_t)6 * cap + e], q[(size_t)7 * cap + e]};
                const double o2[2] = {q[(size_t)8 * cap + e], q[(size_t)9 * cap + e]};
                chi12[e] = edge_build(s_fwd, K1, X2, o1, q[(size_t)10 * cap + e], delta, dsqr, acc);
                chi21[e] = edge_build(s_inv, K2, X1, o2, q[(size_t)11 * cap + e], delta, dsqr, acc);
            }
            block_sum<S3_NACC>(acc, s_red);
            // acc stays as the system: H's upper triangle in acc[0..28), b in acc[28..35)
            const double* b = acc + 28;
            double cur = acc[35];
            const double ini = cur;
            if (it == 0) {
                lambda = lm_lambda_init<7>(acc);
                ni = 2.;
                bad_steps = 0;
            }
            double rho = 0;
            int qmax = 0;
            bool again = true;
            #pragma unroll 1
            for (int tr = 0; tr < 10; ++tr) {
                if (!again) break;
                const Sim3 backup = T;
                double A[49];
                lm_damped<7>(acc, lambda, A);
                const bool ok2 = ldlt<7>(A, b, x);
                T = oplus(x, T);
                const Sim3 Ti = sim3_inverse(T);
                double t1[1] = {0.};
                #pragma unroll 1
                for (int e = tid; e < n; e += S3_THREADS) {
                    if (s_off[e]) continue;
                    const double X1[3] = {q[e], q[(size_t)cap + e], q[(size_t)2 * cap + e]};
                    const double X2[3] = {q[(size_t)3 * cap + e], q[(size_t)4 * cap + e], q[(size_t)5 * cap + e]};
                    const double o1[2] = {q[(size_t)6 * cap + e], q[(size_t)7 * cap + e]};
                    const double o2[2] = {q[(size_t)8 * cap + e], q[(size_t)9 * cap + e]};
                    const double w1 = q[(size_t)10 * cap + e], w2 = q[(size_t)11 * cap + e];
                    double er[2], rho0, rho1;
                    edge_error(T, K1, X2, o1, er);
                    const double c12 = er[0] * (w1 * er[0]) + er[1] * (w1 * er[1]);
                    chi12[e] = c12;
                    huber(c12, delta, dsqr, &rho0, &rho1);
                    t1[0] += rho0;
                    edge_error(Ti, K2, X1, o2, er);
                    const double c21 = er[0] * (w2 * er[0]) + er[1] * (w2 * er[1]);
                    chi21[e] = c21;
                    huber(c21, delta, dsqr, &rho0, &rho1);
                    t1[0] += rho0;
                }
                block_sum<1>(t1, s_red);
                const double temp = ok2 ? t1[0] : DBL_MAX;
                rho = (cur - temp) / lm_scale<7>(x, lambda, b);
                if (lm_accept(rho, temp, lambda, ni)) cur = temp;
                else T = backup;
                ++qmax;
                ++trials;
                again = rho < 0 && qmax < 10;  // a NaN rho leaves the loop
            }
            last_chi = cur;
            stop = lm_stop(qmax, rho, ini, cur, bad_steps);
        }
        // classification (Optimizer.cc:1862-1879, 1896-1910) on the chi2 of the last evaluation; each
        // thread reads what it wrote
        __syncthreads();
        if (tid == 0) s_cnt[0] = 0;
        __syncthreads();
        int cnt = 0;
        for (int e = tid; e < n; e += S3_THREADS) {
            if (s_off[e]) continue;
            const bool bad = chi12[e] > th || chi21[e] > th;  // a NaN chi2 is not > th2
            if (r == 0) {
                if (bad) s_off[e] = 1, ++cnt;
            } else {
                if (bad) s_off[e] = 2;
                else ++cnt;
            }
        }
        if (cnt) atomicAdd(&s_cnt[0], cnt);
        __syncthreads();
        if (r == 0) {
            n_bad = s_cnt[0];
            if (n - n_bad < 10) break;  // return 0: the estimate is not copied out
            more = n_bad > 0 ? 10 : 5;
        } else {
            n_in = s_cnt[0];
            copy_out = true;
        }
    }
    const int32_t* index = a.index + (size_t)s * cap;
    for (int e = tid; e < n; e += S3_THREADS) {
        if (!s_off[e]) continue;
        if (a.kept) a.kept[index[e]] = 0;
        if (a.match_out) a.match_out[(size_t)s * cap + index[e]] = -1;
    }
    if (tid == 0) {
        const Sim3 O = copy_out ? T : S0;
        if (a.sim3_out64) {
            double* o = a.sim3_out64 + (size_t)s * 8;
            for (int k = 0; k < 4; ++k) o[k] = O.q[k];
            for (int k = 0; k < 3; ++k) o[4 + k] = O.t[k];
            o[7] = O.s;
        }
        if (a.sim3_out) {
            double M[13];
            matrix_from_quat(O.q, M);
            for (int k = 0; k < 3; ++k) M[9 + k] = O.t[k];
            M[12] = O.s;
            for (int k = 0; k < 13; ++k) a.sim3_out[(size_t)s * 13 + k] = (float)M[k];
        }
        if (a.n_inliers) a.n_inliers[s] = n_in;
        if (a.info) {
            orb_sim3_opt_info_t I;
            I.n_correspondences = n, I.n_bad = n_bad, I.more_iterations = more;
            I.iterations[0] = iters[0], I.iterations[1] = iters[1];
            I.trials = trials, I.lambda = lambda, I.chi2 = last_chi;
            a.info[s] = I;
        }
    }
}

int launch(S3Args a, float th2, hipStream_t st) {
    a.delta = (double)std::sqrt(th2);  // const float deltaHuber = sqrt(th2)
    a.th2 = (double)th2;
    hipLaunchKernelGGL(k_s3_prepare, dim3(a.S), dim3(S3_THREADS), 0, st, a);
    ORB_HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_s3_solve, dim3(a.S), dim3(S3_THREADS), 0, st, a);
    ORB_HIPCHK(hipGetLastError());
    return ORB_OK;
}

int check_th2(const char* who, float th2) {
    if (!std::isfinite(th2) || th2 < 0)
        return fail(ORB_EINVAL, std::string(who) + ": th2 = " + std::to_string(th2) + " must be finite and not negative");
    return ORB_OK;
}

}  // namespace

extern "C" {

int orb_optimize_sim3(int n, const float* x3dc1, const float* x3dc2, const float* obs1, const float* obs2,
                      const float* inv_sigma2_1, const float* sigma2_2, const uint8_t* usable, const float* K1,
                      const float* K2, float th2, const float* sim3_in, uint8_t* kept, double* sim3_out_f64,
                      float* sim3_out, int32_t* n_inliers, orb_sim3_opt_info_t* info, int device) {
    const char* who = "optimize_sim3";
    if (n < 0 || (n && (!x3dc1 || !x3dc2 || !obs1 || !obs2 || !inv_sigma2_1 || !sigma2_2 || !kept)) || !K1 || !K2 ||
        !sim3_in)
        return fail(ORB_EINVAL, std::string(who) + ": bad arguments");
    if (n > S3_MAX_CAP) return fail(ORB_ENOTSUP, std::string(who) + ": more than 8192 slots");
    if (int r = orb_check_camera(who, "K1", K1)) return r;
    if (int r = orb_check_camera(who, "K2", K2)) return r;
    if (int r = check_th2(who, th2)) return r;
    for (int k = 0; k < 13; ++k)
        if (!std::isfinite(sim3_in[k]))
            return fail(ORB_EINVAL, std::string(who) + ": sim3_in[" + std::to_string(k) + "] is not finite");
    const int cap = std::max(n, 1);
    const size_t N = (size_t)n;
    OrbStagePlan P;
    const auto rX1 = P.in<float>(N * 3), rX2 = P.in<float>(N * 3), rO1 = P.in<float>(N * 2), rO2 = P.in<float>(N * 2),
               rW1 = P.in<float>(N), rW2 = P.in<float>(N);
    const auto rU = P.in<uint8_t>(N);
    const auto rT = P.in<float>(13);
    const auto r64 = P.out<double>(8);
    const auto rI = P.out<orb_sim3_opt_info_t>(1);
    const auto r32 = P.out<float>(13);
    const auto rN = P.out<int32_t>(1);
    const auto rK = P.out<uint8_t>(cap);
    const auto rSoa = P.scratch<double>((size_t)S3_NV * cap);
    const auto rIdx = P.scratch<int32_t>(cap), rCnt = P.scratch<int32_t>(1);
    OrbHostCall call(P, device);
    if (call.err) return call.err;
    S3Args a{};
    a.n_direct = n;
    a.x1 = call.send(rX1, x3dc1), a.x2 = call.send(rX2, x3dc2);
    a.obs1 = call.send(rO1, obs1), a.obs2 = call.send(rO2, obs2);
    a.w1 = call.send(rW1, inv_sigma2_1), a.w2 = call.send(rW2, sigma2_2);
    a.usable = usable ? call.send(rU, usable) : nullptr;
    a.nlevels = 1;
    for (int k = 0; k < 4; ++k) a.K1[k] = (double)K1[k], a.K2[k] = (double)K2[k];
    a.sim3_in = call.send(rT, sim3_in);
    a.sim3_out64 = call.dev(r64);
    a.info = call.dev(rI);
    a.sim3_out = call.dev(r32);
    a.n_inliers = call.dev(rN);
    a.kept = call.dev(rK);
    a.soa = call.dev(rSoa);
    a.index = call.dev(rIdx);
    a.n = call.dev(rCnt);
    a.cap = cap;
    a.S = 1;
    if (int r = call.upload()) return r;
    if (int r = call.finish(launch(a, th2, call.stream()), hipSuccess, std::string(who) + ": ")) return r;
    call.get(r64, sim3_out_f64);
    call.get(rI, info);
    call.get(r32, sim3_out);
    call.get(rN, n_inliers);
    call.get(rK, kept, N);
    return ORB_OK;
}

int orb_optimize_sim3_batch_device(const orb_keypoint_t* d_kps, const int32_t* d_counts, int cap, int S,
                                   const int32_t* d_pair_a, const int32_t* d_pair_b, const int32_t* d_match,
                                   const float* d_mp_pos, const uint8_t* d_mp_bad, const float* d_pose,
                                   const float* level_sigma2, const float* inv_level_sigma2, int nlevels,
                                   const float* K, float th2, const float* d_sim3_in, int32_t* d_match_out,
                                   float* d_sim3_out, double* d_sim3_out_f64, int32_t* d_n_inliers,
                                   orb_sim3_opt_info_t* d_info, void* stream) {
    const char* who = "optimize_sim3_batch";
    if (S < 0 || cap <= 0 || !K) return fail(ORB_EINVAL, std::string(who) + ": bad arguments");
    if (cap > S3_MAX_CAP) return fail(ORB_ENOTSUP, std::string(who) + ": more than 8192 keypoints per keyframe");
    if (S > 65535) return fail(ORB_ENOTSUP, std::string(who) + ": more than 65535 problems per call");
    if (!level_sigma2 || !inv_level_sigma2 || nlevels < 1 || nlevels > ORB_MAX_VIEW_LEVELS)
        return fail(ORB_EINVAL, std::string(who) + ": nlevels must be in [1, 16]");
    if (int r = orb_check_camera(who, "K", K)) return r;
    if (int r = check_th2(who, th2)) return r;
    if (S == 0) return ORB_OK;
    if (!d_kps || !d_counts || !d_pair_a || !d_pair_b || !d_match || !d_mp_pos || !d_pose || !d_sim3_in)
        return fail(ORB_EINVAL, std::string(who) + ": bad arguments");
    S3Args a{};
    a.kps = d_kps;
    a.kcounts = d_counts;
    a.pair_a = d_pair_a, a.pair_b = d_pair_b;
    a.match = d_match;
    a.mp_pos = d_mp_pos;
    a.mp_bad = d_mp_bad;
    a.pose = d_pose;
    a.match_out = d_match_out;
    std::memcpy(a.level_sigma2, level_sigma2, (size_t)nlevels * 4);
    std::memcpy(a.inv_level_sigma2, inv_level_sigma2, (size_t)nlevels * 4);
    a.nlevels = nlevels;
    a.n_direct = -1;
    for (int k = 0; k < 4; ++k) a.K1[k] = a.K2[k] = (double)K[k];
    a.sim3_in = d_sim3_in;
    a.sim3_out = d_sim3_out;
    a.sim3_out64 = d_sim3_out_f64;
    a.n_inliers = d_n_inliers;
    a.info = d_info;
    a.cap = cap;
    a.S = S;
    hipStream_t st = (hipStream_t)stream;
    void* tmp = nullptr;
    if (int r = orb_scratch_alloc(&tmp, st, std::string(who) + ": scratch: ", [&](OrbLayout& L) {
            a.soa = L.take<double>((size_t)S * S3_NV * cap);
            a.index = L.take<int32_t>((size_t)S * cap);
            a.n = L.take<int32_t>(S);
        }))
        return r;
    const int r = launch(a, th2, st);
    (void)hipFreeAsync(tmp, st);
    return r;
}

}  // extern "C"
