// orb_optimizer.hip — Optimizer::PoseOptimization(Frame*) on the GPU (part of liborb_hip.so).
//
// The motion-only optimisation that ends every tracking-time chain of the reference
// (src/Optimizer.cc:154-285; called from Tracking.cc:557, 580, 611, 643, 988, 1004, 1019), with the
// parts of g2o it runs restated in double:
//   set-up          Optimizer.cc:168-237: one edge per keypoint with a MapPoint, obs and the
//                   calibration widened from float, information invSigma2 * I, Huber delta
//                   (double)(float)sqrt(5.991)
//   pose in / out   Converter::toSE3Quat (Converter.cc:38-48), SE3Quat(R, t) + normalizeRotation
//                   (se3quat.h:58-59, 280-285), to_homogeneous_matrix (270-278)
//   edge            EdgeSE3ProjectXYZ::computeError / cam_project / _jacobianOplusXj
//                   (types_six_dof_expmap.h:172-177, .cpp:407-428)
//   quadratic form  base_binary_edge.hpp:91-113 with RobustKernelHuber (robust_kernel_impl.cpp:78-91);
//                   the rho[2] term is commented out in base_edge.h:96-102
//   Levenberg       optimization_algorithm_levenberg.cpp:61-189, update exp(x) * T
//                   (types_six_dof_expmap.h:104-107, se3quat.h:104-110, 223-257)
//   dense solver    linear_solver_dense.h:104-112: Eigen::LDLT, refused when not positive
//   four rounds     Optimizer.cc:242-276
// The quaternion and rotation helpers, the Huber kernel, ldlt<6>, the Levenberg bookkeeping, the
// workgroup sum, the compaction step and the SE3 state with exp(x) * T are those of
// csrc/orb_g2o_math.h, shared with csrc/orb_sim3opt.hip and csrc/orb_localba.hip; this unit holds
// the edge and the schedule.
//
// Arithmetic: all f64, the TU built -ffp-contract=off; inputs are widened from f32 once, in the
// prepare step.  Sums over edges are taken in a fixed order (thread-strided partial sums, an
// xor butterfly across the wave, the four waves in order), so a call gives the same bits on every
// run; the order differs from g2o's edge order, which is what the tests' tolerance measures.
// There is no floating-point atomic.
//
//   k_po_prepare  one workgroup per problem: compacts the keypoints that have a MapPoint in index
//                 order (ballot + popcount prefix, wave totals through LDS) to SoA doubles
//                 X Y Z u v invSigma2 and the index list; zeroes the outlier row.
//   k_po_solve    one workgroup per problem runs the whole schedule.  Thread t owns the edges t,
//                 t + 256, ...; a build pass reduces the 21 + 6 + 1 values of H, b and the robust
//                 chi2, a trial pass one value.  After a reduction every thread holds the same
//                 bits, so the 6 x 6 solve, the update and every decision of the schedule are
//                 taken redundantly by all threads: no broadcast, and branches are uniform.
//                 Every loop has a static bound (4 rounds, its[r] iterations, 10 trials,
//                 ceil(n / 256) edges).  The flags live in LDS, the edges' chi2 of their last
//                 evaluation in scratch, as the classification reads them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <string>

#include "../../include/orb_abi.h"
#include "orb_g2o_math.h"
#include "orb_internal.h"

namespace {

int fail(int code, const std::string& msg) { return orb_internal_set_error(code, msg); }

constexpr int PO_MAX_CAP = 8192;
constexpr int PO_THREADS = 256;
constexpr int PO_WAVES = PO_THREADS / 64;
static_assert(PO_WAVES == G2O_WAVES, "block_sum and compact_slot are written for this many waves");
constexpr int PO_NV = 7;   // X Y Z u v invSigma2 | chi2 of the last evaluation
constexpr int PO_NACC = 28;  // 21 of H (upper triangle), 6 of b, the robust chi2

struct PoArgs {
    // batch form: extractor records of frame frame_of[s]; mp_pos / has_mp rows per problem
    const orb_keypoint_t* kps;
    const int32_t* kcounts;
    const int32_t* frame_of;
    // host form (n_direct >= 0): one problem, obs n x 2 and inv_sigma2 n given directly
    const float* obs;
    const float* inv_sigma2;
    int n_direct;
    const float* mp_pos;
    const uint8_t* has_mp;
    float inv_level_sigma2[ORB_MAX_VIEW_LEVELS];
    int nlevels;
    double fx, fy, cx, cy;
    double delta;  // the Huber delta, (double)(float)sqrt(5.991) (Optimizer.cc:189)
    const float* pose_in;
    float* pose_out;
    double* pose_out64;
    uint8_t* outlier;
    int32_t* n_inliers;
    orb_pose_opt_info_t* info;
    // scratch
    double* soa;     // S x PO_NV x cap
    int32_t* index;  // S x cap
    int32_t* n;      // S
    int cap, S;
};

__global__ void __launch_bounds__(PO_THREADS) k_po_prepare(PoArgs a) {
    __shared__ int s_wtot[PO_WAVES];
    const int s = blockIdx.x, tid = threadIdx.x;
    const bool direct = a.n_direct >= 0;
    const int f = direct ? 0 : a.frame_of[s];
    // an index past the frame's count is no edge, so no read leaves the batch arrays
    const int n_row = direct ? a.n_direct : min(max(a.kcounts[f], 0), a.cap);
    uint8_t* outl = a.outlier + (size_t)s * a.cap;
    for (int i = tid; i < (direct ? a.n_direct : a.cap); i += PO_THREADS) outl[i] = 0;
    double* q = a.soa + (size_t)s * PO_NV * a.cap;
    int32_t* index = a.index + (size_t)s * a.cap;
    const size_t row = (size_t)s * a.cap;
    int base = 0;
    for (int i0 = 0; i0 < n_row; i0 += PO_THREADS) {
        const int i = i0 + tid;
        const bool ok = i < n_row && (a.has_mp ? a.has_mp[row + i] != 0 : true);
        const int o = compact_slot(ok, s_wtot, base);
        if (o >= 0) {
            float u, v, is2;
            if (direct) {
                u = a.obs[2 * i], v = a.obs[2 * i + 1], is2 = a.inv_sigma2[i];
            } else {
                const orb_keypoint_t& kp = a.kps[(size_t)f * a.cap + i];
                u = kp.x, v = kp.y;
                is2 = a.inv_level_sigma2[min(max(kp.octave, 0), a.nlevels - 1)];
            }
            const float* X = a.mp_pos + 3 * (row + i);
            q[o] = (double)X[0], q[a.cap + o] = (double)X[1], q[2 * a.cap + o] = (double)X[2];
            q[3 * a.cap + o] = (double)u, q[4 * a.cap + o] = (double)v, q[5 * a.cap + o] = (double)is2;
            index[o] = i;
        }
    }
    if (tid == 0) a.n[s] = base;
}

struct Cam {
    double fx, fy, cx, cy;
};

// computeError (obs - cam_project(T.map(X))) and chi2 = e' * (invSigma2 I) * e; Xc for the Jacobian
__device__ __forceinline__ double edge_chi2(const Pose& T, const Cam& c, const double* q, int cap, int e, double* err,
                                            double* Xc) {
    const double X[3] = {q[e], q[cap + e], q[2 * cap + e]};
    double r[3];
    rotate(T.q, X, r);
#pragma unroll
    for (int k = 0; k < 3; ++k) Xc[k] = r[k] + T.t[k];
    err[0] = q[3 * cap + e] - ((Xc[0] / Xc[2]) * c.fx + c.cx);
    err[1] = q[4 * cap + e] - ((Xc[1] / Xc[2]) * c.fy + c.cy);
    const double s = q[5 * cap + e];
    return err[0] * (s * err[0]) + err[1] * (s * err[1]);
}

__global__ void __launch_bounds__(PO_THREADS) k_po_solve(PoArgs a) {
    __shared__ double s_red[PO_WAVES][PO_NACC];
    __shared__ uint8_t s_flag[PO_MAX_CAP];  // mvbOutlier of the edges = their level
    __shared__ int s_cnt[2];                // nBad, edges left in the optimisation
    const int s = blockIdx.x, tid = threadIdx.x, cap = a.cap;
    const int n = min(max(a.n[s], 0), min(cap, PO_MAX_CAP));
    double* q = a.soa + (size_t)s * PO_NV * cap;
    double* chi2_e = q + (size_t)6 * cap;
    const Cam cam{a.fx, a.fy, a.cx, a.cy};
    const double delta = a.delta;
    const double dsqr = delta * delta;
    for (int e = tid; e < n; e += PO_THREADS) s_flag[e] = 0;
    if (tid == 0) s_cnt[0] = 0, s_cnt[1] = n;
    Pose T;
    {  // Converter::toSE3Quat
        const float* p = a.pose_in + (size_t)s * 12;
        double R[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = (double)p[k];
        quat_from_matrix(R, T.q);
#pragma unroll
        for (int k = 0; k < 3; ++k) T.t[k] = (double)p[9 + k];
        normalize_rotation(T);
    }
    __syncthreads();
    const float th[4] = {9.210f, 7.378f, 5.991f, 5.991f};
    const int its[4] = {10, 10, 7, 5};
    int iters[4] = {0, 0, 0, 0};
    int trials = 0, rounds = 0, n_bad = 0;
    double lambda = -1., ni = 2., last_chi = 0.;
    double x[6] = {0, 0, 0, 0, 0, 0};
    for (int r = 0; r < 4; ++r) {
        const int n_active = s_cnt[1];
        int bad_steps = 0;
        bool stop = n_active <= 0;  // no level-0 edge: optimize() returns at once
        for (int it = 0; it < its[r]; ++it) {
            if (stop) break;
            ++iters[r];
            // computeActiveErrors + activeRobustChi2 + buildSystem at T
            double acc[PO_NACC];
#pragma unroll
            for (int k = 0; k < PO_NACC; ++k) acc[k] = 0.;
            for (int e = tid; e < n; e += PO_THREADS) {
                if (s_flag[e]) continue;
                double err[2], Xc[3], rho0, rho1, J[12];
                const double c2 = edge_chi2(T, cam, q, cap, e, err, Xc);
                chi2_e[e] = c2;
                huber(c2, delta, dsqr, &rho0, &rho1);
                const double X = Xc[0], Y = Xc[1], Z = Xc[2], z_2 = Z * Z;
                J[0] = X * Y / z_2 * cam.fx;
                J[1] = -(1 + (X * X / z_2)) * cam.fx;
                J[2] = Y / Z * cam.fx;
                J[3] = -1. / Z * cam.fx;
                J[4] = 0;
                J[5] = X / z_2 * cam.fx;
                J[6] = (1 + Y * Y / z_2) * cam.fy;
                J[7] = -X * Y / z_2 * cam.fy;
                J[8] = -X / Z * cam.fy;
                J[9] = 0;
                J[10] = -1. / Z * cam.fy;
                J[11] = Y / z_2 * cam.fy;
                const double sg = q[5 * cap + e];
                const double w = sg * rho1;  // weightedOmega = rho[1] * omega
                const double r0 = (-(sg * err[0])) * rho1, r1 = (-(sg * err[1])) * rho1;
                int c = 0;
#pragma unroll
                for (int j = 0; j < 6; ++j)
#pragma unroll
                    for (int k = j; k < 6; ++k) acc[c++] += (J[j] * w) * J[k] + (J[6 + j] * w) * J[6 + k];
#pragma unroll
                for (int j = 0; j < 6; ++j) acc[21 + j] += J[j] * r0 + J[6 + j] * r1;
                acc[27] += rho0;
            }
            block_sum<PO_NACC>(acc, s_red);
            // acc stays as the system: H's upper triangle in acc[0..21), b in acc[21..27)
            const double* b = acc + 21;
            double cur = acc[27];
            const double ini = cur;
            if (it == 0) {
                lambda = lm_lambda_init<6>(acc);
                ni = 2.;
                bad_steps = 0;
            }
            double rho = 0;
            int qmax = 0;
            bool again = true;
            for (int tr = 0; tr < 10; ++tr) {
                if (!again) break;
                const Pose backup = T;
                double A[36];
                lm_damped<6>(acc, lambda, A);
                const bool ok2 = ldlt<6>(A, b, x);
                T = exp_update(x, T);
                double t1[1] = {0.};
                for (int e = tid; e < n; e += PO_THREADS) {
                    if (s_flag[e]) continue;
                    double err[2], Xc[3], rho0, rho1;
                    const double c2 = edge_chi2(T, cam, q, cap, e, err, Xc);
                    chi2_e[e] = c2;
                    huber(c2, delta, dsqr, &rho0, &rho1);
                    t1[0] += rho0;
                }
                block_sum<1>(t1, s_red);
                const double temp = ok2 ? t1[0] : DBL_MAX;
                rho = (cur - temp) / lm_scale<6>(x, lambda, b);
                if (lm_accept(rho, temp, lambda, ni)) cur = temp;
                else T = backup;
                ++qmax;
                ++trials;
                again = rho < 0 && qmax < 10;  // a NaN rho leaves the loop
            }
            last_chi = cur;
            stop = lm_stop(qmax, rho, ini, cur, bad_steps);
        }
        // classification (Optimizer.cc:251-272)
        __syncthreads();
        if (tid == 0) s_cnt[0] = 0, s_cnt[1] = 0;
        __syncthreads();
        const double thr = (double)th[r];
        int bad = 0, act = 0;
        for (int e = tid; e < n; e += PO_THREADS) {
            if (s_flag[e]) {
                double err[2], Xc[3];
                chi2_e[e] = edge_chi2(T, cam, q, cap, e, err, Xc);
            }
            const double c2 = chi2_e[e];
            if (c2 > thr) {
                s_flag[e] = 1, ++bad;
            } else if (c2 <= thr) {
                s_flag[e] = 0;
            }
            act += s_flag[e] ? 0 : 1;
        }
        if (bad) atomicAdd(&s_cnt[0], bad);
        if (act) atomicAdd(&s_cnt[1], act);
        __syncthreads();
        n_bad = s_cnt[0];
        rounds = r + 1;
        if (n < 10) break;  // optimizer.edges().size() < 10
    }
    const int32_t* index = a.index + (size_t)s * cap;
    uint8_t* outl = a.outlier + (size_t)s * cap;
    for (int e = tid; e < n; e += PO_THREADS) outl[index[e]] = s_flag[e];
    if (tid == 0) {
        double M[12];
        matrix_from_quat(T.q, M);
        for (int k = 0; k < 3; ++k) M[9 + k] = T.t[k];
        for (int k = 0; k < 12; ++k) {
            if (a.pose_out64) a.pose_out64[(size_t)s * 12 + k] = M[k];
            a.pose_out[(size_t)s * 12 + k] = (float)M[k];
        }
        a.n_inliers[s] = n - n_bad;
        if (a.info) {
            orb_pose_opt_info_t I;
            I.n_initial = n, I.n_bad = n_bad, I.rounds = rounds;
            for (int k = 0; k < 4; ++k) I.iterations[k] = iters[k];
            I.trials = trials, I.lambda = lambda, I.chi2 = last_chi;
            a.info[s] = I;
        }
    }
}

int launch(PoArgs a, hipStream_t st) {
    a.delta = (double)(float)std::sqrt(5.991);
    hipLaunchKernelGGL(k_po_prepare, dim3(a.S), dim3(PO_THREADS), 0, st, a);
    ORB_HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_po_solve, dim3(a.S), dim3(PO_THREADS), 0, st, a);
    ORB_HIPCHK(hipGetLastError());
    return ORB_OK;
}

}  // namespace

extern "C" {

int orb_pose_optimization(int n, const float* p3d, const float* obs, const float* inv_sigma2, const uint8_t* has_mp,
                          float fx, float fy, float cx, float cy, const float* pose_in, float* pose_out,
                          double* pose_out_f64, uint8_t* outlier, int32_t* n_inliers, orb_pose_opt_info_t* info,
                          int device) {
    const char* who = "pose_optimization";
    if (n < 0 || (n && (!p3d || !obs || !inv_sigma2 || !outlier)) || !pose_in || !pose_out || !n_inliers)
        return fail(ORB_EINVAL, std::string(who) + ": bad arguments");
    if (n > PO_MAX_CAP) return fail(ORB_ENOTSUP, std::string(who) + ": more than 8192 keypoints");
    const float K[4] = {fx, fy, cx, cy};
    if (int r = orb_check_camera(who, "", K)) return r;
    for (int k = 0; k < 12; ++k)
        if (!std::isfinite(pose_in[k]))
            return fail(ORB_EINVAL, std::string(who) + ": pose_in[" + std::to_string(k) + "] is not finite");
    const int cap = std::max(n, 1);
    const size_t N = (size_t)n;
    OrbStagePlan P;
    const auto rP = P.in<float>(N * 3), rO = P.in<float>(N * 2), rS = P.in<float>(N);
    const auto rH = P.in<uint8_t>(N);
    const auto rT = P.in<float>(12);
    const auto r64 = P.out<double>(12);
    const auto rI = P.out<orb_pose_opt_info_t>(1);
    const auto r32 = P.out<float>(12);
    const auto rN = P.out<int32_t>(1);
    const auto rF = P.out<uint8_t>(cap);
    const auto rSoa = P.scratch<double>((size_t)PO_NV * cap);
    const auto rIdx = P.scratch<int32_t>(cap), rCnt = P.scratch<int32_t>(1);
    OrbHostCall call(P, device);
    if (call.err) return call.err;
    PoArgs a{};
    a.n_direct = n;
    a.mp_pos = call.send(rP, p3d);
    a.obs = call.send(rO, obs);
    a.inv_sigma2 = call.send(rS, inv_sigma2);
    a.has_mp = has_mp ? call.send(rH, has_mp) : nullptr;
    a.nlevels = 1;
    a.fx = (double)fx, a.fy = (double)fy, a.cx = (double)cx, a.cy = (double)cy;
    a.pose_in = call.send(rT, pose_in);
    a.pose_out64 = call.dev(r64);
    a.info = call.dev(rI);
    a.pose_out = call.dev(r32);
    a.n_inliers = call.dev(rN);
    a.outlier = call.dev(rF);
    a.soa = call.dev(rSoa);
    a.index = call.dev(rIdx);
    a.n = call.dev(rCnt);
    a.cap = cap;
    a.S = 1;
    if (int r = call.upload()) return r;
    if (int r = call.finish(launch(a, call.stream()), hipSuccess, std::string(who) + ": ")) return r;
    call.get(r32, pose_out);
    call.get(r64, pose_out_f64);
    call.get(rI, info);
    call.get(rN, n_inliers);
    call.get(rF, outlier, N);
    return ORB_OK;
}

int orb_pose_optimization_batch_device(const orb_keypoint_t* d_kps, const int32_t* d_counts, int cap, int S,
                                       const int32_t* d_frame_of, const float* d_mp_pos, const uint8_t* d_has_mp,
                                       const float* inv_level_sigma2, int n_levels, const float* K4,
                                       const float* d_pose_in, float* d_pose_out, double* d_pose_out_f64,
                                       uint8_t* d_outlier, int32_t* d_n_inliers, orb_pose_opt_info_t* d_info,
                                       void* stream) {
    const char* who = "pose_optimization_batch";
    if (S < 0 || cap <= 0 || !K4) return fail(ORB_EINVAL, std::string(who) + ": bad arguments");
    if (cap > PO_MAX_CAP) return fail(ORB_ENOTSUP, std::string(who) + ": more than 8192 keypoints per frame");
    if (S > 65535) return fail(ORB_ENOTSUP, std::string(who) + ": more than 65535 problems per call");
    if (!inv_level_sigma2 || n_levels < 1 || n_levels > ORB_MAX_VIEW_LEVELS)
        return fail(ORB_EINVAL, std::string(who) + ": n_levels must be in [1, 16]");
    if (int r = orb_check_camera(who, "", K4)) return r;
    if (S == 0) return ORB_OK;
    if (!d_kps || !d_counts || !d_frame_of || !d_mp_pos || !d_has_mp || !d_pose_in || !d_pose_out || !d_outlier ||
        !d_n_inliers)
        return fail(ORB_EINVAL, std::string(who) + ": bad arguments");
    PoArgs a{};
    a.kps = d_kps;
    a.kcounts = d_counts;
    a.frame_of = d_frame_of;
    a.n_direct = -1;
    a.mp_pos = d_mp_pos;
    a.has_mp = d_has_mp;
    std::memcpy(a.inv_level_sigma2, inv_level_sigma2, (size_t)n_levels * 4);
    a.nlevels = n_levels;
    a.fx = (double)K4[0], a.fy = (double)K4[1], a.cx = (double)K4[2], a.cy = (double)K4[3];
    a.pose_in = d_pose_in;
    a.pose_out = d_pose_out;
    a.pose_out64 = d_pose_out_f64;
    a.outlier = d_outlier;
    a.n_inliers = d_n_inliers;
    a.info = d_info;
    a.cap = cap;
    a.S = S;
    hipStream_t st = (hipStream_t)stream;
    void* tmp = nullptr;
    if (int r = orb_scratch_alloc(&tmp, st, std::string(who) + ": scratch: ", [&](OrbLayout& L) {
            a.soa = L.take<double>((size_t)S * PO_NV * cap);
            a.index = L.take<int32_t>((size_t)S * cap);
            a.n = L.take<int32_t>(S);
        }))
        return r;
    const int r = launch(a, st);
    (void)hipFreeAsync(tmp, st);
    return r;
}

}  // extern "C"
