// orb_localba.hip — Optimizer::LocalBundleAdjustment on the GPU (part of liborb_hip.so).
//
// The windowed bundle adjustment of LocalMapping::Run (reference src/Optimizer.cc:287-536, called from
// LocalMapping.cc:84), with the parts of g2o it runs restated in double:
//   graph           Optimizer.cc:356-447, handed over as flat arrays: keyframes (local first, then
//                   fixed), points, one edge per observation, the edges of a point contiguous
//   edge            EdgeSE3ProjectXYZ::computeError / linearizeOplus, both Jacobians
//                   (types_six_dof_expmap.h:172-183, .cpp:384-428)
//   quadratic form  base_binary_edge.hpp:91-113 with RobustKernelHuber
//   block solver    BlockSolver::buildSystem / setLambda / solve with marginalised points
//                   (block_solver.hpp:354-486, 502-589); the reduced system is solved by a dense
//                   unpivoted L L' in place of CHOLMOD, refused on a pivot that is not positive and finite
//   Levenberg       optimization_algorithm_levenberg.cpp:61-189 over poses and points
//   two rounds      Optimizer.cc:449-515 with MapPoint::EraseObservation's count (MapPoint.cc:71-91)
// The SE3 state, exp(x) * T, the Huber kernel, the Levenberg bookkeeping and the workgroup sum are
// those of csrc/orb_g2o_math.h.
//
// Arithmetic: all f64, the TU built -ffp-contract=off.  Every sum has one owner and one written order
// (a point's thread over its edges, a keyframe's wave over its edge list, a block's wave over the
// points in order, block_sum for the two scalars), so a call gives the same bits on every run.  There
// is no floating-point atomic, no workgroup waits for another, and every loop is bounded by a size
// that is fixed before it starts.
//
//   k_lba_prepare  one workgroup per problem: validates, numbers the free keyframes, widens to doubles,
//                  builds the points' edge ranges and masks and the free keyframes' edge lists.
//   k_lba_solve    one workgroup per problem runs both rounds: build (thread per point, wave per free
//                  keyframe), then per trial Dinv, the Schur complement (wave per 6 x 6 block), the
//                  panelled Cholesky through LDS, the substitutions, the update and the trial error.
//                  After a reduction every thread holds the same bits and takes every decision itself.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <string>

#include "../../include/orb_abi.h"
#include "orb_g2o_math.h"
#include "orb_internal.h"

namespace {

int fail(int code, const std::string& msg) { return orb_internal_set_error(code, msg); }

constexpr int LBA_MAX_FREE_KF = ORB_LBA_MAX_FREE_KF;
static_assert(LBA_MAX_FREE_KF == 64, "one 64-bit mask per point names its free keyframes");
constexpr int LBA_THREADS = 256;
constexpr int LBA_WAVES = LBA_THREADS / 64;
static_assert(LBA_WAVES == G2O_WAVES, "block_sum and compact_slot are written for this many waves");
constexpr int LBA_MAX_N = 6 * LBA_MAX_FREE_KF;  // columns of the reduced system
constexpr int LBA_PANEL = 12;                   // Cholesky panel: the columns of two keyframes
constexpr int LBA_PT = 21;  // per point: Hll (00 01 02 11 12 22), b_l 3, Dinv 6, Dinv b_l 3, x_l 3
constexpr int LBA_KF = 27;  // per free keyframe: Hpp's upper triangle 21, b_p 6

struct LbaArgs {
    int S;
    const int32_t *kf_off, *pt_off, *edge_off;
    int n_kf_total, n_pt_total, n_edge_total;
    const float *kf_pose, *kf_K;
    const uint8_t* kf_fixed;
    const float* pt_pos;
    const int32_t* pt_nobs;
    const int32_t *edge_pt, *edge_kf;
    const float *edge_obs, *edge_s;
    float* kf_pose_out;
    double* kf_pose_out64;
    float* pt_pos_out;
    double* pt_pos_out64;
    uint8_t *edge_erased, *pt_bad;
    orb_local_ba_info_t* info;
    double delta;  // the Huber delta, (double)(float)sqrt(5.991) (Optimizer.cc:397)
    // scratch, concatenated as the inputs are
    int32_t *status, *n_free;  // S
    double *kf_T, *kf_Tb;      // n_kf x 7: q t, and the trial's backup
    int32_t* kf_slot;          // n_kf: the free keyframe's number, -1 fixed
    double *pt_X, *pt_Xb;      // n_pt x 3
    double* pt_sys;            // n_pt x LBA_PT
    int32_t *pt_e0, *pt_e1, *pt_cnt;
    unsigned long long* pt_mask;
    uint8_t *pt_act, *pt_state;
    double* e_obs;   // per problem SoA: u | v | invSigma2
    double* e_chi2;  // the chi2 of the edge's last computeError
    double* e_hpl;   // n_edge x 18: the edge's 6 x 3 block of Hpl
    int32_t* e_slot;
    uint8_t* e_state;  // 0 in the optimisation, else the round after which it was erased
    int32_t* csr;      // n_edge: the edges of each free keyframe, ascending
    int32_t* csr_off;  // S x (LBA_MAX_FREE_KF + 1)
    int32_t* slot_kf;  // S x LBA_MAX_FREE_KF
    double* hpp;       // S x LBA_MAX_FREE_KF x LBA_KF
    double* sys;       // S x LBA_MAX_N x LBA_MAX_N: the reduced system, lower triangle, then L
    double* bs;        // S x LBA_MAX_N
};

struct Span {
    int k0, nk, p0, np, e0, ne;
    bool ok;
};

__device__ __forceinline__ Span span_of(const LbaArgs& a, int s) {
    Span w;
    const int k0 = a.kf_off[s], k1 = a.kf_off[s + 1], p0 = a.pt_off[s], p1 = a.pt_off[s + 1];
    const int e0 = a.edge_off[s], e1 = a.edge_off[s + 1];
    w.ok = k0 >= 0 && k0 <= k1 && k1 <= a.n_kf_total && p0 >= 0 && p0 <= p1 && p1 <= a.n_pt_total && e0 >= 0 &&
           e0 <= e1 && e1 <= a.n_edge_total;
    w.k0 = k0, w.nk = k1 - k0, w.p0 = p0, w.np = p1 - p0, w.e0 = e0, w.ne = e1 - e0;
    return w;
}

__global__ void __launch_bounds__(LBA_THREADS) k_lba_prepare(LbaArgs a) {
    __shared__ int s_wtot[LBA_WAVES];
    __shared__ int s_bad;
    __shared__ int s_cnt[LBA_MAX_FREE_KF + 1];
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const Span w = span_of(a, s);
    if (!w.ok) {  // offsets that leave the arrays: nothing of this problem is read
        if (tid == 0) {
            a.status[s] = ORB_EINVAL, a.n_free[s] = 0;
            if (a.info) a.info[s].status = ORB_EINVAL, a.info[s].n_free_kf = 0;
        }
        return;
    }
    if (tid == 0) s_bad = 0;
    // the free keyframes numbered in index order; SE3Quat(R, t) + normalizeRotation
    int n_free = 0;
    for (int i0 = 0; i0 < w.nk; i0 += LBA_THREADS) {
        const int i = i0 + tid;
        const bool fr = i < w.nk && a.kf_fixed[w.k0 + i] == 0;
        const int o = compact_slot(fr, s_wtot, n_free);
        if (i < w.nk) {
            a.kf_slot[w.k0 + i] = o >= 0 && o < LBA_MAX_FREE_KF ? o : -1;
            if (o >= 0 && o < LBA_MAX_FREE_KF) a.slot_kf[s * LBA_MAX_FREE_KF + o] = i;
            const float* p = a.kf_pose + (size_t)(w.k0 + i) * 12;
            double R[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) R[k] = (double)p[k];
            Pose T;
            quat_from_matrix(R, T.q);
#pragma unroll
            for (int k = 0; k < 3; ++k) T.t[k] = (double)p[9 + k];
            normalize_rotation(T);
            double* g = a.kf_T + (size_t)(w.k0 + i) * 7;
#pragma unroll
            for (int k = 0; k < 4; ++k) g[k] = T.q[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) g[4 + k] = T.t[k];
        }
    }
    for (int p = tid; p < w.np; p += LBA_THREADS) {
#pragma unroll
        for (int k = 0; k < 3; ++k) a.pt_X[(size_t)(w.p0 + p) * 3 + k] = (double)a.pt_pos[(size_t)(w.p0 + p) * 3 + k];
        a.pt_e0[w.p0 + p] = 0, a.pt_e1[w.p0 + p] = 0;
        a.pt_cnt[w.p0 + p] = a.pt_nobs[w.p0 + p];
        a.pt_state[w.p0 + p] = 0;
    }
    __syncthreads();
    // the edges: indices in range, points ascending; each point's range
    const int32_t* ept = a.edge_pt + w.e0;
    const int32_t* ekf = a.edge_kf + w.e0;
    double* eo = a.e_obs + (size_t)w.e0 * 3;
    for (int e = tid; e < w.ne; e += LBA_THREADS) {
        const int p = ept[e], i = ekf[e];
        bool bad = p < 0 || p >= w.np || i < 0 || i >= w.nk;
        if (!bad && e > 0 && p < ept[e - 1]) bad = true;
        if (!bad) {
            if (e == 0 || ept[e - 1] != p) a.pt_e0[w.p0 + p] = e;
            if (e == w.ne - 1 || ept[e + 1] != p) a.pt_e1[w.p0 + p] = e + 1;
        }
        eo[e] = (double)a.edge_obs[(size_t)(w.e0 + e) * 2];
        eo[w.ne + e] = (double)a.edge_obs[(size_t)(w.e0 + e) * 2 + 1];
        eo[2 * w.ne + e] = (double)a.edge_s[w.e0 + e];
        a.e_slot[w.e0 + e] = bad ? -1 : a.kf_slot[w.k0 + i];
        a.e_state[w.e0 + e] = 0;
        if (bad) s_bad = 1;
    }
    __syncthreads();
    if (!s_bad) {
        // a point's edges: no more than its observations, no keyframe twice; its mask
        for (int p = tid; p < w.np; p += LBA_THREADS) {
            const int b0 = a.pt_e0[w.p0 + p], b1 = a.pt_e1[w.p0 + p];
            bool bad = b1 - b0 > a.pt_nobs[w.p0 + p] || b1 - b0 > w.nk;  // more edges than keyframes: one twice
            unsigned long long m = 0;
            if (!bad)
                for (int x = b0; x < b1; ++x) {
                    for (int y = x + 1; y < b1; ++y) bad |= ekf[x] == ekf[y];
                    const int sl = a.e_slot[w.e0 + x];
                    if (sl >= 0) m |= 1ull << sl;
                }
            a.pt_mask[w.p0 + p] = m;
            if (bad) s_bad = 1;
        }
    }
    __syncthreads();
    const int st = n_free == 0 || n_free > LBA_MAX_FREE_KF ? ORB_ENOTSUP : s_bad ? ORB_EINVAL : ORB_OK;
    if (tid == 0) {
        a.status[s] = st, a.n_free[s] = n_free;
        if (a.info) {
            orb_local_ba_info_t I = {};
            I.status = st, I.n_free_kf = n_free;
            a.info[s] = I;
        }
    }
    if (st != ORB_OK) return;
    // the edge list of each free keyframe, ascending: a wave per keyframe counts, then fills
    for (int k = tid; k <= LBA_MAX_FREE_KF; k += LBA_THREADS) s_cnt[k] = 0;
    __syncthreads();
    for (int sl = wave; sl < n_free; sl += LBA_WAVES) {
        int c = 0;
        for (int e0 = 0; e0 < w.ne; e0 += 64) {
            const int e = e0 + lane;
            c += __popcll(__ballot(e < w.ne && a.e_slot[w.e0 + e] == sl));
        }
        if (lane == 0) s_cnt[sl + 1] = c;
    }
    __syncthreads();
    if (tid == 0)
        for (int k = 0; k < n_free; ++k) s_cnt[k + 1] += s_cnt[k];
    __syncthreads();
    for (int k = tid; k <= n_free; k += LBA_THREADS) a.csr_off[s * (LBA_MAX_FREE_KF + 1) + k] = s_cnt[k];
    for (int sl = wave; sl < n_free; sl += LBA_WAVES) {
        int c = s_cnt[sl];
        for (int e0 = 0; e0 < w.ne; e0 += 64) {
            const int e = e0 + lane;
            const bool mine = e < w.ne && a.e_slot[w.e0 + e] == sl;
            const unsigned long long bal = __ballot(mine);
            if (mine) a.csr[w.e0 + c + __popcll(bal & ((1ull << lane) - 1ull))] = e;
            c += __popcll(bal);
        }
    }
}

__device__ __forceinline__ Pose load_pose(const double* g) {
    Pose T;
#pragma unroll
    for (int k = 0; k < 4; ++k) T.q[k] = g[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) T.t[k] = g[4 + k];
    return T;
}

__device__ __forceinline__ void store_pose(double* g, const Pose& T) {
#pragma unroll
    for (int k = 0; k < 4; ++k) g[k] = T.q[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) g[4 + k] = T.t[k];
}

struct Cam {
    double fx, fy, cx, cy;
};

__device__ __forceinline__ Cam load_cam(const float* K) {
    return Cam{(double)K[0], (double)K[1], (double)K[2], (double)K[3]};
}

// computeError (obs - cam_project(T.map(X))) and chi2 = e' * (invSigma2 I) * e; Xc for the Jacobians
__device__ __forceinline__ double edge_chi2(const Pose& T, const Cam& c, const double* X, double u, double v, double sg,
                                            double* err, double* Xc) {
    double r[3];
    rotate(T.q, X, r);
#pragma unroll
    for (int k = 0; k < 3; ++k) Xc[k] = r[k] + T.t[k];
    err[0] = u - ((Xc[0] / Xc[2]) * c.fx + c.cx);
    err[1] = v - ((Xc[1] / Xc[2]) * c.fy + c.cy);
    return err[0] * (sg * err[0]) + err[1] * (sg * err[1]);
}

// _jacobianOplusXi: -1/z * tmp * R (2 x 3), the terms with tmp's two zeros left out
__device__ __forceinline__ void jacobian_point(const Pose& T, const Cam& c, const double* Xc, double* A) {
    const double x = Xc[0], y = Xc[1], z = Xc[2];
    double R[9];
    matrix_from_quat(T.q, R);
    const double m = -1. / z;
    const double m00 = m * c.fx, m02 = m * (-x / z * c.fx), m11 = m * c.fy, m12 = m * (-y / z * c.fy);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        A[j] = m00 * R[j] + m02 * R[6 + j];
        A[3 + j] = m11 * R[3 + j] + m12 * R[6 + j];
    }
}

// _jacobianOplusXj (2 x 6)
__device__ __forceinline__ void jacobian_pose(const Cam& c, const double* Xc, double* B) {
    const double x = Xc[0], y = Xc[1], z = Xc[2], z_2 = z * z;
    B[0] = x * y / z_2 * c.fx;
    B[1] = -(1 + (x * x / z_2)) * c.fx;
    B[2] = y / z * c.fx;
    B[3] = -1. / z * c.fx;
    B[4] = 0;
    B[5] = x / z_2 * c.fx;
    B[6] = (1 + y * y / z_2) * c.fy;
    B[7] = -x * y / z_2 * c.fy;
    B[8] = -x / z * c.fy;
    B[9] = 0;
    B[10] = -1. / z * c.fy;
    B[11] = y / z_2 * c.fy;
}

// std::max(v, m) over the workgroup; every thread gets the same bits (s_red is block_sum's)
__device__ __forceinline__ double block_max(double v, double (*s_red)[2]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double o = __shfl_xor(v, m);
        v = o < v ? v : o;
    }
    __syncthreads();
    if (lane == 0) s_red[wave][0] = v;
    __syncthreads();
    double r = s_red[0][0];
#pragma unroll
    for (int k = 1; k < LBA_WAVES; ++k) r = s_red[k][0] < r ? r : s_red[k][0];
    return r;
}

__global__ void __launch_bounds__(LBA_THREADS) k_lba_solve(LbaArgs a) {
    __shared__ double s_red[LBA_WAVES][2];
    __shared__ double s_panel[LBA_MAX_N * LBA_PANEL];
    __shared__ double s_x[LBA_MAX_N], s_b[LBA_MAX_N], s_y[LBA_MAX_N];
    __shared__ uint8_t s_kact[LBA_MAX_FREE_KF];
    __shared__ int s_cnt[3];
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (a.status[s] != ORB_OK) return;
    const Span w = span_of(a, s);
    const int L = min(max(a.n_free[s], 0), LBA_MAX_FREE_KF), N = 6 * L;
    const double delta = a.delta, dsqr = delta * delta;
    const int32_t* ept = a.edge_pt + w.e0;
    const int32_t* ekf = a.edge_kf + w.e0;
    const double* eo = a.e_obs + (size_t)w.e0 * 3;
    double* chi2_e = a.e_chi2 + w.e0;
    double* hpl = a.e_hpl + (size_t)w.e0 * 18;
    const int32_t* e_slot = a.e_slot + w.e0;
    uint8_t* e_state = a.e_state + w.e0;
    const int32_t* csr = a.csr + w.e0;
    const int32_t* csr_off = a.csr_off + s * (LBA_MAX_FREE_KF + 1);
    const int32_t* slot_kf = a.slot_kf + s * LBA_MAX_FREE_KF;
    double* kfT = a.kf_T + (size_t)w.k0 * 7;
    double* kfTb = a.kf_Tb + (size_t)w.k0 * 7;
    const float* kfK = a.kf_K + (size_t)w.k0 * 4;
    const int32_t* kf_slot = a.kf_slot + w.k0;
    double* ptX = a.pt_X + (size_t)w.p0 * 3;
    double* ptXb = a.pt_Xb + (size_t)w.p0 * 3;
    double* pts = a.pt_sys + (size_t)w.p0 * LBA_PT;
    const int32_t* pe0 = a.pt_e0 + w.p0;
    const int32_t* pe1 = a.pt_e1 + w.p0;
    int32_t* pcnt = a.pt_cnt + w.p0;
    unsigned long long* pmask = a.pt_mask + w.p0;
    uint8_t* pact = a.pt_act + w.p0;
    uint8_t* pstate = a.pt_state + w.p0;
    double* hpp = a.hpp + (size_t)s * LBA_MAX_FREE_KF * LBA_KF;
    double* A = a.sys + (size_t)s * LBA_MAX_N * LBA_MAX_N;  // N x N, row stride N
    double* bs = a.bs + (size_t)s * LBA_MAX_N;

    double lambda = -1., ni = 2.;
    for (int r = 0; r < 2; ++r) {
        orb_local_ba_round_t Ir = {};
        const int its = r == 0 ? 5 : 10;  // optimize(5), optimize(10)
        // initializeOptimization(): the vertices that still have an edge
        __syncthreads();
        if (tid < 3) s_cnt[tid] = 0;
        for (int k = tid; k < LBA_MAX_N; k += LBA_THREADS) s_x[k] = 0.;
        __syncthreads();
        {
            int n_e = 0, n_p = 0;
            #pragma unroll 1
            for (int p = tid; p < w.np; p += LBA_THREADS) {
                unsigned long long m = 0;
                int act = 0;
                #pragma unroll 1
                for (int e = pe0[p]; e < pe1[p]; ++e) {
                    if (e_state[e]) continue;
                    ++act;
                    if (e_slot[e] >= 0) m |= 1ull << e_slot[e];
                }
                pmask[p] = m, pact[p] = act ? 1 : 0;
                n_e += act, n_p += act ? 1 : 0;
#pragma unroll
                for (int k = 0; k < 3; ++k) pts[(size_t)p * LBA_PT + 18 + k] = 0.;
            }
            if (n_e) atomicAdd(&s_cnt[0], n_e);
            if (n_p) atomicAdd(&s_cnt[1], n_p);
            if (tid < L) {
                int act = 0;
                for (int c = csr_off[tid]; c < csr_off[tid + 1]; ++c) act |= e_state[csr[c]] == 0;
                s_kact[tid] = (uint8_t)act;
                if (act) atomicAdd(&s_cnt[2], 1);
            }
        }
        __syncthreads();
        Ir.active_edges = s_cnt[0], Ir.active_points = s_cnt[1], Ir.active_keyframes = s_cnt[2];
        int bad_steps = 0;
        bool stop = Ir.active_edges <= 0;  // no vertex to optimise: optimize() returns at once
        for (int it = 0; it < its; ++it) {
            if (stop) break;
            ++Ir.iterations;
            // computeActiveErrors + activeRobustChi2 + buildSystem: a thread per point
            double red[2] = {0., 0.};  // the robust chi2; then the trial's scale and chi2
            double maxd = 0.;
            #pragma unroll 1
            for (int p = tid; p < w.np; p += LBA_THREADS) {
                if (!pact[p]) continue;
                double H[6] = {0, 0, 0, 0, 0, 0}, bl[3] = {0, 0, 0};
                const double X[3] = {ptX[3 * p], ptX[3 * p + 1], ptX[3 * p + 2]};
                #pragma unroll 1
                for (int e = pe0[p]; e < pe1[p]; ++e) {
                    if (e_state[e]) continue;
                    const int i = ekf[e];
                    const Pose T = load_pose(kfT + (size_t)i * 7);
                    const Cam cam = load_cam(kfK + (size_t)i * 4);
                    double err[2], Xc[3], rho0, rho1, Aj[6];
                    const double sg = eo[2 * w.ne + e];
                    const double c2 = edge_chi2(T, cam, X, eo[e], eo[w.ne + e], sg, err, Xc);
                    chi2_e[e] = c2;
                    huber(c2, delta, dsqr, &rho0, &rho1);
                    red[0] += rho0;
                    jacobian_point(T, cam, Xc, Aj);
                    const double wg = sg * rho1;  // weightedOmega = rho[1] * omega
                    const double r0 = (-(sg * err[0])) * rho1, r1 = (-(sg * err[1])) * rho1;
                    int c = 0;
#pragma unroll
                    for (int j = 0; j < 3; ++j)
#pragma unroll
                        for (int k = j; k < 3; ++k) H[c++] += (Aj[j] * wg) * Aj[k] + (Aj[3 + j] * wg) * Aj[3 + k];
#pragma unroll
                    for (int j = 0; j < 3; ++j) bl[j] += Aj[j] * r0 + Aj[3 + j] * r1;
                    if (e_slot[e] >= 0) {
                        double Bj[12];
                        jacobian_pose(cam, Xc, Bj);
#pragma unroll
                        for (int j = 0; j < 6; ++j)
#pragma unroll
                            for (int k = 0; k < 3; ++k)
                                hpl[(size_t)e * 18 + 3 * j + k] = (Bj[j] * wg) * Aj[k] + (Bj[6 + j] * wg) * Aj[3 + k];
                    }
                }
                double* g = pts + (size_t)p * LBA_PT;
#pragma unroll
                for (int k = 0; k < 6; ++k) g[k] = H[k];
#pragma unroll
                for (int k = 0; k < 3; ++k) g[6 + k] = bl[k];
                const double d0 = fabs(H[0]), d1 = fabs(H[3]), d2 = fabs(H[5]);
                maxd = d0 < maxd ? maxd : d0;
                maxd = d1 < maxd ? maxd : d1;
                maxd = d2 < maxd ? maxd : d2;
            }
            // Hpp and b_p: a wave per free keyframe over its edge list, the lanes strided, then a butterfly
            for (int sl = wave; sl < L; sl += LBA_WAVES) {
                if (!s_kact[sl]) continue;
                const int i = slot_kf[sl];
                const Pose T = load_pose(kfT + (size_t)i * 7);
                const Cam cam = load_cam(kfK + (size_t)i * 4);
                double acc[LBA_KF];
#pragma unroll
                for (int k = 0; k < LBA_KF; ++k) acc[k] = 0.;
                #pragma unroll 1
                for (int c = csr_off[sl] + lane; c < csr_off[sl + 1]; c += 64) {
                    const int e = csr[c];
                    if (e_state[e]) continue;
                    const int p = ept[e];
                    const double X[3] = {ptX[3 * p], ptX[3 * p + 1], ptX[3 * p + 2]};
                    double err[2], Xc[3], rho0, rho1, Bj[12];
                    const double sg = eo[2 * w.ne + e];
                    const double c2 = edge_chi2(T, cam, X, eo[e], eo[w.ne + e], sg, err, Xc);
                    huber(c2, delta, dsqr, &rho0, &rho1);
                    jacobian_pose(cam, Xc, Bj);
                    const double wg = sg * rho1;
                    const double r0 = (-(sg * err[0])) * rho1, r1 = (-(sg * err[1])) * rho1;
                    int k27 = 0;
#pragma unroll
                    for (int j = 0; j < 6; ++j)
#pragma unroll
                        for (int k = j; k < 6; ++k) acc[k27++] += (Bj[j] * wg) * Bj[k] + (Bj[6 + j] * wg) * Bj[6 + k];
#pragma unroll
                    for (int j = 0; j < 6; ++j) acc[21 + j] += Bj[j] * r0 + Bj[6 + j] * r1;
                }
#pragma unroll
                for (int k = 0; k < LBA_KF; ++k) {
#pragma unroll
                    for (int m = 32; m >= 1; m >>= 1) acc[k] += __shfl_xor(acc[k], m);
                }
                if (lane == 0) {
#pragma unroll
                    for (int k = 0; k < LBA_KF; ++k) hpp[sl * LBA_KF + k] = acc[k];
#pragma unroll
                    for (int j = 0, c = 0; j < 6; c += 6 - j, ++j) {
                        const double v = fabs(acc[c]);
                        maxd = v < maxd ? maxd : v;
                    }
                }
            }
            block_sum<1>(red, s_red);
            maxd = block_max(maxd, s_red);
            double cur = red[0];
            const double ini = cur;
            if (it == 0) {
                Ir.chi2_before = cur;
                lambda = 1e-5 * maxd;  // computeLambdaInit over poses and points
                ni = 2.;
                bad_steps = 0;
            }
            double rho = 0;
            int qmax = 0;
            bool again = true;
            for (int tr = 0; tr < 10; ++tr) {
                if (!again) break;
                // push(); setLambda on Hll; Dinv and Dinv b_l: a thread per point
                #pragma unroll 1
                for (int p = tid; p < w.np; p += LBA_THREADS) {
                    if (!pact[p]) continue;
                    double* g = pts + (size_t)p * LBA_PT;
#pragma unroll
                    for (int k = 0; k < 3; ++k) ptXb[3 * p + k] = ptX[3 * p + k];
                    // the full symmetric m of Matrix3d::inverse(): cofactors over the determinant
                    const double m0 = g[0] + lambda, m1 = g[1], m2 = g[2], m4 = g[3] + lambda, m5 = g[4], m8 = g[5] + lambda;
                    const double c00 = m4 * m8 - m5 * m5, c01 = m5 * m2 - m1 * m8, c02 = m1 * m5 - m4 * m2;
                    const double det = m0 * c00 + m1 * c01 + m2 * c02;
                    const double id = 1. / det;
                    const double d00 = c00 * id, d01 = (m2 * m5 - m1 * m8) * id, d02 = (m1 * m5 - m2 * m4) * id;
                    const double d11 = (m0 * m8 - m2 * m2) * id, d12 = (m2 * m1 - m0 * m5) * id;
                    const double d22 = (m0 * m4 - m1 * m1) * id;
                    g[9] = d00, g[10] = d01, g[11] = d02, g[12] = d11, g[13] = d12, g[14] = d22;
                    g[15] = d00 * g[6] + d01 * g[7] + d02 * g[8];
                    g[16] = d01 * g[6] + d11 * g[7] + d12 * g[8];
                    g[17] = d02 * g[6] + d12 * g[7] + d22 * g[8];
                }
                #pragma unroll 1
                for (int i = tid; i < w.nk; i += LBA_THREADS) {
                    if (kf_slot[i] < 0 || !s_kact[kf_slot[i]]) continue;
#pragma unroll
                    for (int k = 0; k < 7; ++k) kfTb[(size_t)i * 7 + k] = kfT[(size_t)i * 7 + k];
                }
                __syncthreads();
                // Hschur = Hpp + lambda I - sum_p (B_i1 Dinv) B_i2' and bschur = b_p - sum_p B_i1 (Dinv b_l): a wave
                // per block of the upper block triangle sums over the points that both keyframes see, in point
                // order; lanes 0-35 own the block's entries, lanes 36-41 of a diagonal block its part of bschur.
                // An inactive keyframe's rows are the identity's.
                const int nblk = L * (L + 1) / 2;
                for (int b = wave; b < nblk; b += LBA_WAVES) {
                    int i1 = 0, rem = b;
                    for (int k = 0; k < LBA_MAX_FREE_KF; ++k) {
                        if (rem < L - i1) break;
                        rem -= L - i1, ++i1;
                    }
                    const int i2 = i1 + rem;
                    const int er = lane / 6, ec = lane % 6, cr = lane - 36;
                    const bool diag = i1 == i2;
                    const bool ent = lane < 36 && (!diag || er <= ec);
                    const bool cf = diag && lane >= 36 && lane < 42;
                    double acc = 0., coef = 0.;
                    const bool live = s_kact[i1] && s_kact[i2];
                    if (!live) {
                        if (diag && lane < 36 && er == ec) acc = 1.;
                    } else {
                        if (diag && ent) acc = hpp[i1 * LBA_KF + er * 6 - er * (er - 1) / 2 + (ec - er)] + (er == ec ? lambda : 0.);
                        const unsigned long long both = (1ull << i1) | (1ull << i2);
                        for (int q0 = 0; q0 < w.np; q0 += 64) {
                            const int q = q0 + lane;
                            unsigned long long bal = __ballot(q < w.np && (pmask[q] & both) == both);
                            for (int k = 0; k < 64; ++k) {
                                if (!bal) break;
                                const int p = q0 + __ffsll(bal) - 1;
                                bal &= bal - 1;
                                int ea = -1, eb = -1;
                                for (int c0 = pe0[p]; c0 < pe1[p]; c0 += 64) {
                                    const int e = c0 + lane;
                                    const int sl = e < pe1[p] && e_state[e] == 0 ? e_slot[e] : -1;
                                    const unsigned long long ba = __ballot(sl == i1), bb = __ballot(sl == i2);
                                    if (ba) ea = c0 + __ffsll(ba) - 1;
                                    if (bb) eb = c0 + __ffsll(bb) - 1;
                                }
                                if (ea < 0 || eb < 0) continue;  // the mask names edges that exist
                                const double* g = pts + (size_t)p * LBA_PT;
                                if (ent) {
                                    const double* B1 = hpl + (size_t)ea * 18 + 3 * er;
                                    const double* B2 = hpl + (size_t)eb * 18 + 3 * ec;
                                    const double bd0 = B1[0] * g[9] + B1[1] * g[10] + B1[2] * g[11];
                                    const double bd1 = B1[0] * g[10] + B1[1] * g[12] + B1[2] * g[13];
                                    const double bd2 = B1[0] * g[11] + B1[1] * g[13] + B1[2] * g[14];
                                    acc -= bd0 * B2[0] + bd1 * B2[1] + bd2 * B2[2];
                                }
                                if (cf) {
                                    const double* B1 = hpl + (size_t)ea * 18 + 3 * cr;
                                    coef += B1[0] * g[15] + B1[1] * g[16] + B1[2] * g[17];
                                }
                            }
                        }
                    }
                    if (ent) A[(size_t)(6 * i2 + ec) * N + 6 * i1 + er] = acc;
                    if (cf) bs[6 * i1 + cr] = live ? hpp[i1 * LBA_KF + 21 + cr] - coef : 0.;
                }
                __syncthreads();
                // the dense L L' of the lower triangle, right-looking in panels of LBA_PANEL columns staged
                // through LDS; every entry's subtractions run in column order
                bool ok2 = true;
                for (int c0 = 0; c0 < N; c0 += LBA_PANEL) {
                    const int pw = min(LBA_PANEL, N - c0), ph = N - c0;
                    for (int idx = tid; idx < ph * pw; idx += LBA_THREADS) {
                        const int pr = idx / pw, pc = idx % pw;
                        s_panel[pr * LBA_PANEL + pc] = A[(size_t)(c0 + pr) * N + c0 + pc];
                    }
                    __syncthreads();
                    for (int c = 0; c < pw; ++c) {
                        const double d = s_panel[c * LBA_PANEL + c];
                        if (!(d > 0) || !isfinite(d)) {
                            ok2 = false;
                            break;
                        }
                        const double sq = sqrt(d);
                        __syncthreads();  // every thread has read the pivot
                        for (int pr = c + tid; pr < ph; pr += LBA_THREADS)
                            s_panel[pr * LBA_PANEL + c] = pr == c ? sq : s_panel[pr * LBA_PANEL + c] / sq;
                        __syncthreads();
                        const int rw = pw - c - 1, rh = ph - c - 1;
                        for (int idx = tid; idx < rw * rh; idx += LBA_THREADS) {
                            const int pr = c + 1 + idx / rw, pc = c + 1 + idx % rw;
                            if (pr >= pc) s_panel[pr * LBA_PANEL + pc] -= s_panel[pr * LBA_PANEL + c] * s_panel[pc * LBA_PANEL + c];
                        }
                        __syncthreads();
                    }
                    if (!ok2) break;
                    for (int idx = tid; idx < ph * pw; idx += LBA_THREADS) {
                        const int pr = idx / pw, pc = idx % pw;
                        if (pr >= pc) A[(size_t)(c0 + pr) * N + c0 + pc] = s_panel[pr * LBA_PANEL + pc];
                    }
                    const int th = ph - pw;
                    for (int idx = tid; idx < th * th; idx += LBA_THREADS) {
                        const int ti = idx / th, tj = idx % th;
                        if (tj > ti) continue;
                        double v = A[(size_t)(c0 + pw + ti) * N + c0 + pw + tj];
                        for (int c = 0; c < pw; ++c) v -= s_panel[(pw + ti) * LBA_PANEL + c] * s_panel[(pw + tj) * LBA_PANEL + c];
                        A[(size_t)(c0 + pw + ti) * N + c0 + pw + tj] = v;
                    }
                    __syncthreads();
                }
                if (!ok2) ++Ir.refused;
                __syncthreads();
                if (ok2) {
                    // L y = bschur by columns, then L' x = y by rows of L: one barrier per column
                    for (int k = tid; k < N; k += LBA_THREADS) s_b[k] = bs[k];
                    for (int k = 0; k < N; ++k) {
                        __syncthreads();
                        const double yk = s_b[k] / A[(size_t)k * N + k];
                        if (tid == 0) s_y[k] = yk;
                        for (int i = k + 1 + tid; i < N; i += LBA_THREADS) s_b[i] -= A[(size_t)i * N + k] * yk;
                    }
                    for (int k = N - 1; k >= 0; --k) {
                        __syncthreads();
                        const double xk = s_y[k] / A[(size_t)k * N + k];
                        if (tid == 0) s_x[k] = xk;
                        for (int i = tid; i < k; i += LBA_THREADS) s_y[i] -= A[(size_t)k * N + i] * xk;
                    }
                    __syncthreads();
                    // x_l = Dinv (b_l - B' x_p)
                    #pragma unroll 1
                    for (int p = tid; p < w.np; p += LBA_THREADS) {
                        if (!pact[p]) continue;
                        double* g = pts + (size_t)p * LBA_PT;
                        double cl[3] = {g[6], g[7], g[8]};
                        #pragma unroll 1
                        for (int e = pe0[p]; e < pe1[p]; ++e) {
                            const int sl = e_slot[e];
                            if (e_state[e] || sl < 0) continue;
                            const double* Be = hpl + (size_t)e * 18;
#pragma unroll
                            for (int k = 0; k < 3; ++k) {
                                double t = Be[k] * -s_x[6 * sl];
#pragma unroll
                                for (int j = 1; j < 6; ++j) t += Be[3 * j + k] * -s_x[6 * sl + j];
                                cl[k] += t;
                            }
                        }
                        g[18] = g[9] * cl[0] + g[10] * cl[1] + g[11] * cl[2];
                        g[19] = g[10] * cl[0] + g[12] * cl[1] + g[13] * cl[2];
                        g[20] = g[11] * cl[0] + g[13] * cl[1] + g[14] * cl[2];
                    }
                }
                // computeScale's terms and update(x): X += x_l, T = exp(x_p) * T (a refused solve leaves x as it was)
                red[0] = 0., red[1] = 0.;
                #pragma unroll 1
                for (int p = tid; p < w.np; p += LBA_THREADS) {
                    if (!pact[p]) continue;
                    const double* g = pts + (size_t)p * LBA_PT;
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        red[0] += g[18 + k] * (lambda * g[18 + k] + g[6 + k]);
                        ptX[3 * p + k] += g[18 + k];
                    }
                }
                for (int k = tid; k < N; k += LBA_THREADS)
                    if (s_kact[k / 6]) red[0] += s_x[k] * (lambda * s_x[k] + hpp[(k / 6) * LBA_KF + 21 + k % 6]);
                #pragma unroll 1
                for (int i = tid; i < w.nk; i += LBA_THREADS) {
                    const int sl = kf_slot[i];
                    if (sl < 0 || !s_kact[sl]) continue;
                    double x6[6];
#pragma unroll
                    for (int k = 0; k < 6; ++k) x6[k] = s_x[6 * sl + k];
                    store_pose(kfT + (size_t)i * 7, exp_update(x6, load_pose(kfT + (size_t)i * 7)));
                }
                __syncthreads();
                // computeActiveErrors + activeRobustChi2 at the trial state
                #pragma unroll 1
                for (int p = tid; p < w.np; p += LBA_THREADS) {
                    if (!pact[p]) continue;
                    const double X[3] = {ptX[3 * p], ptX[3 * p + 1], ptX[3 * p + 2]};
                    #pragma unroll 1
                    for (int e = pe0[p]; e < pe1[p]; ++e) {
                        if (e_state[e]) continue;
                        const int i = ekf[e];
                        double err[2], Xc[3], rho0, rho1;
                        const double c2 = edge_chi2(load_pose(kfT + (size_t)i * 7), load_cam(kfK + (size_t)i * 4), X, eo[e],
                                                    eo[w.ne + e], eo[2 * w.ne + e], err, Xc);
                        chi2_e[e] = c2;
                        huber(c2, delta, dsqr, &rho0, &rho1);
                        red[1] += rho0;
                    }
                }
                block_sum<2>(red, s_red);
                const double temp = ok2 ? red[1] : DBL_MAX;
                rho = (cur - temp) / (red[0] + 1e-3);
                if (lm_accept(rho, temp, lambda, ni)) {
                    cur = temp;
                } else {  // pop()
                    #pragma unroll 1
                    for (int p = tid; p < w.np; p += LBA_THREADS) {
                        if (!pact[p]) continue;
#pragma unroll
                        for (int k = 0; k < 3; ++k) ptX[3 * p + k] = ptXb[3 * p + k];
                    }
                    #pragma unroll 1
                    for (int i = tid; i < w.nk; i += LBA_THREADS) {
                        if (kf_slot[i] < 0 || !s_kact[kf_slot[i]]) continue;
#pragma unroll
                        for (int k = 0; k < 7; ++k) kfT[(size_t)i * 7 + k] = kfTb[(size_t)i * 7 + k];
                    }
                }
                __syncthreads();
                ++qmax;
                ++Ir.trials;
                again = rho < 0 && qmax < 10;  // a NaN rho leaves the loop
            }
            Ir.chi2_after = cur;
            stop = lm_stop(qmax, rho, ini, cur, bad_steps);
        }
        Ir.lambda = lambda;
        if (tid == 0 && a.info) a.info[s].round[r] = Ir;
        // the classification (Optimizer.cc:453-470, 497-515), sequential within a point: a thread per point
        __syncthreads();
        #pragma unroll 1
        for (int p = tid; p < w.np; p += LBA_THREADS) {
            if (pstate[p]) continue;  // pMP->isBad()
            const double X[3] = {ptX[3 * p], ptX[3 * p + 1], ptX[3 * p + 2]};
            int cnt = pcnt[p];
            bool bad = false;
            #pragma unroll 1
            for (int e = pe0[p]; e < pe1[p]; ++e) {
                if (bad || e_state[e]) continue;
                const int i = ekf[e];
                double rX[3];
                rotate(kfT + (size_t)i * 7, X, rX);
                const double z = rX[2] + kfT[(size_t)i * 7 + 6];
                if (chi2_e[e] > 5.991 || !(z > 0.0)) {
                    e_state[e] = (uint8_t)(r + 1);
                    if (--cnt <= 2) bad = true;  // MapPoint::EraseObservation -> SetBadFlag
                }
            }
            pcnt[p] = cnt;
            if (bad) pstate[p] = (uint8_t)(r + 1);
        }
    }
    __syncthreads();
    #pragma unroll 1
    for (int i = tid; i < w.nk; i += LBA_THREADS) {
        double M[12];
        matrix_from_quat(kfT + (size_t)i * 7, M);
#pragma unroll
        for (int k = 0; k < 3; ++k) M[9 + k] = kfT[(size_t)i * 7 + 4 + k];
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            if (a.kf_pose_out64) a.kf_pose_out64[(size_t)(w.k0 + i) * 12 + k] = M[k];
            if (a.kf_pose_out) a.kf_pose_out[(size_t)(w.k0 + i) * 12 + k] = (float)M[k];
        }
    }
    for (int k = tid; k < 3 * w.np; k += LBA_THREADS) {
        if (a.pt_pos_out64) a.pt_pos_out64[(size_t)w.p0 * 3 + k] = ptX[k];
        if (a.pt_pos_out) a.pt_pos_out[(size_t)w.p0 * 3 + k] = (float)ptX[k];
    }
    if (a.edge_erased)
        for (int e = tid; e < w.ne; e += LBA_THREADS) a.edge_erased[w.e0 + e] = e_state[e];
    if (a.pt_bad)
        for (int p = tid; p < w.np; p += LBA_THREADS) a.pt_bad[w.p0 + p] = pstate[p];
}

// The scratch regions of a call over S problems and the given totals.
void regions(LbaArgs& a, OrbLayout& Y) {
    const size_t S = (size_t)a.S, nk = (size_t)a.n_kf_total, np = (size_t)a.n_pt_total, ne = (size_t)a.n_edge_total;
    a.status = Y.take<int32_t>(S), a.n_free = Y.take<int32_t>(S);
    a.kf_T = Y.take<double>(nk * 7), a.kf_Tb = Y.take<double>(nk * 7);
    a.kf_slot = Y.take<int32_t>(nk);
    a.pt_X = Y.take<double>(np * 3), a.pt_Xb = Y.take<double>(np * 3);
    a.pt_sys = Y.take<double>(np * LBA_PT);
    a.pt_e0 = Y.take<int32_t>(np), a.pt_e1 = Y.take<int32_t>(np), a.pt_cnt = Y.take<int32_t>(np);
    a.pt_mask = Y.take<unsigned long long>(np);
    a.pt_act = Y.take<uint8_t>(np), a.pt_state = Y.take<uint8_t>(np);
    a.e_obs = Y.take<double>(ne * 3), a.e_chi2 = Y.take<double>(ne), a.e_hpl = Y.take<double>(ne * 18);
    a.e_slot = Y.take<int32_t>(ne), a.e_state = Y.take<uint8_t>(ne), a.csr = Y.take<int32_t>(ne);
    a.csr_off = Y.take<int32_t>(S * (LBA_MAX_FREE_KF + 1)), a.slot_kf = Y.take<int32_t>(S * LBA_MAX_FREE_KF);
    a.hpp = Y.take<double>(S * LBA_MAX_FREE_KF * LBA_KF);
    a.sys = Y.take<double>(S * LBA_MAX_N * LBA_MAX_N), a.bs = Y.take<double>(S * LBA_MAX_N);
}

int launch(LbaArgs a, hipStream_t st) {
    a.delta = (double)(float)std::sqrt(5.991);
    hipLaunchKernelGGL(k_lba_prepare, dim3(a.S), dim3(LBA_THREADS), 0, st, a);
    ORB_HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_lba_solve, dim3(a.S), dim3(LBA_THREADS), 0, st, a);
    ORB_HIPCHK(hipGetLastError());
    return ORB_OK;
}

}  // namespace

extern "C" {

int orb_local_bundle_adjustment(int n_kf, const float* kf_pose, const float* kf_K, const uint8_t* kf_fixed, int n_pt,
                                const float* pt_pos, const int32_t* pt_nobs, int n_edge, const int32_t* edge_pt,
                                const int32_t* edge_kf, const float* edge_obs, const float* edge_inv_sigma2,
                                float* kf_pose_out, double* kf_pose_out_f64, float* pt_pos_out, double* pt_pos_out_f64,
                                uint8_t* edge_erased, uint8_t* pt_bad, orb_local_ba_info_t* info, int device) {
    const std::string who = "local_bundle_adjustment";
    if (n_kf < 0 || n_pt < 0 || n_edge < 0 || (n_kf && (!kf_pose || !kf_K || !kf_fixed)) || (n_pt && (!pt_pos || !pt_nobs)) ||
        (n_edge && (!edge_pt || !edge_kf || !edge_obs || !edge_inv_sigma2)))
        return fail(ORB_EINVAL, who + ": bad arguments");
    int n_free = 0;
    for (int i = 0; i < n_kf; ++i) n_free += kf_fixed[i] ? 0 : 1;
    if (n_free == 0) return fail(ORB_ENOTSUP, who + ": no free keyframe");
    if (n_free > LBA_MAX_FREE_KF)
        return fail(ORB_ENOTSUP, who + ": more than " + std::to_string(LBA_MAX_FREE_KF) + " free keyframes");
    for (int i = 0; i < n_kf; ++i) {
        if (int r = orb_check_camera(who.c_str(), ("keyframe " + std::to_string(i)).c_str(), kf_K + 4 * i)) return r;
        for (int k = 0; k < 12; ++k)
            if (!std::isfinite(kf_pose[12 * i + k]))
                return fail(ORB_EINVAL, who + ": kf_pose[" + std::to_string(12 * i + k) + "] is not finite");
    }
    const size_t NK = (size_t)n_kf, NP = (size_t)n_pt, NE = (size_t)n_edge;
    OrbStagePlan P;
    const auto rOff = P.in<int32_t>(6);
    const auto rPose = P.in<float>(NK * 12), rK = P.in<float>(NK * 4);
    const auto rFix = P.in<uint8_t>(NK);
    const auto rPos = P.in<float>(NP * 3);
    const auto rNobs = P.in<int32_t>(NP), rEpt = P.in<int32_t>(NE), rEkf = P.in<int32_t>(NE);
    const auto rObs = P.in<float>(NE * 2), rSig = P.in<float>(NE);
    const auto rInfo = P.out<orb_local_ba_info_t>(1);
    const auto rP64 = P.out<double>(NK * 12), rX64 = P.out<double>(NP * 3);
    const auto rP32 = P.out<float>(NK * 12), rX32 = P.out<float>(NP * 3);
    const auto rEr = P.out<uint8_t>(NE), rBad = P.out<uint8_t>(NP);
    LbaArgs a{};
    a.S = 1, a.n_kf_total = n_kf, a.n_pt_total = n_pt, a.n_edge_total = n_edge;
    const size_t scratch = orb_layout_size([&](OrbLayout& Y) { regions(a, Y); });
    const auto rScr = P.scratch<uint8_t>(scratch);
    OrbHostCall call(P, device);
    if (call.err) return call.err;
    const int32_t off[6] = {0, n_kf, 0, n_pt, 0, n_edge};
    const int32_t* d_off = call.send(rOff, off);
    a.kf_off = d_off, a.pt_off = d_off + 2, a.edge_off = d_off + 4;
    a.kf_pose = call.send(rPose, kf_pose), a.kf_K = call.send(rK, kf_K), a.kf_fixed = call.send(rFix, kf_fixed);
    a.pt_pos = call.send(rPos, pt_pos), a.pt_nobs = call.send(rNobs, pt_nobs);
    a.edge_pt = call.send(rEpt, edge_pt), a.edge_kf = call.send(rEkf, edge_kf);
    a.edge_obs = call.send(rObs, edge_obs), a.edge_s = call.send(rSig, edge_inv_sigma2);
    a.info = call.dev(rInfo);
    a.kf_pose_out64 = call.dev(rP64), a.pt_pos_out64 = call.dev(rX64);
    a.kf_pose_out = call.dev(rP32), a.pt_pos_out = call.dev(rX32);
    a.edge_erased = call.dev(rEr), a.pt_bad = call.dev(rBad);
    OrbLayout Y(call.dev(rScr));
    regions(a, Y);
    if (int r = call.upload()) return r;
    if (int r = call.finish(launch(a, call.stream()), hipSuccess, who + ": ")) return r;
    const orb_local_ba_info_t* I = call.host(rInfo);
    if (I->status == ORB_EINVAL)
        return fail(ORB_EINVAL, who + ": the edges must be grouped by ascending point, name each (point, keyframe) pair "
                                      "once with indices in range, and be no more than pt_nobs per point");
    if (I->status != ORB_OK) return fail(I->status, who + ": refused on the device");
    call.get(rInfo, info);
    call.get(rP64, kf_pose_out_f64), call.get(rX64, pt_pos_out_f64);
    call.get(rP32, kf_pose_out), call.get(rX32, pt_pos_out);
    call.get(rEr, edge_erased), call.get(rBad, pt_bad);
    return ORB_OK;
}

int orb_local_bundle_adjustment_batch_device(int S, const int32_t* d_kf_off, const int32_t* d_pt_off,
                                             const int32_t* d_edge_off, int n_kf_total, int n_pt_total, int n_edge_total,
                                             const float* d_kf_pose, const float* d_kf_K, const uint8_t* d_kf_fixed,
                                             const float* d_pt_pos, const int32_t* d_pt_nobs, const int32_t* d_edge_pt,
                                             const int32_t* d_edge_kf, const float* d_edge_obs,
                                             const float* d_edge_inv_sigma2, float* d_kf_pose_out,
                                             double* d_kf_pose_out_f64, float* d_pt_pos_out, double* d_pt_pos_out_f64,
                                             uint8_t* d_edge_erased, uint8_t* d_pt_bad, orb_local_ba_info_t* d_info,
                                             void* stream) {
    const std::string who = "local_bundle_adjustment_batch";
    if (S < 0 || n_kf_total < 0 || n_pt_total < 0 || n_edge_total < 0) return fail(ORB_EINVAL, who + ": bad arguments");
    if (S > 65535) return fail(ORB_ENOTSUP, who + ": more than 65535 problems per call");
    if (S == 0) return ORB_OK;
    if (!d_kf_off || !d_pt_off || !d_edge_off || (n_kf_total && (!d_kf_pose || !d_kf_K || !d_kf_fixed)) ||
        (n_pt_total && (!d_pt_pos || !d_pt_nobs)) ||
        (n_edge_total && (!d_edge_pt || !d_edge_kf || !d_edge_obs || !d_edge_inv_sigma2)))
        return fail(ORB_EINVAL, who + ": bad arguments");
    LbaArgs a{};
    a.S = S, a.n_kf_total = n_kf_total, a.n_pt_total = n_pt_total, a.n_edge_total = n_edge_total;
    a.kf_off = d_kf_off, a.pt_off = d_pt_off, a.edge_off = d_edge_off;
    a.kf_pose = d_kf_pose, a.kf_K = d_kf_K, a.kf_fixed = d_kf_fixed;
    a.pt_pos = d_pt_pos, a.pt_nobs = d_pt_nobs;
    a.edge_pt = d_edge_pt, a.edge_kf = d_edge_kf, a.edge_obs = d_edge_obs, a.edge_s = d_edge_inv_sigma2;
    a.kf_pose_out = d_kf_pose_out, a.kf_pose_out64 = d_kf_pose_out_f64;
    a.pt_pos_out = d_pt_pos_out, a.pt_pos_out64 = d_pt_pos_out_f64;
    a.edge_erased = d_edge_erased, a.pt_bad = d_pt_bad, a.info = d_info;
    hipStream_t st = (hipStream_t)stream;
    void* tmp = nullptr;
    if (int r = orb_scratch_alloc(&tmp, st, who + ": scratch: ", [&](OrbLayout& Y) { regions(a, Y); })) return r;
    const int r = launch(a, st);
    (void)hipFreeAsync(tmp, st);
    return r;
}

}  // extern "C"
