// orb_essgraph.hip — Optimizer::OptimizeEssentialGraph on the GPU (part of liborb_hip.so).
//
// The pose-graph optimisation that LoopClosing::CorrectLoop runs once a loop is verified (reference
// src/Optimizer.cc:1470-1719, called at LoopClosing.cc:560), with the parts of g2o it runs restated in
// double:
//   vertices        VertexSim3Expmap per keyframe (Optimizer.cc:1498-1531): CorrectedSim3 or Sim3(R, t, 1)
//   edges           EdgeSim3 (types_seven_dof_expmap.h:99-126): error (C * v1 * v2^-1).log(), information
//                   I, measurement Sjw * Swi (Optimizer.cc:1539-1659)
//   Jacobian        BaseBinaryEdge::linearizeOplus, numeric (base_binary_edge.hpp:131-205)
//   quadratic form  base_binary_edge.hpp:55-90, no robust kernel
//   block solver    BlockSolver_7_3 without marginalised vertices: Hpp solved directly, by an unpivoted
//                   L L' over the block profile in place of CHOLMOD
//   Levenberg       optimization_algorithm_levenberg.cpp:61-189 with setUserLambdaInit(1e-16)
//   results         the SE3 recovery and the point correction (Optimizer.cc:1666-1718)
// The Sim3 state, its product, inverse, exponential and logarithm and the Levenberg bookkeeping are
// those of csrc/orb_g2o_math.h.
//
// Arithmetic: all f64, the TU built -ffp-contract=off.  Every sum has one owner and one written order
// (a free vertex's thread over its edge list, a block's thread over the edges that name its pair, a
// factor entry's thread over the columns in ascending order, block_sum for the scalars), so a call
// gives the same bits on every run.  There is no floating-point atomic, no workgroup waits for
// another, and every loop is bounded by a size that is fixed before it starts.
//
// The integer structure of the system (which vertices are active and free, the free vertices'
// edge lists, the pairs that own an off-diagonal block, the block profile) is derived on the host from
// the edge rows alone: the profile has to be known before any scratch is sized.  Every floating-point
// value and every decision of the schedule is the kernels'; the host reads one small record per trial
// to know what to enqueue next.
//
//   k_eg_prepare     thread per keyframe / edge: widening, the estimates, the measurements
//   k_eg_linearize   thread per (edge, column): the error, or one column of one Jacobian
//   k_eg_begin       one workgroup: chi2 at the iteration's start, lambda and ni at iteration 0
//   k_eg_diag        thread per (free vertex, entry): the diagonal block and b over the edge list
//   k_eg_assemble    thread per (block, entry): H + lambda I into the profile storage
//   k_eg_factor_diag one workgroup per panel: the panel's diagonal block
//   k_eg_factor_rows many workgroups per panel: the rows below it that reach into the panel
//   k_eg_solve       one workgroup: both substitutions, by panels
//   k_eg_update      thread per free vertex: push and oplus
//   k_eg_trial       one workgroup: the trial's chi2, rho, the verdict, pop, what comes next
//   k_eg_poses       thread per keyframe: [R | t / s]
//   k_eg_points      thread per point: the two-Sim3 map (also orb_sim3_correct_points)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/orb_abi.h"
#include "orb_g2o_math.h"
#include "orb_internal.h"

namespace {

int fail(int code, const std::string& msg) { return orb_internal_set_error(code, msg); }

constexpr int EG_THREADS = 256;
static_assert(EG_THREADS / 64 == G2O_WAVES, "block_sum is written for this many waves");
constexpr int EG_PANEL_BLOCKS = 4;               // block columns of a factor panel
constexpr int EG_PW = 7 * EG_PANEL_BLOCKS;       // ... as scalar columns
constexpr int EG_SHARE_BLOCKS = 8;               // block rows of one workgroup in k_eg_factor_rows
constexpr int EG_RS = 7 * EG_SHARE_BLOCKS;       // ... as scalar rows
constexpr int EG_COLS = 15;                      // linearize: the error, 7 columns of Ji, 7 of Jj

enum { EG_NEXT_TRIAL = 0, EG_NEXT_ITERATION = 1, EG_DONE = 2 };

// The Levenberg state, in device memory; the host reads `next` after each trial.
struct EgState {
    double lambda, ni, cur, ini, rho;
    int32_t qmax, bad_steps, it, next;
    int32_t refused_now;  // this trial's factorisation met a pivot that is not positive and finite
    int32_t pad;
};

struct EgArgs {
    int n_kf, n_edge, n_free, N;
    const float* kf_pose;
    const double *kf_corr, *kf_nonc;
    const uint8_t *kf_has_corr, *kf_has_nonc;
    const int32_t *edge_i, *edge_j;
    const uint8_t* edge_kind;
    // structure
    const int32_t* kf_slot;    // n_kf: the free active vertex's block row, -1 otherwise
    const int32_t* slot_kf;    // n_free
    const int32_t* csr_off;    // n_free + 1
    const int32_t* csr;        // the edges of each free vertex, ascending
    const int32_t* pair_off;   // n_pair + 1
    const int32_t* pair_edge;  // the edges that name each (row, column) pair, ascending
    const int32_t *pair_row, *pair_col;
    const int32_t* blk_first;  // n_free: f(i), the first block column of block row i
    const int64_t* blk_off;    // n_free: where block row i starts in the profile storage, in doubles
    int n_pair;
    // state
    Sim3 *S0, *est, *bak, *meas;
    double* e_err;  // n_edge x 7
    double* e_J;    // n_edge x 2 x 49, row-major (error component, column)
    double* hdiag;  // n_free x 49
    double *b, *y, *x;  // N
    double* A;      // the profile storage: H + lambda I, then L
    EgState* st;
    orb_essential_graph_info_t* info;
};

__device__ __forceinline__ Sim3 load_sim3(const double* p) {
    Sim3 S;
#pragma unroll
    for (int k = 0; k < 4; ++k) S.q[k] = p[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) S.t[k] = p[4 + k];
    S.s = p[7];
    return S;
}

__device__ __forceinline__ Sim3 vertex_in(const EgArgs& a, int i) {  // Optimizer.cc:1508-1520
    if (a.kf_has_corr && a.kf_has_corr[i]) return load_sim3(a.kf_corr + (size_t)i * 8);
    return sim3_from_pose(a.kf_pose + (size_t)i * 12);
}

__device__ __forceinline__ Sim3 noncorrected_or(const EgArgs& a, int i) {
    if (a.kf_has_nonc && a.kf_has_nonc[i]) return load_sim3(a.kf_nonc + (size_t)i * 8);
    return vertex_in(a, i);
}

__global__ void __launch_bounds__(EG_THREADS) k_eg_prepare(EgArgs a) {
    const int g = blockIdx.x * EG_THREADS + threadIdx.x;
    if (g < a.n_kf) {
        const Sim3 S = vertex_in(a, g);
        a.S0[g] = S, a.est[g] = S;
    } else if (g < a.n_kf + a.n_edge) {
        const int e = g - a.n_kf, i = a.edge_i[e], j = a.edge_j[e];
        const bool normal = a.edge_kind[e] != 0;
        const Sim3 Siw = normal ? noncorrected_or(a, i) : vertex_in(a, i);
        const Sim3 Sjw = normal ? noncorrected_or(a, j) : vertex_in(a, j);
        a.meas[e] = sim3_mul(Sjw, sim3_inverse(Siw));  // Sji = Sjw * Swi
    }
}

// EdgeSim3::computeError
__device__ __forceinline__ void edge_error(const Sim3& C, const Sim3& v1, const Sim3& v2, double* err) {
    sim3_log(sim3_mul(sim3_mul(C, v1), sim3_inverse(v2)), err);
}

__device__ __forceinline__ double dot7(const double* e) {
    double s = e[0] * e[0];
#pragma unroll
    for (int k = 1; k < 7; ++k) s += e[k] * e[k];
    return s;
}

__global__ void __launch_bounds__(EG_THREADS) k_eg_linearize(EgArgs a) {
    const int g = blockIdx.x * EG_THREADS + threadIdx.x;
    if (g >= a.n_edge * EG_COLS) return;
    const int e = g / EG_COLS, col = g % EG_COLS;
    const int i = a.edge_i[e], j = a.edge_j[e];
    const Sim3 C = a.meas[e], vi = a.est[i], vj = a.est[j];
    if (col == 0) {
        double err[7];
        edge_error(C, vi, vj, err);
#pragma unroll
        for (int k = 0; k < 7; ++k) a.e_err[(size_t)e * 7 + k] = err[k];
        return;
    }
    const int side = col > 7 ? 1 : 0, d = (col - 1) % 7;
    double* J = a.e_J + ((size_t)e * 2 + side) * 49;
    if (a.kf_slot[side ? j : i] < 0) {  // a fixed vertex gets no Jacobian
#pragma unroll
        for (int k = 0; k < 7; ++k) J[7 * k + d] = 0.;
        return;
    }
    const double delta = 1e-9, scalar = 1.0 / (2 * delta);
    double up[7], um[7], ep[7], em[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) up[k] = k == d ? delta : 0.0, um[k] = k == d ? -delta : 0.0;
    if (side == 0) {
        edge_error(C, sim3_oplus(up, vi), vj, ep);
        edge_error(C, sim3_oplus(um, vi), vj, em);
    } else {
        edge_error(C, vi, sim3_oplus(up, vj), ep);
        edge_error(C, vi, sim3_oplus(um, vj), em);
    }
#pragma unroll
    for (int k = 0; k < 7; ++k) J[7 * k + d] = scalar * (ep[k] - em[k]);
}

// activeChi2 at the estimates: the edges thread-strided, then block_sum; every thread gets it
__device__ double active_chi2(const EgArgs& a, double (*s_red)[2], double extra, double* extra_out) {
    double v[2] = {0., extra};
    #pragma unroll 1
    for (int e = threadIdx.x; e < a.n_edge; e += EG_THREADS) {
        double err[7];
        edge_error(a.meas[e], a.est[a.edge_i[e]], a.est[a.edge_j[e]], err);
        v[0] += dot7(err);
    }
    block_sum<2>(v, s_red);
    if (extra_out) *extra_out = v[1];
    return v[0];
}

__global__ void __launch_bounds__(EG_THREADS) k_eg_begin(EgArgs a) {
    __shared__ double s_red[G2O_WAVES][2];
    const double chi = active_chi2(a, s_red, 0., nullptr);
    if (threadIdx.x == 0) {
        EgState& s = *a.st;
        s.cur = chi, s.ini = chi;
        if (s.it == 0) {
            s.lambda = 1e-16;  // setUserLambdaInit
            s.ni = 2.;
            s.bad_steps = 0;
            a.info->chi2_before = chi;
        }
        s.rho = 0., s.qmax = 0;
        ++a.info->iterations;
    }
}

__global__ void __launch_bounds__(EG_THREADS) k_eg_diag(EgArgs a) {
    const int g = blockIdx.x * EG_THREADS + threadIdx.x;
    if (g >= a.n_free * 56) return;
    const int sl = g / 56, ent = g % 56, kf = a.slot_kf[sl];
    const int r = ent < 49 ? ent / 7 : ent - 49, c = ent < 49 ? ent % 7 : 0;
    double acc = 0.;
    #pragma unroll 1
    for (int q = a.csr_off[sl]; q < a.csr_off[sl + 1]; ++q) {
        const int e = a.csr[q];
        const double* J = a.e_J + ((size_t)e * 2 + (a.edge_i[e] == kf ? 0 : 1)) * 49;
        double s;
        if (ent < 49) {  // A' A
            s = J[r] * J[c];
#pragma unroll
            for (int k = 1; k < 7; ++k) s += J[7 * k + r] * J[7 * k + c];
        } else {  // A' (-(I e))
            const double* err = a.e_err + (size_t)e * 7;
            s = J[r] * -err[0];
#pragma unroll
            for (int k = 1; k < 7; ++k) s += J[7 * k + r] * -err[k];
        }
        acc += s;
    }
    if (ent < 49) a.hdiag[(size_t)sl * 49 + ent] = acc;
    else a.b[sl * 7 + r] = acc;
}

// where (R, k) of the profile storage is: first(R) <= k <= 7 (R / 7) + 6
__device__ __forceinline__ int eg_first(const EgArgs& a, int R) { return 7 * a.blk_first[R / 7]; }
__device__ __forceinline__ double* eg_row(const EgArgs& a, int R) {
    const int I = R / 7, w = 7 * (I - a.blk_first[I] + 1);
    return a.A + a.blk_off[I] + (size_t)(R % 7) * w - 7 * a.blk_first[I];
}

__global__ void __launch_bounds__(EG_THREADS) k_eg_assemble(EgArgs a) {
    const int g = blockIdx.x * EG_THREADS + threadIdx.x;
    const int blk = g / 49, ent = g % 49, r = ent / 7, c = ent % 7;
    if (blk < a.n_free) {
        const double v = a.hdiag[(size_t)blk * 49 + ent] + (r == c ? a.st->lambda : 0.);
        eg_row(a, 7 * blk + r)[7 * blk + c] = v;
    } else if (blk < a.n_free + a.n_pair) {
        const int p = blk - a.n_free, row = a.pair_row[p], colb = a.pair_col[p];
        double acc = 0.;
        #pragma unroll 1
        for (int q = a.pair_off[p]; q < a.pair_off[p + 1]; ++q) {
            const int e = a.pair_edge[q];
            const bool i_is_row = a.kf_slot[a.edge_i[e]] == row;
            const double* Jr = a.e_J + ((size_t)e * 2 + (i_is_row ? 0 : 1)) * 49;
            const double* Jc = a.e_J + ((size_t)e * 2 + (i_is_row ? 1 : 0)) * 49;
            double s = Jr[r] * Jc[c];
#pragma unroll
            for (int k = 1; k < 7; ++k) s += Jr[7 * k + r] * Jc[7 * k + c];
            acc += s;
        }
        eg_row(a, 7 * row + r)[7 * colb + c] = acc;
    }
}

// The panel [c0, c0 + pw): its diagonal block, every entry subtracting its products in ascending
// column order (the columns before the panel from the factor, those inside it through LDS).
__global__ void __launch_bounds__(EG_THREADS) k_eg_factor_diag(EgArgs a, int c0) {
    __shared__ double sD[EG_PW][EG_PW + 1];
    __shared__ double s_piv;
    if (a.st->refused_now) return;
    const int tid = threadIdx.x, pw = min(EG_PW, a.N - c0);
    for (int idx = tid; idx < pw * pw; idx += EG_THREADS) {
        const int r = idx / pw, c = idx % pw;
        if (c > r) continue;
        const int R = c0 + r, C = c0 + c, fr = eg_first(a, R), fc = eg_first(a, C);
        double v = 0.;
        if (fr <= C) {
            const double *pr = eg_row(a, R), *pc = eg_row(a, C);
            v = pr[C];
            #pragma unroll 1
            for (int k = max(fr, fc); k < c0; ++k) v -= pr[k] * pc[k];
        }
        sD[r][c] = v;
    }
    __syncthreads();
    bool ok = true;
    #pragma unroll 1
    for (int c = 0; c < pw; ++c) {
        double v = 0.;
        if (tid >= c && tid < pw) {
            v = sD[tid][c];
            #pragma unroll 1
            for (int k = 0; k < c; ++k) v -= sD[tid][k] * sD[c][k];
            if (tid == c) s_piv = v;
        }
        __syncthreads();
        const double d = s_piv;
        if (!(d > 0) || !isfinite(d)) {
            ok = false;
            break;
        }
        const double sq = sqrt(d);
        if (tid >= c && tid < pw) sD[tid][c] = tid == c ? sq : v / sq;
        __syncthreads();
    }
    if (!ok) {
        if (tid == 0) a.st->refused_now = 1;
        return;
    }
    for (int idx = tid; idx < pw * pw; idx += EG_THREADS) {
        const int r = idx / pw, c = idx % pw;
        if (c > r) continue;
        const int R = c0 + r, C = c0 + c;
        if (eg_first(a, R) <= C) eg_row(a, R)[C] = sD[r][c];
    }
}

// The rows below the panel, EG_RS per workgroup: an entry per thread for the columns before the panel,
// then a thread per row through the panel's columns.  Only columns [c0, c0 + pw) of these rows are written;
// what is read of other rows was finished by earlier launches.
__global__ void __launch_bounds__(EG_THREADS) k_eg_factor_rows(EgArgs a, int c0) {
    __shared__ double sD[EG_PW][EG_PW + 1];
    __shared__ double sR[EG_RS][EG_PW + 1];
    if (a.st->refused_now) return;
    const int tid = threadIdx.x, pw = min(EG_PW, a.N - c0), r0 = c0 + pw + blockIdx.x * EG_RS;
    bool reach = false;
    if (tid < EG_RS && r0 + tid < a.N) reach = eg_first(a, r0 + tid) < c0 + pw;
    if (!__syncthreads_or(reach)) return;
    for (int idx = tid; idx < pw * pw; idx += EG_THREADS) {
        const int r = idx / pw, c = idx % pw;
        const int R = c0 + r, C = c0 + c;
        sD[r][c] = c <= r && eg_first(a, R) <= C ? eg_row(a, R)[C] : 0.;
    }
    for (int idx = tid; idx < EG_RS * pw; idx += EG_THREADS) {
        const int lr = idx / pw, c = idx % pw, R = r0 + lr, C = c0 + c;
        double v = 0.;
        if (R < a.N) {
            const int fr = eg_first(a, R);
            if (fr <= C) {
                const int fc = eg_first(a, C);
                const double *pr = eg_row(a, R), *pc = eg_row(a, C);
                v = pr[C];
                #pragma unroll 1
                for (int k = max(fr, fc); k < c0; ++k) v -= pr[k] * pc[k];
            }
        }
        sR[lr][c] = v;
    }
    __syncthreads();
    const int R = r0 + tid;
    if (tid < EG_RS && R < a.N) {
        const int fr = eg_first(a, R);
        double* pr = eg_row(a, R);
        #pragma unroll 1
        for (int c = 0; c < pw; ++c) {
            if (fr > c0 + c) continue;
            double v = sR[tid][c];
            #pragma unroll 1
            for (int k = 0; k < c; ++k) v -= sR[tid][k] * sD[c][k];
            v /= sD[c][c];
            sR[tid][c] = v;
            pr[c0 + c] = v;
        }
    }
}

// L y = b by panels of EG_THREADS rows (a thread per row for the columns before the panel, then the
// panel's columns one barrier each), then L' x = y by rows of L from the last: for every entry the
// subtractions run in ascending, then descending, column order.
__global__ void __launch_bounds__(EG_THREADS) k_eg_solve(EgArgs a) {
    __shared__ double s_b[EG_THREADS];
    if (a.st->refused_now) return;
    const int tid = threadIdx.x, N = a.N;
    #pragma unroll 1
    for (int p0 = 0; p0 < N; p0 += EG_THREADS) {
        const int R = p0 + tid;
        int fr = 0;
        const double* pr = nullptr;
        double v = 0.;
        if (R < N) {
            fr = eg_first(a, R), pr = eg_row(a, R);
            v = a.b[R];
            #pragma unroll 1
            for (int k = fr; k < p0; ++k) v -= pr[k] * a.y[k];
        }
        s_b[tid] = v;
        __syncthreads();
        const int pn = min(EG_THREADS, N - p0);
        #pragma unroll 1
        for (int c = 0; c < pn; ++c) {
            const double yk = s_b[c] / eg_row(a, p0 + c)[p0 + c];
            if (tid == c) a.y[p0 + c] = yk;
            __syncthreads();  // s_b[c] is read before thread c + 1 .. write theirs; y is visible
            if (tid > c && R < N && fr <= p0 + c) s_b[tid] -= pr[p0 + c] * yk;
            __syncthreads();
        }
    }
    #pragma unroll 1
    for (int k = N - 1; k >= 0; --k) {
        __syncthreads();
        const double* pk = eg_row(a, k);
        const double xk = a.y[k] / pk[k];
        __syncthreads();  // every thread has read y[k]
        if (tid == 0) a.x[k] = xk;
        for (int i = eg_first(a, k) + tid; i < k; i += EG_THREADS) a.y[i] -= pk[i] * xk;
    }
}

__global__ void __launch_bounds__(EG_THREADS) k_eg_update(EgArgs a) {  // push(); update(x)
    const int sl = blockIdx.x * EG_THREADS + threadIdx.x;
    if (sl >= a.n_free) return;
    const int i = a.slot_kf[sl];
    const Sim3 T = a.est[i];
    a.bak[i] = T;
    double u[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) u[k] = a.x[sl * 7 + k];
    a.est[i] = sim3_oplus(u, T);
}

__global__ void __launch_bounds__(EG_THREADS) k_eg_trial(EgArgs a, int n_iterations) {
    __shared__ double s_red[G2O_WAVES][2];
    const int tid = threadIdx.x;
    EgState s = *a.st;
    double part = 0.;  // computeScale's terms
    #pragma unroll 1
    for (int k = tid; k < a.N; k += EG_THREADS) part += a.x[k] * (s.lambda * a.x[k] + a.b[k]);
    double scale;
    const double chi = active_chi2(a, s_red, part, &scale);
    scale += 1e-3;
    const double temp = s.refused_now ? DBL_MAX : chi;
    const double rho = (s.cur - temp) / scale;
    double lambda = s.lambda, ni = s.ni;
    const bool acc = lm_accept(rho, temp, lambda, ni);
    if (!acc) {  // pop()
        #pragma unroll 1
        for (int sl = tid; sl < a.n_free; sl += EG_THREADS) a.est[a.slot_kf[sl]] = a.bak[a.slot_kf[sl]];
    }
    if (tid != 0) return;
    orb_essential_graph_info_t& I = *a.info;
    if (I.trials < ORB_EG_MAX_TRIALS) {
        I.trial_rho[I.trials] = rho, I.trial_chi2[I.trials] = temp, I.trial_accepted[I.trials] = acc ? 1 : 0;
    }
    ++I.trials;
    if (s.refused_now) ++I.refused;
    s.lambda = lambda, s.ni = ni, s.rho = rho;
    if (acc) s.cur = temp;
    ++s.qmax;
    s.refused_now = 0;
    if (rho < 0 && s.qmax < 10) {  // a NaN rho leaves the loop
        s.next = EG_NEXT_TRIAL;
    } else {
        int bad = s.bad_steps;
        const bool stop = lm_stop(s.qmax, rho, s.ini, s.cur, bad);
        s.bad_steps = bad;
        ++s.it;
        s.next = stop || s.it >= n_iterations ? EG_DONE : EG_NEXT_ITERATION;
    }
    I.lambda = s.lambda, I.chi2_after = s.cur;
    *a.st = s;
}

struct EgOut {
    int n_kf;
    const Sim3* est;
    double* sim3;
    float* pose;
    double* pose64;
};

__global__ void __launch_bounds__(EG_THREADS) k_eg_poses(EgOut o) {
    const int i = blockIdx.x * EG_THREADS + threadIdx.x;
    if (i >= o.n_kf) return;
    const Sim3 S = o.est[i];
    double M[12];
    sim3_to_pose(S, M);
#pragma unroll
    for (int k = 0; k < 4; ++k) o.sim3[(size_t)i * 8 + k] = S.q[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) o.sim3[(size_t)i * 8 + 4 + k] = S.t[k];
    o.sim3[(size_t)i * 8 + 7] = S.s;
#pragma unroll
    for (int k = 0; k < 12; ++k) o.pose64[(size_t)i * 12 + k] = M[k], o.pose[(size_t)i * 12 + k] = (float)M[k];
}

struct EgPts {
    int n_pt, n_pair;
    const float* pos;
    const int32_t* pair;
    const double *from, *to;  // n_pair x 8 doubles each
    float* out;
    double* out64;
};

// to[pair]^-1.map(from[pair].map(P)); pair == -1: two identity Sim3s, the point as it is
__global__ void __launch_bounds__(EG_THREADS) k_eg_points(EgPts p) {
    const int g = blockIdx.x * EG_THREADS + threadIdx.x;
    if (g >= p.n_pt) return;
    const double P[3] = {(double)p.pos[3 * (size_t)g], (double)p.pos[3 * (size_t)g + 1], (double)p.pos[3 * (size_t)g + 2]};
    double Q[3] = {P[0], P[1], P[2]};
    const int r = p.pair[g];
    if (r >= 0 && r < p.n_pair) {
        double M[3];
        sim3_map(load_sim3(p.from + (size_t)r * 8), P, M);
        sim3_map(sim3_inverse(load_sim3(p.to + (size_t)r * 8)), M, Q);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) p.out64[3 * (size_t)g + k] = Q[k], p.out[3 * (size_t)g + k] = (float)Q[k];
}

inline dim3 grid_for(size_t n) { return dim3((unsigned)std::max<size_t>(1, (n + EG_THREADS - 1) / EG_THREADS)); }

int check_sim3(const std::string& who, const char* name, const double* v, size_t row) {
    for (int k = 0; k < 8; ++k)
        if (!std::isfinite(v[k]))
            return fail(ORB_EINVAL, who + ": " + name + "[" + std::to_string(row * 8 + k) + "] is not finite");
    if (!(v[7] > 0)) return fail(ORB_EINVAL, who + ": " + name + "[" + std::to_string(row * 8 + 7) + "]: the scale must be positive");
    return ORB_OK;
}

// The integer structure of the system, from the edge rows alone.
struct EgStructure {
    std::vector<int32_t> kf_slot, slot_kf, csr_off, csr, pair_off, pair_edge, pair_row, pair_col, blk_first;
    std::vector<int64_t> blk_off;
    int n_active = 0, n_free = 0;
    int64_t profile_doubles = 0;
};

void build_structure(int n_kf, const uint8_t* kf_fixed, int n_edge, const int32_t* ei, const int32_t* ej, EgStructure& S) {
    std::vector<uint8_t> active(n_kf, 0);
    for (int e = 0; e < n_edge; ++e) active[ei[e]] = active[ej[e]] = 1;
    S.kf_slot.assign(n_kf, -1);
    for (int i = 0; i < n_kf; ++i) {
        if (!active[i]) continue;
        ++S.n_active;
        if (!kf_fixed[i]) S.kf_slot[i] = S.n_free++, S.slot_kf.push_back(i);
    }
    const int nf = S.n_free;
    S.csr_off.assign(nf + 1, 0);
    S.blk_first.resize(nf);
    for (int i = 0; i < nf; ++i) S.blk_first[i] = i;
    std::vector<std::pair<int64_t, int32_t>> keyed;  // (row * nf + column, edge): sorted, the edges of a pair ascending
    for (int e = 0; e < n_edge; ++e) {
        const int si = S.kf_slot[ei[e]], sj = S.kf_slot[ej[e]];
        if (si >= 0) ++S.csr_off[si + 1];
        if (sj >= 0) ++S.csr_off[sj + 1];
        if (si >= 0 && sj >= 0) {
            const int row = std::max(si, sj), col = std::min(si, sj);
            S.blk_first[row] = std::min(S.blk_first[row], col);
            keyed.emplace_back((int64_t)row * nf + col, e);
        }
    }
    for (int i = 0; i < nf; ++i) S.csr_off[i + 1] += S.csr_off[i];
    S.csr.resize(S.csr_off[nf]);
    std::vector<int32_t> fill(S.csr_off.begin(), S.csr_off.end() - 1);
    for (int e = 0; e < n_edge; ++e) {
        const int si = S.kf_slot[ei[e]], sj = S.kf_slot[ej[e]];
        if (si >= 0) S.csr[fill[si]++] = e;
        if (sj >= 0) S.csr[fill[sj]++] = e;
    }
    std::sort(keyed.begin(), keyed.end());
    S.pair_off.push_back(0);
    for (size_t k = 0; k < keyed.size(); ++k) {
        if (k == 0 || keyed[k].first != keyed[k - 1].first) {
            if (k) S.pair_off.push_back((int32_t)k);
            S.pair_row.push_back((int32_t)(keyed[k].first / nf)), S.pair_col.push_back((int32_t)(keyed[k].first % nf));
        }
        S.pair_edge.push_back(keyed[k].second);
    }
    if (!keyed.empty()) S.pair_off.push_back((int32_t)keyed.size());
    S.blk_off.resize(nf);
    for (int i = 0; i < nf; ++i) {
        S.blk_off[i] = S.profile_doubles;
        S.profile_doubles += (int64_t)49 * (i - S.blk_first[i] + 1);
    }
}

int launch_points(const EgPts& p, hipStream_t st) {
    if (p.n_pt <= 0) return ORB_OK;
    hipLaunchKernelGGL(k_eg_points, grid_for(p.n_pt), dim3(EG_THREADS), 0, st, p);
    ORB_HIPCHK(hipGetLastError());
    return ORB_OK;
}

}  // namespace

extern "C" {

void orb_sim3_from_pose(const float* Tcw, double* sim3) {
    const Sim3 S = sim3_from_pose(Tcw);
    std::memcpy(sim3, &S, sizeof S);
}

void orb_sim3_to_pose(const double* sim3, float* pose, double* pose_f64) {
    Sim3 S;
    std::memcpy(&S, sim3, sizeof S);
    double M[12];
    sim3_to_pose(S, M);
    for (int k = 0; k < 12; ++k) {
        if (pose_f64) pose_f64[k] = M[k];
        if (pose) pose[k] = (float)M[k];
    }
}

int orb_sim3_correct_points(int n_pt, const float* pt_pos, const int32_t* pt_pair, int n_pair, const double* sim3_from,
                            const double* sim3_to, float* pt_pos_out, double* pt_pos_out_f64, int device) {
    const std::string who = "sim3_correct_points";
    if (n_pt < 0 || n_pair < 0 || (n_pt && (!pt_pos || !pt_pair)) || (n_pair && (!sim3_from || !sim3_to)))
        return fail(ORB_EINVAL, who + ": bad arguments");
    for (int p = 0; p < n_pt; ++p)
        if (pt_pair[p] < -1 || pt_pair[p] >= n_pair)
            return fail(ORB_EINVAL, who + ": pt_pair[" + std::to_string(p) + "] is out of range");
    for (int r = 0; r < n_pair; ++r) {
        if (int e = check_sim3(who, "sim3_from", sim3_from + (size_t)r * 8, r)) return e;
        if (int e = check_sim3(who, "sim3_to", sim3_to + (size_t)r * 8, r)) return e;
    }
    if (n_pt == 0) return ORB_OK;
    const size_t NP = (size_t)n_pt, NR = (size_t)n_pair;
    OrbStagePlan P;
    const auto rPos = P.in<float>(NP * 3);
    const auto rPair = P.in<int32_t>(NP);
    const auto rFrom = P.in<double>(NR * 8), rTo = P.in<double>(NR * 8);
    const auto rO64 = P.out<double>(NP * 3);
    const auto rO32 = P.out<float>(NP * 3);
    OrbHostCall call(P, device);
    if (call.err) return call.err;
    EgPts p{};
    p.n_pt = n_pt, p.n_pair = n_pair;
    p.pos = call.send(rPos, pt_pos), p.pair = call.send(rPair, pt_pair);
    p.from = call.send(rFrom, sim3_from), p.to = call.send(rTo, sim3_to);
    p.out64 = call.dev(rO64), p.out = call.dev(rO32);
    if (int r = call.upload()) return r;
    if (int r = call.finish(launch_points(p, call.stream()), hipSuccess, who + ": ")) return r;
    call.get(rO64, pt_pos_out_f64), call.get(rO32, pt_pos_out);
    return ORB_OK;
}

int orb_optimize_essential_graph(int n_kf, const float* kf_pose, const double* kf_corrected,
                                 const uint8_t* kf_has_corrected, const double* kf_noncorrected,
                                 const uint8_t* kf_has_noncorrected, const uint8_t* kf_fixed, int n_edge,
                                 const int32_t* edge_i, const int32_t* edge_j, const uint8_t* edge_kind, int n_pt,
                                 const float* pt_pos, const int32_t* pt_ref, const uint8_t* pt_skip, int n_iterations,
                                 double* kf_sim3_out, float* kf_pose_out, double* kf_pose_out_f64, float* pt_pos_out,
                                 double* pt_pos_out_f64, orb_essential_graph_info_t* info, int device) {
    const std::string who = "optimize_essential_graph";
    if (n_kf < 0 || n_edge < 0 || n_pt < 0 || n_iterations < 0 || (n_kf && (!kf_pose || !kf_fixed)) ||
        (n_edge && (!edge_i || !edge_j || !edge_kind)) || (n_pt && (!pt_pos || !pt_ref)) ||
        (kf_has_corrected && !kf_corrected) || (kf_has_noncorrected && !kf_noncorrected))
        return fail(ORB_EINVAL, who + ": bad arguments");
    if (n_kf > ORB_EG_MAX_KF) return fail(ORB_ENOTSUP, who + ": more than " + std::to_string(ORB_EG_MAX_KF) + " keyframes");
    for (int e = 0; e < n_edge; ++e) {
        if (edge_i[e] < 0 || edge_i[e] >= n_kf || edge_j[e] < 0 || edge_j[e] >= n_kf)
            return fail(ORB_EINVAL, who + ": edge " + std::to_string(e) + " names a keyframe out of range");
        if (edge_i[e] == edge_j[e]) return fail(ORB_EINVAL, who + ": edge " + std::to_string(e) + " is a self-edge");
        if (edge_kind[e] > 1) return fail(ORB_EINVAL, who + ": edge_kind[" + std::to_string(e) + "] must be 0 or 1");
    }
    for (int p = 0; p < n_pt; ++p)
        if (pt_ref[p] < -1 || pt_ref[p] >= n_kf)
            return fail(ORB_EINVAL, who + ": pt_ref[" + std::to_string(p) + "] is out of range");
    for (int i = 0; i < n_kf; ++i) {
        for (int k = 0; k < 12; ++k)
            if (!std::isfinite(kf_pose[12 * (size_t)i + k]))
                return fail(ORB_EINVAL, who + ": kf_pose[" + std::to_string(12 * (size_t)i + k) + "] is not finite");
        if (kf_has_corrected && kf_has_corrected[i])
            if (int r = check_sim3(who, "kf_corrected", kf_corrected + (size_t)i * 8, i)) return r;
        if (kf_has_noncorrected && kf_has_noncorrected[i])
            if (int r = check_sim3(who, "kf_noncorrected", kf_noncorrected + (size_t)i * 8, i)) return r;
    }
    EgStructure G;
    build_structure(n_kf, kf_fixed, n_edge, edge_i, edge_j, G);
    if (n_edge && G.n_active == G.n_free) return fail(ORB_EINVAL, who + ": no fixed keyframe among those the edges touch");
    const int64_t profile_bytes = G.profile_doubles * 8;
    if ((uint64_t)profile_bytes > ORB_EG_MAX_PROFILE_BYTES)
        return fail(ORB_ENOTSUP, who + ": the factor's profile of " + std::to_string(profile_bytes) +
                                     " bytes is above ORB_EG_MAX_PROFILE_BYTES");
    const size_t NK = (size_t)n_kf, NE = (size_t)n_edge, NP = (size_t)n_pt, NF = (size_t)G.n_free, NPAIR = G.pair_row.size();
    const size_t N = NF * 7;
    OrbStagePlan P;
    const auto rPose = P.in<float>(NK * 12);
    const auto rCorr = P.in<double>(kf_has_corrected ? NK * 8 : 0), rNonc = P.in<double>(kf_has_noncorrected ? NK * 8 : 0);
    const auto rHasC = P.in<uint8_t>(kf_has_corrected ? NK : 0), rHasN = P.in<uint8_t>(kf_has_noncorrected ? NK : 0);
    const auto rEi = P.in<int32_t>(NE), rEj = P.in<int32_t>(NE);
    const auto rEk = P.in<uint8_t>(NE);
    const auto rPos = P.in<float>(NP * 3);
    const auto rRef = P.in<int32_t>(NP);
    const auto rSlot = P.in<int32_t>(NK), rSlotKf = P.in<int32_t>(NF), rCsrOff = P.in<int32_t>(NF + 1),
               rCsr = P.in<int32_t>(G.csr.size()), rPairOff = P.in<int32_t>(NPAIR + 1),
               rPairEdge = P.in<int32_t>(G.pair_edge.size()), rPairRow = P.in<int32_t>(NPAIR),
               rPairCol = P.in<int32_t>(NPAIR), rBlkFirst = P.in<int32_t>(NF);
    const auto rBlkOff = P.in<int64_t>(NF);
    const auto rState = P.in<EgState>(1);
    const auto rInfoIn = P.in<orb_essential_graph_info_t>(1);
    const auto rNext = P.out<EgState>(1);  // where the state is copied for the host to read `next`
    const auto rInfo = P.out<orb_essential_graph_info_t>(1);
    const auto rSim3 = P.out<double>(NK * 8), rP64 = P.out<double>(NK * 12), rX64 = P.out<double>(NP * 3);
    const auto rP32 = P.out<float>(NK * 12), rX32 = P.out<float>(NP * 3);
    const auto rS0 = P.scratch<Sim3>(NK), rEst = P.scratch<Sim3>(NK), rBak = P.scratch<Sim3>(NK), rMeas = P.scratch<Sim3>(NE);
    const auto rErr = P.scratch<double>(NE * 7), rJ = P.scratch<double>(NE * 98), rHd = P.scratch<double>(NF * 49);
    const auto rB = P.scratch<double>(N), rY = P.scratch<double>(N), rXs = P.scratch<double>(N);
    const auto rA = P.scratch<double>((size_t)G.profile_doubles);
    OrbHostCall call(P, device);
    if (call.err) return call.err;
    EgArgs a{};
    a.n_kf = n_kf, a.n_edge = n_edge, a.n_free = G.n_free, a.N = (int)N, a.n_pair = (int)NPAIR;
    a.kf_pose = call.send(rPose, kf_pose);
    a.kf_corr = kf_has_corrected ? call.send(rCorr, kf_corrected) : nullptr;
    a.kf_nonc = kf_has_noncorrected ? call.send(rNonc, kf_noncorrected) : nullptr;
    a.kf_has_corr = kf_has_corrected ? call.send(rHasC, kf_has_corrected) : nullptr;
    a.kf_has_nonc = kf_has_noncorrected ? call.send(rHasN, kf_has_noncorrected) : nullptr;
    a.edge_i = call.send(rEi, edge_i), a.edge_j = call.send(rEj, edge_j), a.edge_kind = call.send(rEk, edge_kind);
    const float* d_pos = call.send(rPos, pt_pos);
    const int32_t* d_ref = call.send(rRef, pt_ref);
    a.kf_slot = call.send(rSlot, G.kf_slot.data()), a.slot_kf = call.send(rSlotKf, G.slot_kf.data());
    a.csr_off = call.send(rCsrOff, G.csr_off.data()), a.csr = call.send(rCsr, G.csr.data());
    if (G.pair_off.empty()) G.pair_off.push_back(0);
    a.pair_off = call.send(rPairOff, G.pair_off.data()), a.pair_edge = call.send(rPairEdge, G.pair_edge.data());
    a.pair_row = call.send(rPairRow, G.pair_row.data()), a.pair_col = call.send(rPairCol, G.pair_col.data());
    a.blk_first = call.send(rBlkFirst, G.blk_first.data()), a.blk_off = call.send(rBlkOff, G.blk_off.data());
    EgState st0{};
    st0.lambda = -1., st0.ni = 2., st0.next = EG_DONE;
    call.put(rState, &st0);
    orb_essential_graph_info_t I0{};
    I0.status = ORB_OK, I0.n_active = G.n_active, I0.n_free = G.n_free, I0.n_edges = n_edge;
    I0.profile_bytes = profile_bytes, I0.lambda = -1.;
    call.put(rInfoIn, &I0);
    a.st = call.dev(rState), a.info = call.dev(rInfoIn);
    a.S0 = call.dev(rS0), a.est = call.dev(rEst), a.bak = call.dev(rBak), a.meas = call.dev(rMeas);
    a.e_err = call.dev(rErr), a.e_J = call.dev(rJ), a.hdiag = call.dev(rHd);
    a.b = call.dev(rB), a.y = call.dev(rY), a.x = call.dev(rXs), a.A = call.dev(rA);
    if (int r = call.upload()) return r;
    hipStream_t s = call.stream();
    auto run = [&]() -> int {
        hipLaunchKernelGGL(k_eg_prepare, grid_for(NK + NE), dim3(EG_THREADS), 0, s, a);
        ORB_HIPCHK(hipGetLastError());
        if (N) ORB_HIPCHK(hipMemsetAsync(a.x, 0, N * 8, s));
        int next = N && n_edge && n_iterations > 0 ? EG_NEXT_ITERATION : EG_DONE;
        for (int it = 0; it < n_iterations && next == EG_NEXT_ITERATION; ++it) {
            hipLaunchKernelGGL(k_eg_linearize, grid_for(NE * EG_COLS), dim3(EG_THREADS), 0, s, a);
            hipLaunchKernelGGL(k_eg_begin, dim3(1), dim3(EG_THREADS), 0, s, a);
            hipLaunchKernelGGL(k_eg_diag, grid_for(NF * 56), dim3(EG_THREADS), 0, s, a);
            ORB_HIPCHK(hipGetLastError());
            next = EG_NEXT_TRIAL;
            for (int tr = 0; tr < 10 && next == EG_NEXT_TRIAL; ++tr) {
                ORB_HIPCHK(hipMemsetAsync(a.A, 0, (size_t)profile_bytes, s));
                hipLaunchKernelGGL(k_eg_assemble, grid_for((NF + NPAIR) * 49), dim3(EG_THREADS), 0, s, a);
                for (int c0 = 0; c0 < (int)N; c0 += EG_PW) {
                    hipLaunchKernelGGL(k_eg_factor_diag, dim3(1), dim3(EG_THREADS), 0, s, a, c0);
                    const int below = (int)N - c0 - EG_PW;
                    if (below > 0)
                        hipLaunchKernelGGL(k_eg_factor_rows, dim3((below + EG_RS - 1) / EG_RS), dim3(EG_THREADS), 0, s, a, c0);
                }
                hipLaunchKernelGGL(k_eg_solve, dim3(1), dim3(EG_THREADS), 0, s, a);
                hipLaunchKernelGGL(k_eg_update, grid_for(NF), dim3(EG_THREADS), 0, s, a);
                hipLaunchKernelGGL(k_eg_trial, dim3(1), dim3(EG_THREADS), 0, s, a, n_iterations);
                ORB_HIPCHK(hipGetLastError());
                ORB_HIPCHK(hipMemcpyAsync(call.host(rNext), a.st, sizeof(EgState), hipMemcpyDeviceToHost, s));
                ORB_HIPCHK(hipStreamSynchronize(s));
                next = call.host(rNext)->next;
            }
        }
        ORB_HIPCHK(hipMemcpyAsync(call.dev(rInfo), a.info, sizeof(orb_essential_graph_info_t), hipMemcpyDeviceToDevice, s));
        EgOut o{n_kf, a.est, call.dev(rSim3), call.dev(rP32), call.dev(rP64)};
        if (n_kf) hipLaunchKernelGGL(k_eg_poses, grid_for(NK), dim3(EG_THREADS), 0, s, o);
        ORB_HIPCHK(hipGetLastError());
        EgPts p{};
        p.n_pt = n_pt, p.n_pair = n_kf, p.pos = d_pos, p.pair = d_ref;
        p.from = (const double*)a.S0, p.to = (const double*)a.est;
        p.out64 = call.dev(rX64), p.out = call.dev(rX32);
        return launch_points(p, s);
    };
    if (int r = call.finish(run(), hipSuccess, who + ": ")) return r;
    call.get(rInfo, info);
    call.get(rSim3, kf_sim3_out), call.get(rP64, kf_pose_out_f64), call.get(rP32, kf_pose_out);
    if (!pt_skip) {
        call.get(rX64, pt_pos_out_f64), call.get(rX32, pt_pos_out);
    } else {
        const double* x64 = call.host(rX64);
        const float* x32 = call.host(rX32);
        for (size_t p = 0; p < NP; ++p) {
            if (pt_skip[p]) continue;
            if (pt_pos_out_f64) std::memcpy(pt_pos_out_f64 + 3 * p, x64 + 3 * p, 24);
            if (pt_pos_out) std::memcpy(pt_pos_out + 3 * p, x32 + 3 * p, 12);
        }
    }
    return ORB_OK;
}

}  // extern "C"
