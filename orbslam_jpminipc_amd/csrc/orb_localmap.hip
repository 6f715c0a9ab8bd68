// orb_localmap.hip — LocalMapping::CreateNewMapPoints on the GPU (part of liborb_hip.so).
//
// What the reference does between ORBmatcher::SearchForTriangulation and the new MapPoints
// (src/LocalMapping.cc:227-393, 474-491; KeyFrame::ComputeSceneMedianDepth, src/KeyFrame.cc:659-689),
// DESIGN.md §20; the CPU statement of the same reading is tests/native/local_mapping_model.cpp, which
// shares no text with this file.  IEEE f32 / f64 operations, the reference build's three fused
// multiply-adds per image written out, no libm call.  The cv::Mat arithmetic is csrc/orb_cv_math.h's,
// the triangulation's fill and SVD csrc/orb_jacobi_svd.h's.
//
//   lm_compute_f12   ComputeF12 as a __host__ __device__ function: orb_compute_f12 runs it on the host,
//                    k_lm_triangulate on thread 0 where the caller asks for F12.
//   k_lm_median      one workgroup per keyframe (or per pair, on the pair's second keyframe): the depths
//                    of the slots that hold a MapPoint gathered into LDS, sorted[(n - 1) / q] selected by
//                    rank counting (a NaN ranks after every number), and for a pair the baseline gate.
//   k_lm_triangulate one workgroup per pair: the matched slots compacted in ascending idx1 order, then
//                    one lane per match ordinal with the 4 x 4 work matrix, Vt and W on the lane's own
//                    LDS column (160 B per lane: 256 lanes hold 40 KiB), every gate of lines 299-374, and
//                    an ordered compaction of the accepted ordinals.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "../../include/orb_abi.h"
#include "orb_internal.h"
#include "orb_jacobi_svd.h"

namespace {

int fail(int code, const std::string& msg) { return orb_internal_set_error(code, msg); }

constexpr int LM_MAX_CAP = 8192;
constexpr int LM_MAX_PAIRS = 65535;
constexpr int LM_THREADS = 256;  // 160 B of LDS per lane

// cv::Mat arithmetic on 3-vectors and 3 x 3 matrices: csrc/orb_cv_math.h
using orb_cv::dot3;
using orb_cv::M3;
using orb_cv::norm3;

// LocalMapping::ComputeF12 (LocalMapping.cc:474-491).  R1w, R2w row-major 3 x 3, K1 / K2: fx fy cx cy.
__host__ __device__ inline void lm_compute_f12(const float* R1w, const float* t1w, const float* R2w, const float* t2w,
                                               const float* K1, const float* K2, float* F12) {
    // R12 = R1w*R2w.t(): gemm with GEMM_2_T, the general path (one double accumulator, k ascending);
    // -R1w*R2w.t() is the same gemm with alpha = -1, evaluated to a matrix before the next product
    const M3 R1 = orb_cv::load3x3(R1w), R2 = orb_cv::load3x3(R2w);
    const M3 R12 = orb_cv::gemm3<false, true>(R1, R2, 1.0), N12 = orb_cv::gemm3<false, true>(R1, R2, -1.0);
    // (..)*t2w+t1w: one gemm(N12, t2w, 1, t1w, 1), the short path
    float t12[3];
    orb_cv::gemm3_add(N12.m, t2w, t1w, t12);
    const M3 t12x = {{0.0f, -t12[2], t12[1], t12[2], 0.0f, -t12[0], -t12[1], t12[0], 0.0f}};
    const M3 K1t = {{K1[0], 0.0f, 0.0f, 0.0f, K1[1], 0.0f, K1[2], K1[3], 1.0f}};  // K1.t(), evaluated
    const M3 K2m = {{K2[0], 0.0f, K2[2], 0.0f, K2[1], K2[3], 0.0f, 0.0f, 1.0f}};
    const M3 F = orb_cv::mul3(orb_cv::mul3(orb_cv::mul3(orb_cv::inv3(K1t), t12x), R12), orb_cv::inv3(K2m));
    for (int k = 0; k < 9; ++k) F12[k] = F.m[k];
}

struct LmArgs {
    const orb_keypoint_t* kps;  // B x cap
    const int32_t* counts;      // B
    const int32_t* pair_a;      // P (NULL in k_lm_median: job j is keyframe j)
    const int32_t* pair_b;
    const int32_t* match;       // P x cap
    const float* pose;          // B x 12: Rcw row-major, tcw
    const float* ow;            // B x 3, or NULL: -Rcw.t()*tcw computed here
    const float* mp_pos;        // B x cap x 3, or NULL (no gate)
    const uint8_t* has_mp;      // B x cap
    float K1[4], K2[4];
    float sf1[ORB_MAX_VIEW_LEVELS], s21[ORB_MAX_VIEW_LEVELS], sf2[ORB_MAX_VIEW_LEVELS], s22[ORB_MAX_VIEW_LEVELS];
    int nl1, nl2;
    int cap, P, q;
    int32_t* gate;              // P: 0 go on, 1 short baseline, 2 no MapPoint; NULL = no gate
    float* median;              // jobs, may be NULL
    int32_t* n_depths;          // jobs, may be NULL
    float* x3d;                 // P x cap x 3; this and the following may be NULL
    uint8_t* status;            // P x cap
    float* cosr;                // P x cap
    int32_t* n_new;             // P
    int32_t* new1;              // P x cap
    int32_t* new2;
    float* F12;                 // P x 9
};

// GetCameraCenter of keyframe f: the caller's, or -Rcw.t()*tcw
__device__ __forceinline__ void lm_center(const LmArgs& a, int f, float* O) {
    if (a.ow) {
#pragma unroll
        for (int k = 0; k < 3; ++k) O[k] = a.ow[(size_t)f * 3 + k];
        return;
    }
    const float* T = a.pose + (size_t)f * 12;
    orb_cv::camera_centre(T, T + 9, O);
}

__global__ void __launch_bounds__(LM_THREADS) k_lm_median(LmArgs a) {
    __shared__ float s_z[LM_MAX_CAP];
    __shared__ int s_n;
    const int j = blockIdx.x, tid = threadIdx.x;
    const int f = a.pair_b ? a.pair_b[j] : j;
    const int n = min(max(a.counts[f], 0), a.cap);
    const float* T = a.pose + (size_t)f * 12;
    if (tid == 0) s_n = 0;
    __syncthreads();
    for (int i = tid; i < n; i += LM_THREADS)
        if (a.has_mp[(size_t)f * a.cap + i]) {
            // z = Rcw2.dot(x3Dw)+zcw: the dot and the sum in double, narrowed once
            const float* X = a.mp_pos + ((size_t)f * a.cap + i) * 3;
            s_z[atomicAdd(&s_n, 1)] = (float)(dot3(T + 6, X) + (double)T[11]);
        }
    __syncthreads();
    const int nz = s_n;
    if (nz == 0) {  // the reference indexes an empty vector here
        if (tid == 0) {
            if (a.median) a.median[j] = __builtin_nanf("");
            if (a.n_depths) a.n_depths[j] = 0;
            if (a.gate) a.gate[j] = 2;
        }
        return;
    }
    // sorted[(size - 1) / q]: the element with exactly that many before it, where "before" is a smaller
    // value, a number before a NaN, or an equal value in a lower slot
    const int idx = (nz - 1) / a.q;
    for (int e = tid; e < nz; e += LM_THREADS) {
        const float ce = s_z[e];
        const bool en = ce != ce;
        int rank = 0;
        for (int k = 0; k < nz; ++k) {
            const float ck = s_z[k];
            const bool kn = ck != ck;
            rank += ck < ce || (en && !kn) || ((ck == ce || (en && kn)) && k < e);
        }
        if (rank != idx) continue;
        if (a.median) a.median[j] = ce;
        if (a.n_depths) a.n_depths[j] = nz;
        if (a.gate) {  // LocalMapping.cc:258-265
            float O1[3], O2[3], vb[3];
            lm_center(a, a.pair_a[j], O1);
            lm_center(a, f, O2);
            orb_cv::sub3(O2, O1, vb);
            const float baseline = (float)norm3(vb);
            const float ratioBaselineDepth = baseline / ce;
            a.gate[j] = (double)ratioBaselineDepth < 0.01 ? 1 : 0;
        }
    }
}

// What the loop over the matches reads of one keyframe
struct LmCam {
    float R[9], t[3], O[3];
    float fx, fy, cx, cy, invfx, invfy;
};

__device__ __forceinline__ LmCam lm_cam(const LmArgs& a, int f, const float* K) {
    LmCam c;
    const float* T = a.pose + (size_t)f * 12;
#pragma unroll
    for (int k = 0; k < 9; ++k) c.R[k] = T[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) c.t[k] = T[9 + k];
    lm_center(a, f, c.O);
    c.fx = K[0], c.fy = K[1], c.cx = K[2], c.cy = K[3];
    c.invfx = 1.0f / c.fx;
    c.invfy = 1.0f / c.fy;
    return c;
}

// xn = ((x-cx)*invfx, (y-cy)*invfy, 1) and ray = Rwc*xn: Rwc = Rcw.t() is a matrix of its own, the product
// gemm's short path
__device__ __forceinline__ void lm_ray(const LmCam& c, float x, float y, float* xn, float* ray) {
    xn[0] = (x - c.cx) * c.invfx;
    xn[1] = (y - c.cy) * c.invfy;
    xn[2] = 1.0f;
#pragma unroll
    for (int i = 0; i < 3; ++i) ray[i] = c.R[i] * xn[0] + c.R[3 + i] * xn[1] + c.R[6 + i] * xn[2];
}

// The reprojection gate of one image (LocalMapping.cc:338-347 / 350-359): true = rejected.  z is the
// depth the caller has tested already.
__device__ __forceinline__ bool lm_reproj_fails(const LmCam& c, const float* p3, float z, float kx, float ky,
                                                float sigmaSquare) {
    const float x = (float)(dot3(c.R, p3) + (double)c.t[0]);
    const float y = (float)(dot3(c.R + 3, p3) + (double)c.t[1]);
    const float invz = (float)(1.0 / (double)z);
    const float u = __builtin_fmaf(c.fx * x, invz, c.cx);
    const float v = __builtin_fmaf(c.fy * y, invz, c.cy);
    const float errX = u - kx;
    const float errY = v - ky;
    // (the reference build squares errY, rounds, and fuses errX*errX into the sum, as in CheckRT)
    return (double)__builtin_fmaf(errX, errX, errY * errY) > 5.991 * (double)sigmaSquare;
}

// One match of LocalMapping.cc:291-391 on the lane's LDS column.  Returns the status code; *cosp is
// cosParallaxRays, pt the Euclidean point where the match got that far (zeros before).
__device__ int lm_triangulate_one(const LmArgs& a, const LmCam& c1, const LmCam& c2, const orb_keypoint_t& kp1,
                                  const orb_keypoint_t& kp2, float ratioFactor, const TriColumn& col, float* cosp,
                                  float* pt) {
    pt[0] = pt[1] = pt[2] = 0.0f;
    float xn1[3], xn2[3], ray1[3], ray2[3];
    lm_ray(c1, kp1.x, kp1.y, xn1, ray1);
    lm_ray(c2, kp2.x, kp2.y, xn2, ray2);
    const float cosParallaxRays = (float)(dot3(ray1, ray2) / (norm3(ray1) * norm3(ray2)));
    *cosp = cosParallaxRays;
    if (cosParallaxRays < 0.0f || (double)cosParallaxRays > 0.9998) return 2;
    // A.row(r) = xn*Tcw.row(2) - Tcw.row(r & 1) of the two [Rcw|tcw]
    const float xs[4] = {xn1[0], xn1[1], xn2[0], xn2[1]};
    float T1[12], T2[12], vr[4];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            T1[4 * i + j] = j < 3 ? c1.R[3 * i + j] : c1.t[i];
            T2[4 * i + j] = j < 3 ? c2.R[3 * i + j] : c2.t[i];
        }
    triangulate_vt3(T1, T2, xs, col, vr);
    if (vr[3] == 0.0f) return 3;
    float p3[3];
    orb_cv::scale3(vr, 1. / (double)vr[3], p3);  // rowRange(0,3)/x3D.at<float>(3): a MatExpr scale
    pt[0] = p3[0], pt[1] = p3[1], pt[2] = p3[2];
    const float z1 = (float)(dot3(c1.R + 6, p3) + (double)c1.t[2]);
    if (z1 <= 0.0f) return 4;
    const float z2 = (float)(dot3(c2.R + 6, p3) + (double)c2.t[2]);
    if (z2 <= 0.0f) return 5;
    if (lm_reproj_fails(c1, p3, z1, kp1.x, kp1.y, a.s21[min(max(kp1.octave, 0), a.nl1 - 1)])) return 6;
    if (lm_reproj_fails(c2, p3, z2, kp2.x, kp2.y, a.s22[min(max(kp2.octave, 0), a.nl2 - 1)])) return 7;
    float normal1[3], normal2[3];
    orb_cv::sub3(p3, c1.O, normal1);
    orb_cv::sub3(p3, c2.O, normal2);
    const float dist1 = (float)norm3(normal1);
    const float dist2 = (float)norm3(normal2);
    if (dist1 == 0.0f || dist2 == 0.0f) return 8;
    const float ratioDist = dist1 / dist2;
    const float ratioOctave = a.sf1[min(max(kp1.octave, 0), a.nl1 - 1)] / a.sf2[min(max(kp2.octave, 0), a.nl2 - 1)];
    if (ratioDist * ratioFactor < ratioOctave || ratioDist > ratioOctave * ratioFactor) return 9;
    return 1;
}

__global__ void __launch_bounds__(LM_THREADS) k_lm_triangulate(LmArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t smem[(LM_THREADS / 64) * TRI_WAVE_BYTES];
    __shared__ uint16_t s_ord[LM_MAX_CAP];  // idx1 of every match ordinal
    __shared__ int s_wtot[LM_THREADS / 64];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int f1 = a.pair_a[p], f2 = a.pair_b[p];
    const size_t row = (size_t)p * a.cap;
    // the rows as a pair without a match leaves them
    for (int i = tid; i < a.cap; i += LM_THREADS) {
        if (a.x3d) a.x3d[(row + i) * 3] = a.x3d[(row + i) * 3 + 1] = a.x3d[(row + i) * 3 + 2] = 0.0f;
        if (a.status) a.status[row + i] = 0;
        if (a.cosr) a.cosr[row + i] = __builtin_nanf("");
        if (a.new1) a.new1[row + i] = -1;
        if (a.new2) a.new2[row + i] = -1;
    }
    if (tid == 0 && a.F12) {
        const float* T1 = a.pose + (size_t)f1 * 12;
        const float* T2 = a.pose + (size_t)f2 * 12;
        lm_compute_f12(T1, T1 + 9, T2, T2 + 9, a.K1, a.K2, a.F12 + (size_t)p * 9);
    }
    if (a.gate && a.gate[p] != 0) {  // `continue` before the matcher runs: nothing is triangulated
        if (tid == 0 && a.n_new) a.n_new[p] = 0;
        return;
    }
    const orb_keypoint_t* k1 = a.kps + (size_t)f1 * a.cap;
    const orb_keypoint_t* k2 = a.kps + (size_t)f2 * a.cap;
    const int32_t* m12 = a.match + row;
    const int n1 = min(max(a.counts[f1], 0), a.cap), n2 = min(max(a.counts[f2], 0), a.cap);
    // vMatchedIndices: the matched slots in ascending idx1 (an entry is a match only inside [0, n2))
    int N = 0;
    for (int i0 = 0; i0 < n1; i0 += LM_THREADS) {
        const int i = i0 + tid;
        const int m = i < n1 ? m12[i] : -1;
        const bool ok = (unsigned)m < (unsigned)n2;
        const unsigned long long bal = __ballot(ok);
        if (lane == 0) s_wtot[wave] = __popcll(bal);
        __syncthreads();
        int off = N, tot = 0;
#pragma unroll
        for (int w = 0; w < LM_THREADS / 64; ++w) {
            const int t = s_wtot[w];
            if (w < wave) off += t;
            tot += t;
        }
        if (ok) s_ord[off + __popcll(bal & ((1ull << lane) - 1ull))] = (uint16_t)i;
        N += tot;
        __syncthreads();
    }
    const LmCam c1 = lm_cam(a, f1, a.K1), c2 = lm_cam(a, f2, a.K2);
    const float ratioFactor = 1.5f * a.sf1[1];  // 1.5f*GetScaleFactor(), the level-1 entry
    const TriColumn col(smem + wave * TRI_WAVE_BYTES, lane);
    int nnew = 0;
    for (int o0 = 0; o0 < N; o0 += LM_THREADS) {
        const int o = o0 + tid;
        int st = 0, i = 0, m = 0;
        if (o < N) {
            i = s_ord[o];
            m = m12[i];
            float cs, pt[3];
            st = lm_triangulate_one(a, c1, c2, k1[i], k2[m], ratioFactor, col, &cs, pt);
            if (a.status) a.status[row + i] = (uint8_t)st;
            if (a.cosr) a.cosr[row + i] = cs;
            if (a.x3d) a.x3d[(row + i) * 3] = pt[0], a.x3d[(row + i) * 3 + 1] = pt[1], a.x3d[(row + i) * 3 + 2] = pt[2];
        }
        // the accepted ordinals, in order
        const bool acc = st == 1;
        const unsigned long long bal = __ballot(acc);
        if (lane == 0) s_wtot[wave] = __popcll(bal);
        __syncthreads();
        int off = nnew, tot = 0;
#pragma unroll
        for (int w = 0; w < LM_THREADS / 64; ++w) {
            const int t = s_wtot[w];
            if (w < wave) off += t;
            tot += t;
        }
        if (acc) {
            const int d = off + __popcll(bal & ((1ull << lane) - 1ull));
            if (a.new1) a.new1[row + d] = i;
            if (a.new2) a.new2[row + d] = m;
        }
        nnew += tot;
        __syncthreads();
    }
    if (tid == 0 && a.n_new) a.n_new[p] = nnew;
}

int check_levels(const std::string& w, const char* which, int nlevels) {
    if (nlevels < 1 || nlevels > ORB_MAX_VIEW_LEVELS)
        return fail(ORB_EINVAL, w + which + "nlevels = " + std::to_string(nlevels) + " is not in 1..16");
    if (nlevels < 2)  // GetScaleFactor() is mvScaleFactors[1]
        return fail(ORB_ENOTSUP, w + which + "nlevels = 1: the reference reads the level-1 scale factor");
    return ORB_OK;
}

int check_finite(const std::string& w, const char* name, const float* v, int n) {
    for (int k = 0; k < n; ++k)
        if (!std::isfinite(v[k]))
            return fail(ORB_EINVAL, w + name + "[" + std::to_string(k) + "] = " + std::to_string(v[k]) + " must be finite");
    return ORB_OK;
}

void set_tables(LmArgs& a, const float* K1, const float* sf1, const float* s21, int nl1, const float* K2,
                const float* sf2, const float* s22, int nl2) {
    for (int k = 0; k < 4; ++k) a.K1[k] = K1[k], a.K2[k] = K2[k];
    for (int k = 0; k < ORB_MAX_VIEW_LEVELS; ++k) {
        a.sf1[k] = k < nl1 ? sf1[k] : 0.0f;
        a.s21[k] = k < nl1 ? s21[k] : 0.0f;
        a.sf2[k] = k < nl2 ? sf2[k] : 0.0f;
        a.s22[k] = k < nl2 ? s22[k] : 0.0f;
    }
    a.nl1 = nl1, a.nl2 = nl2;
}

// k_lm_median (when the gate's inputs are there) -> k_lm_triangulate on `st`.  a.gate: P ints where gated.
int run_create(LmArgs& a, hipStream_t st) {
    a.q = 2;
    if (a.gate) {
        hipLaunchKernelGGL(k_lm_median, dim3(a.P), dim3(LM_THREADS), 0, st, a);
        ORB_HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_lm_triangulate, dim3(a.P), dim3(LM_THREADS), 0, st, a);
    ORB_HIPCHK(hipGetLastError());
    return ORB_OK;
}

void view_pose(const orb_frame_view_t* V, float* T) {
    for (int k = 0; k < 9; ++k) T[k] = V->Rcw[k];
    for (int k = 0; k < 3; ++k) T[9 + k] = V->tcw[k];
}

int check_view(const std::string& w, const char* which, const orb_frame_view_t* V) {
    if (V->n < 0 || (V->n && !V->kps)) return fail(ORB_EINVAL, w + "bad arguments");
    if (V->n > LM_MAX_CAP) return fail(ORB_ENOTSUP, w + "more than 8192 keypoints per keyframe");
    const float K[4] = {V->fx, V->fy, V->cx, V->cy};
    if (int r = orb_check_camera(w.substr(0, w.size() - 2).c_str(), which, K)) return r;
    if (int r = check_finite(w, (std::string(which) + " Rcw").c_str(), V->Rcw, 9)) return r;
    if (int r = check_finite(w, (std::string(which) + " tcw").c_str(), V->tcw, 3)) return r;
    return check_finite(w, (std::string(which) + " Ow").c_str(), V->Ow, 3);
}

}  // namespace

extern "C" {

int orb_compute_f12(const orb_frame_view_t* KF1, const orb_frame_view_t* KF2, float* F12) {
    if (!KF1 || !KF2 || !F12) return fail(ORB_EINVAL, "compute F12: bad arguments");
    const float K1[4] = {KF1->fx, KF1->fy, KF1->cx, KF1->cy}, K2[4] = {KF2->fx, KF2->fy, KF2->cx, KF2->cy};
    lm_compute_f12(KF1->Rcw, KF1->tcw, KF2->Rcw, KF2->tcw, K1, K2, F12);
    return ORB_OK;
}

int orb_scene_median_depth_batch_device(const int32_t* d_counts, int cap, int B, const float* d_pose,
                                        const float* d_mp_pos, const uint8_t* d_has_mp, int q, float* d_depth,
                                        int32_t* d_n, void* stream) {
    const std::string w = "scene median depth: ";
    if (cap < 1 || B < 0) return fail(ORB_EINVAL, w + "bad arguments");
    if (cap > LM_MAX_CAP) return fail(ORB_ENOTSUP, w + "more than 8192 keypoints per keyframe");
    if (B > LM_MAX_PAIRS) return fail(ORB_ENOTSUP, w + "more than 65535 keyframes per batch");
    if (q < 1) return fail(ORB_EINVAL, w + "q = " + std::to_string(q) + " must be at least 1");
    if (B == 0) return ORB_OK;
    if (!d_counts || !d_pose || !d_mp_pos || !d_has_mp) return fail(ORB_EINVAL, w + "bad arguments");
    LmArgs a{};
    a.counts = d_counts, a.cap = cap, a.P = B, a.pose = d_pose, a.mp_pos = d_mp_pos, a.has_mp = d_has_mp, a.q = q;
    a.median = d_depth, a.n_depths = d_n;
    hipLaunchKernelGGL(k_lm_median, dim3(B), dim3(LM_THREADS), 0, (hipStream_t)stream, a);
    ORB_HIPCHK(hipGetLastError());
    return ORB_OK;
}

int orb_scene_median_depth(const orb_frame_view_t* KF, const float* mp_pos, const uint8_t* has_mp, int q, float* depth,
                           int device) {
    const std::string w = "scene median depth: ";
    if (!KF || KF->n < 0 || (KF->n && (!mp_pos || !has_mp))) return fail(ORB_EINVAL, w + "bad arguments");
    if (KF->n > LM_MAX_CAP) return fail(ORB_ENOTSUP, w + "more than 8192 keypoints per keyframe");
    if (q < 1) return fail(ORB_EINVAL, w + "q = " + std::to_string(q) + " must be at least 1");
    int n_mp = 0;
    for (int i = 0; i < KF->n; ++i) n_mp += has_mp[i] != 0;
    if (n_mp == 0) return fail(ORB_EINVAL, w + "the keyframe holds no MapPoint (the reference indexes an empty vector)");
    const int cap = KF->n;
    OrbStagePlan P;
    const auto rC = P.in<int32_t>(1);
    const auto rT = P.in<float>(12);
    const auto rX = P.in<float>((size_t)cap * 3);
    const auto rH = P.in<uint8_t>(cap);
    const auto rD = P.out<float>(1);
    OrbHostCall call(P, device);
    if (call.err) return call.err;
    float T[12];
    view_pose(KF, T);
    const int32_t n = KF->n;
    const int32_t* dc = call.send(rC, &n);
    const float* dT = call.send(rT, T);
    const float* dX = call.send(rX, mp_pos);
    const uint8_t* dH = call.send(rH, has_mp);
    if (int r = call.upload()) return r;
    const int r = orb_scene_median_depth_batch_device(dc, cap, 1, dT, dX, dH, q, call.dev(rD), nullptr, call.stream());
    if (int rf = call.finish(r, hipSuccess, w)) return rf;
    call.get(rD, depth);
    return ORB_OK;
}

int orb_create_new_map_points_batch_device(const orb_keypoint_t* d_kps, const int32_t* d_counts, int cap, int P,
                                           const int32_t* d_pair_a, const int32_t* d_pair_b, const int32_t* d_match,
                                           const float* d_pose, const float* d_mp_pos, const uint8_t* d_has_mp,
                                           const float* scale_factors, const float* level_sigma2, int nlevels,
                                           const float* K4, float* d_x3d, uint8_t* d_status, float* d_cos_rays,
                                           int32_t* d_n_new, int32_t* d_new_idx1, int32_t* d_new_idx2,
                                           int32_t* d_skipped, float* d_median_depth, float* d_F12, void* stream) {
    const std::string w = "create new map points: ";
    if (cap < 1 || P < 0) return fail(ORB_EINVAL, w + "bad arguments");
    if (cap > LM_MAX_CAP) return fail(ORB_ENOTSUP, w + "more than 8192 keypoints per keyframe");
    if (P > LM_MAX_PAIRS) return fail(ORB_ENOTSUP, w + "more than 65535 pairs per batch");
    if (!scale_factors || !level_sigma2 || !K4) return fail(ORB_EINVAL, w + "bad arguments");
    if (int r = check_levels(w, "", nlevels)) return r;
    if (int r = orb_check_camera("create new map points", "", K4)) return r;
    if ((d_mp_pos == nullptr) != (d_has_mp == nullptr))
        return fail(ORB_EINVAL, w + "d_mp_pos and d_has_mp go together (both NULL: no baseline gate)");
    if (P == 0) return ORB_OK;
    if (!d_kps || !d_counts || !d_pair_a || !d_pair_b || !d_match || !d_pose) return fail(ORB_EINVAL, w + "bad arguments");
    hipStream_t st = (hipStream_t)stream;
    LmArgs a{};
    a.kps = d_kps, a.counts = d_counts, a.pair_a = d_pair_a, a.pair_b = d_pair_b, a.match = d_match, a.pose = d_pose;
    a.mp_pos = d_mp_pos, a.has_mp = d_has_mp, a.cap = cap, a.P = P;
    set_tables(a, K4, scale_factors, level_sigma2, nlevels, K4, scale_factors, level_sigma2, nlevels);
    a.x3d = d_x3d, a.status = d_status, a.cosr = d_cos_rays, a.n_new = d_n_new, a.new1 = d_new_idx1, a.new2 = d_new_idx2;
    a.median = d_median_depth, a.F12 = d_F12;
    void* block = nullptr;
    if (d_mp_pos) {
        a.gate = d_skipped;
        if (!a.gate)
            if (int r = orb_scratch_alloc(&block, st, w, [&](OrbLayout& L) { a.gate = L.take<int32_t>(P); })) return r;
    } else if (d_skipped) {
        const hipError_t e = hipMemsetAsync(d_skipped, 0, (size_t)P * 4, st);
        if (e != hipSuccess) return fail(ORB_EDEVICE, w + hipGetErrorString(e));
    }
    const int r = run_create(a, st);
    if (block) (void)hipFreeAsync(block, st);
    return r;
}

int orb_create_new_map_points(const orb_frame_view_t* KF1, const orb_frame_view_t* KF2, const int32_t* match12,
                              const float* mp_pos2, const uint8_t* has_mp2, float* x3d, uint8_t* status,
                              float* cos_rays, int32_t* n_new, int32_t* new_idx1, int32_t* new_idx2, int32_t* skipped,
                              float* median_depth, int device) {
    const std::string w = "create new map points: ";
    if (!KF1 || !KF2) return fail(ORB_EINVAL, w + "bad arguments");
    if (int r = check_view(w, "KF1", KF1)) return r;
    if (int r = check_view(w, "KF2", KF2)) return r;
    if (int r = check_levels(w, "KF1 ", KF1->nlevels)) return r;
    if (int r = check_levels(w, "KF2 ", KF2->nlevels)) return r;
    const int n1 = KF1->n, n2 = KF2->n;
    if (n1 && !match12) return fail(ORB_EINVAL, w + "match12 is NULL");
    for (int i = 0; i < n1; ++i)
        if (match12[i] < -1 || match12[i] >= n2)
            return fail(ORB_EINVAL, w + "match12[" + std::to_string(i) + "] = " + std::to_string(match12[i]) +
                                        " is outside [-1, n2)");
    if ((mp_pos2 == nullptr) != (has_mp2 == nullptr))
        return fail(ORB_EINVAL, w + "mp_pos2 and has_mp2 go together (both NULL: no baseline gate)");
    const bool gated = mp_pos2 != nullptr;
    if (gated) {
        int n_mp = 0;
        for (int i = 0; i < n2; ++i) n_mp += has_mp2[i] != 0;
        if (n_mp == 0) return fail(ORB_EINVAL, w + "KF2 holds no MapPoint (the reference indexes an empty vector)");
    }
    const int cap = std::max(std::max(n1, n2), 1);
    OrbStagePlan P;
    const auto rK = P.in<orb_keypoint_t>((size_t)2 * cap);
    const auto rH = P.in<int32_t>(4);  // n1, n2, pair_a = 0, pair_b = 1
    const auto rM = P.in<int32_t>(cap);
    const auto rT = P.in<float>(24);
    const auto rO = P.in<float>(6);
    const auto rX = P.in<float>(gated ? (size_t)2 * cap * 3 : 0);
    const auto rHas = P.in<uint8_t>(gated ? (size_t)2 * cap : 0);
    const auto rS = P.out<int32_t>(2);  // n_new, skipped
    const auto rMed = P.out<float>(1);
    const auto rP = P.out<float>((size_t)cap * 3);
    const auto rC = P.out<float>(cap);
    const auto rN1 = P.out<int32_t>(cap), rN2 = P.out<int32_t>(cap);
    const auto rSt = P.out<uint8_t>(cap);
    OrbHostCall call(P, device);
    if (call.err) return call.err;
    call.zero_in();
    call.put(rK, KF1->kps, (size_t)n1);
    if (n2) memcpy(call.host(rK) + cap, KF2->kps, (size_t)n2 * sizeof(orb_keypoint_t));
    const int32_t hdr[4] = {n1, n2, 0, 1};
    call.put(rH, hdr);
    int32_t* hm = call.host(rM);
    for (int i = 0; i < cap; ++i) hm[i] = i < n1 ? match12[i] : -1;
    float T[24], O[6];
    view_pose(KF1, T);
    view_pose(KF2, T + 12);
    for (int k = 0; k < 3; ++k) O[k] = KF1->Ow[k], O[3 + k] = KF2->Ow[k];
    call.put(rT, T);
    call.put(rO, O);
    if (gated && n2) {
        memcpy(call.host(rX) + (size_t)cap * 3, mp_pos2, (size_t)n2 * 12);
        memcpy(call.host(rHas) + cap, has_mp2, (size_t)n2);
    }
    if (int r = call.upload()) return r;
    const int32_t* dh = call.dev(rH);
    LmArgs a{};
    a.kps = call.dev(rK), a.counts = dh, a.pair_a = dh + 2, a.pair_b = dh + 3, a.match = call.dev(rM);
    a.pose = call.dev(rT), a.ow = call.dev(rO), a.cap = cap, a.P = 1;
    if (gated) a.mp_pos = call.dev(rX), a.has_mp = call.dev(rHas), a.gate = call.dev(rS) + 1;
    const float K1[4] = {KF1->fx, KF1->fy, KF1->cx, KF1->cy}, K2[4] = {KF2->fx, KF2->fy, KF2->cx, KF2->cy};
    set_tables(a, K1, KF1->scale_factors, KF1->level_sigma2, KF1->nlevels, K2, KF2->scale_factors, KF2->level_sigma2,
               KF2->nlevels);
    a.x3d = call.dev(rP), a.status = call.dev(rSt), a.cosr = call.dev(rC), a.n_new = call.dev(rS);
    a.new1 = call.dev(rN1), a.new2 = call.dev(rN2), a.median = call.dev(rMed);
    hipError_t e = hipSuccess;
    if (!gated) e = hipMemsetAsync(call.dev(rS), 0, 8, call.stream());
    if (e == hipSuccess) e = hipMemsetAsync(call.dev(rMed), 0xFF, 4, call.stream());  // NaN where no median is taken
    const int r = e == hipSuccess ? run_create(a, call.stream()) : ORB_OK;
    if (int rf = call.finish(r, e, w)) return rf;
    call.get(rS, n_new, 1, 0);
    call.get(rS, skipped, 1, 1);
    call.get(rMed, median_depth);
    call.get(rP, x3d, (size_t)n1 * 3);
    call.get(rC, cos_rays, (size_t)n1);
    call.get(rN1, new_idx1, (size_t)n1);
    call.get(rN2, new_idx2, (size_t)n1);
    call.get(rSt, status, (size_t)n1);
    return ORB_OK;
}

}  // extern "C"
