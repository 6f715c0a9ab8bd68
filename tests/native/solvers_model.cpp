// CPU model of orb_pnp_check_inliers / orb_sim3_check_inliers and their batch forms: the
// per-correspondence set-up of the PnPsolver and Sim3Solver constructors (reference
// src/PnPsolver.cc:40-82, 126-128; src/Sim3Solver.cc:37-112), PnPsolver::CheckInliers (280-311),
// Sim3Solver::CheckInliers with Project / FromCameraToImage (335-359, 377-418) and the two
// keep-the-best loops (PnPsolver.cc:181-196, Sim3Solver.cc:183-200), restated statement for
// statement.  Built -ffp-contract=off; the fused multiply-adds that g++ -O3 -march=native makes of
// the reference's own translation units (scripts/contraction_check_solvers.sh) are written as
// std::fma, the cv::Mat arithmetic follows OpenCV 2.4 as oracle/ocv_ops.h states it (a separate
// binary: uncontracted; parity unpinned against a real OpenCV 2.4 build).
// Single-threaded; scripts/solvers_timing.py also times it.
//
// `variant` (tests only): bit 0 = plain, no fused operation anywhere; bit 1 = the Sim3 bound kept
// as the double 9.210 * sigma2 instead of the truncated size_t; bit 2 = only the three PnP row
// sums without their fused operations.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace {

constexpr int V_PLAIN = 1, V_UNTRUNC = 2, V_ROW_PLAIN = 4;

inline double mad(bool plain, double a, double b, double c) { return plain ? a * b + c : std::fma(a, b, c); }
inline float madf(bool plain, float a, float b, float c) { return plain ? a * b + c : std::fmaf(a, b, c); }

// mRi[r][0]*X + mRi[r][1]*Y + mRi[r][2]*Z + mti[r] as the reference build evaluates it
inline double pnp_row(bool plain, const double* r, double t, float X, float Y, float Z) {
    return mad(plain, r[2], (double)Z, mad(plain, r[0], (double)X, r[1] * (double)Y)) + t;
}

// cv::Mat A(3x3) * x + t (ocv::gemm3_add): float row sums left to right, then the double add
inline void gemm3_add(const float* A, int stride, const float* x, const float* t, int tstride, float* out) {
    for (int i = 0; i < 3; ++i) {
        const float* a = A + i * stride;
        float s = a[0] * x[0];
        s = s + a[1] * x[1];
        s = s + a[2] * x[2];
        out[i] = (float)((double)s + (double)t[i * tstride]);
    }
}

// the two values Project / FromCameraToImage push for a camera-frame point P
inline void to_image(bool plain, const float* P, const float* K, float* out) {
    const float fx = K[0], fy = K[1], cx = K[2], cy = K[3];
    const float invz = 1 / (P[2]);
    const float x = P[0] * invz;
    const float y = P[1] * invz;
    out[0] = madf(plain, fx, x, cx);
    out[1] = madf(plain, fy, y, cy);
}

// (a - b).dot(a - b) of two 2x1 CV_32F
inline float diff_dot2(const float* a, const float* b) {
    const float d0 = a[0] - b[0], d1 = a[1] - b[1];
    double r = 0;
    r += (double)d0 * d0;
    r += (double)d1 * d1;
    return (float)r;
}

void set_bit(uint64_t* mask, int i, bool v) {
    if (mask && v) mask[i >> 6] |= 1ull << (i & 63);
}

}  // namespace

extern "C" {

// PnPsolver's constructor over one SearchByBoW(KF, F) row: frame keypoints j ascending whose match
// m = match[j] is a keyframe keypoint (0 <= m < n_kf) with a MapPoint that is not bad.
// Returns N; writes p3d (N x 3), p2d (N x 2), sigma2 (N), index (N).
int solvers_model_pnp_setup(const float* f_xy, const int32_t* f_octave, int n_f, int n_kf, const int32_t* match,
                            const float* mp_pos, const uint8_t* mp_bad, const float* level_sigma2, float* p3d,
                            float* p2d, float* sigma2, int32_t* index) {
    int idx = 0;
    for (int i = 0; i < n_f; i++) {
        const int m = match[i];
        if (m < 0 || m >= n_kf) continue;      // pMP == NULL
        if (mp_bad && mp_bad[m]) continue;     // pMP->isBad()
        p2d[2 * idx] = f_xy[2 * i];
        p2d[2 * idx + 1] = f_xy[2 * i + 1];
        sigma2[idx] = level_sigma2[f_octave[i]];
        for (int k = 0; k < 3; ++k) p3d[3 * idx + k] = mp_pos[3 * m + k];
        index[idx] = i;
        idx++;
    }
    return idx;
}

// Sim3Solver's constructor over one SearchByBoW(KF1, KF2) row (match12[i1] = idx2), the pair (i1,
// idx2) standing for GetIndexInKeyFrame.  pose: Rcw | tcw (12 floats) per keyframe.
int solvers_model_sim3_setup(const int32_t* oct1, int n1, const int32_t* oct2, int n2, const int32_t* match12,
                             const float* pos1, const uint8_t* bad1, const float* pos2, const uint8_t* bad2,
                             const float* pose1, const float* pose2, const float* level_sigma2, float* x3dc1,
                             float* x3dc2, float* sigma2_1, float* sigma2_2, int32_t* index) {
    int idx = 0;
    for (int i1 = 0; i1 < n1; i1++) {
        const int i2 = match12[i1];
        if (i2 < 0 || i2 >= n2) continue;
        if ((bad1 && bad1[i1]) || (bad2 && bad2[i2])) continue;
        sigma2_1[idx] = level_sigma2[oct1[i1]];
        sigma2_2[idx] = level_sigma2[oct2[i2]];
        gemm3_add(pose1, 3, pos1 + 3 * i1, pose1 + 9, 1, x3dc1 + 3 * idx);
        gemm3_add(pose2, 3, pos2 + 3 * i2, pose2 + 9, 1, x3dc2 + 3 * idx);
        index[idx] = i1;
        idx++;
    }
    return idx;
}

// n_hyp iterations of PnPsolver::iterate without the hypothesis: CheckInliers, then lines 181-196.
// R n_hyp x 9, t n_hyp x 3 (mRi, mti).  masks n_hyp x W, W = (n + 63) / 64 (zeroed here); err
// n_hyp x n (error2).  Any output may be NULL.
int solvers_model_pnp(int n, const float* p3d, const float* p2d, const float* sigma2, float th2, double fu, double fv,
                      double uc, double vc, int n_hyp, const double* R, const double* t, int min_inliers, int best_in,
                      int variant, int32_t* counts, uint64_t* masks, int32_t* best_at, int32_t* first_ok, float* err) {
    const bool plain = variant & V_PLAIN;
    const bool rplain = variant & (V_PLAIN | V_ROW_PLAIN);
    const int W = (n + 63) / 64;
    std::vector<float> mvMaxError(n);
    for (int i = 0; i < n; i++) mvMaxError[i] = sigma2[i] * th2;
    if (masks)
        for (size_t k = 0; k < (size_t)n_hyp * W; ++k) masks[k] = 0;
    int mnBestInliers = best_in;
    int holder = best_in > 0 ? -2 : -1;
    int first = -1;
    for (int h = 0; h < n_hyp; h++) {
        const double* mRi = R + 9 * h;
        const double* mti = t + 3 * h;
        int mnInliersi = 0;
        for (int i = 0; i < n; i++) {
            const float X = p3d[3 * i], Y = p3d[3 * i + 1], Z = p3d[3 * i + 2];
            const float Xc = pnp_row(rplain, mRi, mti[0], X, Y, Z);
            const float Yc = pnp_row(rplain, mRi + 3, mti[1], X, Y, Z);
            const float invZc = 1 / pnp_row(rplain, mRi + 6, mti[2], X, Y, Z);
            const double ue = mad(plain, fu * Xc, invZc, uc);
            const double ve = mad(plain, fv * Yc, invZc, vc);
            const float distX = p2d[2 * i] - ue;
            const float distY = p2d[2 * i + 1] - ve;
            const float error2 = madf(plain, distX, distX, distY * distY);
            if (err) err[(size_t)h * n + i] = error2;
            const bool in = error2 < mvMaxError[i];
            if (in) mnInliersi++;
            set_bit(masks ? masks + (size_t)h * W : nullptr, i, in);
        }
        if (counts) counts[h] = mnInliersi;
        if (mnInliersi >= min_inliers) {
            if (mnInliersi > mnBestInliers) {
                mnBestInliers = mnInliersi;
                holder = h;
            }
            if (first < 0) first = h;
        }
        if (best_at) best_at[h] = holder;
    }
    if (first_ok) *first_ok = first;
    return 0;
}

// n_hyp iterations of Sim3Solver::iterate without computeT: CheckInliers, then lines 183-200.
// K1 / K2: fx, fy, cx, cy.  T12 / T21: n_hyp x 12, rows 0-2 of mT12i / mT21i (row-major 3x4).
int solvers_model_sim3(int n, const float* x3dc1, const float* x3dc2, const float* sigma2_1, const float* sigma2_2,
                       const float* K1, const float* K2, int n_hyp, const float* T12, const float* T21,
                       int min_inliers, int best_in, int variant, int32_t* counts, uint64_t* masks, int32_t* best_at,
                       int32_t* first_accept, float* err1, float* err2) {
    const bool plain = variant & V_PLAIN;
    const int W = (n + 63) / 64;
    std::vector<float> b1(n), b2(n), P1im1(2 * (size_t)n), P2im2(2 * (size_t)n);
    for (int i = 0; i < n; i++) {
        if (variant & V_UNTRUNC) {  // err < (double): the float is widened, compared against 9.21 * sigma2
            b1[i] = b2[i] = 0;
        } else {
            const size_t m1 = 9.210 * sigma2_1[i];
            const size_t m2 = 9.210 * sigma2_2[i];
            b1[i] = (float)m1;  // err1 < mvnMaxError1[i] converts the integer to float
            b2[i] = (float)m2;
        }
        to_image(plain, x3dc1 + 3 * i, K1, &P1im1[2 * i]);
        to_image(plain, x3dc2 + 3 * i, K2, &P2im2[2 * i]);
    }
    if (masks)
        for (size_t k = 0; k < (size_t)n_hyp * W; ++k) masks[k] = 0;
    int mnBestInliers = best_in;
    int holder = best_in > 0 ? -2 : -1;
    int first = -1;
    for (int h = 0; h < n_hyp; h++) {
        const float* t12 = T12 + 12 * h;
        const float* t21 = T21 + 12 * h;
        int mnInliersi = 0;
        for (int i = 0; i < n; i++) {
            float P[3], P2im1[2], P1im2[2];
            gemm3_add(t12, 4, x3dc2 + 3 * i, t12 + 3, 4, P);
            to_image(plain, P, K1, P2im1);
            gemm3_add(t21, 4, x3dc1 + 3 * i, t21 + 3, 4, P);
            to_image(plain, P, K2, P1im2);
            const float e1 = diff_dot2(&P1im1[2 * i], P2im1);
            const float e2 = diff_dot2(P1im2, &P2im2[2 * i]);
            if (err1) err1[(size_t)h * n + i] = e1;
            if (err2) err2[(size_t)h * n + i] = e2;
            bool in;
            if (variant & V_UNTRUNC)
                in = (double)e1 < 9.210 * sigma2_1[i] && (double)e2 < 9.210 * sigma2_2[i];
            else
                in = e1 < b1[i] && e2 < b2[i];
            if (in) mnInliersi++;
            set_bit(masks ? masks + (size_t)h * W : nullptr, i, in);
        }
        if (counts) counts[h] = mnInliersi;
        if (mnInliersi >= mnBestInliers) {
            mnBestInliers = mnInliersi;
            holder = h;
            if (mnInliersi > min_inliers && first < 0) first = h;
        }
        if (best_at) best_at[h] = holder;
    }
    if (first_accept) *first_accept = first;
    return 0;
}

}  // extern "C"
