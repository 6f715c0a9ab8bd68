// CPU model of orb_initializer_reconstruct: ReconstructF / ReconstructH, CheckRT, Triangulate and
// DecomposeE of the reference (src/Initializer.cc:468-745, 796-927), restated statement for
// statement, with the OpenCV 2.4 expressions they are written in restated as read (DESIGN.md §18
// lists every one: which steps are double, where the narrowing is).  No OpenCV 2.4 source or
// binary is at hand: parity with a real build is unpinned.  The SVD, inv() and the 3 x 3 short
// product are those of initializer_ransac_model.cpp, included below and not copied; norm, dot,
// subtract and A*x+t are oracle/ocv_ops.cpp's.  Built -ffp-contract=off; the three fused
// multiply-adds per image that g++ -O3 -march=native makes of CheckRT's reprojection lines and the
// two it makes of ReconstructH's d1*d1 - d2*d2 and d1*d1 - d3*d3 are written out as fmaf
// (scripts/contraction_check_initializer_reconstruct.sh).  Shares nothing with
// csrc/orb_initializer.hip.  -DINITIALIZER_RECONSTRUCT_MODEL_MAIN adds a main() for the sanitizer run.
#include "initializer_ransac_model.cpp"

#include <algorithm>

#include "../../oracle/ocv_ops.h"

namespace {

// cv::determinant of a 3x3 CV_32F: lapack.cpp's det3 macro, a double
double det3(const float* m) {
    return m[0] * ((double)m[4] * m[8] - (double)m[5] * m[7]) - m[1] * ((double)m[3] * m[8] - (double)m[5] * m[6]) +
           m[2] * ((double)m[3] * m[7] - (double)m[4] * m[6]);
}

// gemm with a transpose flag leaves the 2 <= len <= 4 path (it is taken with flags == 0 only) for
// GEMMSingleMul_<float, double>: one double accumulator per element, k ascending, times alpha, narrowed.
// d = alpha * op(a) * op(b); a is 3 x 3, b is 3 x bcols (b transposed only when 3 x 3).
void gemm_general(const float* a, bool ta, const float* b, bool tb, int bcols, double alpha, float* d) {
    float out[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < bcols; j++) {
            double s0 = 0;
            for (int k = 0; k < 3; k++)
                s0 += (double)(ta ? a[k * 3 + i] : a[i * 3 + k]) * (double)(tb ? b[j * 3 + k] : b[k * bcols + j]);
            out[i * bcols + j] = (float)(s0 * alpha);
        }
    std::memcpy(d, out, sizeof(float) * 3 * bcols);
}

// gemm's short path with alpha: (alpha*A)*B is one gemm(A, B, alpha): (float)((double)t * alpha)
void mul3_alpha(const float* a, const float* b, double alpha, float* d) {
    float out[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            float t = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
            out[3 * i + j] = (float)((double)t * alpha);
        }
    std::memcpy(d, out, sizeof(out));
}

// M / s and M *= s: MatOp_AddEx with alpha (= 1./s or s) -> convertTo(m, type, alpha, 0):
// cvtScale_<float, float, float>, x * (float)alpha + (float)0
void scale(const float* x, int n, double alpha, float* out) {
    const float a = (float)alpha, b = (float)0.0;
    for (int i = 0; i < n; i++) out[i] = x[i] * a + b;
}

// -M of a Mat: cv::subtract(Scalar(0), M)
void negate(const float* x, int n, float* out) {
    for (int i = 0; i < n; i++) out[i] = 0.0f - x[i];
}

void make_K(const float* K4, float* K) {
    const float k[9] = {K4[0], 0, K4[2], 0, K4[1], K4[3], 0, 0, 1};
    std::memcpy(K, k, sizeof(k));
}

void Triangulate(const float* kp1, const float* kp2, const float* P1, const float* P2, float* x3D) {
    float A[16];
    // A.row(i) = x*P.row(2) - P.row(r): MatOp_AddEx(a, b, alpha = x, beta = -1) -> addWeighted_<float, double>
    const float xs[4] = {kp1[0], kp1[1], kp2[0], kp2[1]};
    const float* Ps[4] = {P1, P1, P2, P2};
    for (int r = 0; r < 4; r++)
        for (int j = 0; j < 4; j++)
            A[r * 4 + j] = (float)((double)Ps[r][8 + j] * (double)xs[r] + (double)Ps[r][(r & 1) * 4 + j] * -1.0 + 0.0);
    float w[4], u[16], vt[16];
    SVDecomp(A, 4, 4, w, u, vt);
    // x3D = vt.row(3).t(); x3D = x3D.rowRange(0,3)/x3D.at<float>(3): a MatExpr scale by 1./w
    scale(vt + 12, 3, 1. / (double)vt[15], x3D);
}

struct CheckOut {
    int nGood;
    float parallax, cosSel;
};

// acos_variant: 0 = libm's acosf; +1 / -1 = its result moved one ulp up / down (the tolerance
// measurement of scripts/gen_initializer_reconstruct_golden.py); 2 = the reprojection lines without
// their fused multiply-adds (what a build without FMA computes; a test looks for a threshold that
// tells the two apart).  errs (2 per key of frame 1, may be NULL): squareError1 / squareError2 of
// every match that got as far as computing them, NaN elsewhere.
CheckOut CheckRT(const float* R, const float* t, const float* vKeys1, int n1, const float* vKeys2,
                 const std::vector<std::pair<int, int>>& vMatches12, const uint8_t* vbMatchesInliers, const float* K,
                 float* vP3D, float th2, uint8_t* vbGood, int acos_variant, float* errs) {
    const float fx = K[0];
    const float fy = K[4];
    const float cx = K[2];
    const float cy = K[5];
    std::fill(vbGood, vbGood + n1, 0);
    std::fill(vP3D, vP3D + 3 * (size_t)n1, 0.0f);
    std::vector<float> vCosParallax;
    const bool plain = acos_variant == 2;
    if (errs) std::fill(errs, errs + 2 * (size_t)n1, std::nanf(""));
    float P1[12] = {K[0], K[1], K[2], 0, K[3], K[4], K[5], 0, K[6], K[7], K[8], 0};
    const float O1[3] = {0, 0, 0};
    float Rt[12], P2[12];
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) Rt[r * 4 + c] = R[r * 3 + c];
        Rt[r * 4 + 3] = t[r];
    }
    for (int i = 0; i < 3; i++)  // P2 = K*P2: gemm's short path, 3 x 3 by 3 x 4
        for (int j = 0; j < 4; j++) {
            float s = K[3 * i] * Rt[j] + K[3 * i + 1] * Rt[4 + j] + K[3 * i + 2] * Rt[8 + j];
            P2[i * 4 + j] = (float)((double)s * 1.0);
        }
    float O2[3];
    gemm_general(R, true, t, false, 1, -1.0, O2);  // -R.t()*t: one gemm, GEMM_1_T, alpha = -1
    int nGood = 0;
    for (size_t i = 0, iend = vMatches12.size(); i < iend; i++) {
        if (!vbMatchesInliers[i]) continue;
        const float* kp1 = vKeys1 + 2 * vMatches12[i].first;
        const float* kp2 = vKeys2 + 2 * vMatches12[i].second;
        float p3dC1[3];
        Triangulate(kp1, kp2, P1, P2, p3dC1);
        if (!std::isfinite(p3dC1[0]) || !std::isfinite(p3dC1[1]) || !std::isfinite(p3dC1[2])) {
            vbGood[vMatches12[i].first] = false;
            continue;
        }
        float normal1[3], normal2[3];
        ocv::sub3(p3dC1, O1, normal1);
        float dist1 = ocv::norm3(normal1);
        ocv::sub3(p3dC1, O2, normal2);
        float dist2 = ocv::norm3(normal2);
        float cosParallax = ocv::dot3(normal1, normal2) / (dist1 * dist2);
        if (p3dC1[2] <= 0 && cosParallax < 0.99998) continue;
        float p3dC2[3];
        ocv::gemm3_add(R, p3dC1, t, p3dC2);
        if (p3dC2[2] <= 0 && cosParallax < 0.99998) continue;
        float im1x, im1y;
        float invZ1 = 1.0 / p3dC1[2];
        im1x = plain ? fx * p3dC1[0] * invZ1 + cx : fmaf(fx * p3dC1[0], invZ1, cx);
        im1y = plain ? fy * p3dC1[1] * invZ1 + cy : fmaf(fy * p3dC1[1], invZ1, cy);
        float squareError1 = plain ? (im1x - kp1[0]) * (im1x - kp1[0]) + (im1y - kp1[1]) * (im1y - kp1[1])
                                   : fmaf(im1x - kp1[0], im1x - kp1[0], (im1y - kp1[1]) * (im1y - kp1[1]));
        if (errs) errs[2 * vMatches12[i].first] = squareError1;
        if (squareError1 > th2) continue;
        float im2x, im2y;
        float invZ2 = 1.0 / p3dC2[2];
        im2x = plain ? fx * p3dC2[0] * invZ2 + cx : fmaf(fx * p3dC2[0], invZ2, cx);
        im2y = plain ? fy * p3dC2[1] * invZ2 + cy : fmaf(fy * p3dC2[1], invZ2, cy);
        float squareError2 = plain ? (im2x - kp2[0]) * (im2x - kp2[0]) + (im2y - kp2[1]) * (im2y - kp2[1])
                                   : fmaf(im2x - kp2[0], im2x - kp2[0], (im2y - kp2[1]) * (im2y - kp2[1]));
        if (errs) errs[2 * vMatches12[i].first + 1] = squareError2;
        if (squareError2 > th2) continue;
        vCosParallax.push_back(cosParallax);
        std::memcpy(vP3D + 3 * (size_t)vMatches12[i].first, p3dC1, 12);
        nGood++;
        if (cosParallax < 0.99998) vbGood[vMatches12[i].first] = true;
    }
    CheckOut o;
    o.nGood = nGood;
    o.cosSel = std::nanf("");
    if (nGood > 0) {
        // std::sort is undefined with a NaN in the range; the choice here and in the kernel: a NaN
        // sorts after every number
        std::sort(vCosParallax.begin(), vCosParallax.end(),
                  [](float a, float b) { return a < b || (!std::isnan(a) && std::isnan(b)); });
        size_t idx = std::min(50, int(vCosParallax.size() - 1));
        float ac = acosf(vCosParallax[idx]);
        if (acos_variant > 0) ac = std::nextafterf(ac, INFINITY);
        if (acos_variant < 0) ac = std::nextafterf(ac, -INFINITY);
        o.parallax = ac * 180 / 3.1415926535897932384626433832795;
        o.cosSel = vCosParallax[idx];
    } else
        o.parallax = 0;
    return o;
}

void DecomposeE(const float* E, float* R1, float* R2, float* t) {
    float w[3], u[9], vt[9];
    SVDecomp(E, 3, 3, w, u, vt);
    const float col[3] = {u[2], u[5], u[8]};
    scale(col, 3, 1. / ocv::norm3(col), t);  // t = t/cv::norm(t)
    const float W[9] = {0, -1, 0, 1, 0, 0, 0, 0, 1};
    float uW[9];
    mul3(u, W, uW);  // R1 = u*W*vt
    mul3(uW, vt, R1);
    if (det3(R1) < 0) negate(R1, 9, R1);
    gemm_general(u, false, W, true, 3, 1.0, uW);  // R2 = u*W.t()*vt: the first product is GEMM_2_T
    mul3(uW, vt, R2);
    if (det3(R2) < 0) negate(R2, 9, R2);
}

int RuleF(const int* nGood, const float* parallax, int N, float minParallax, int minTriangulated) {
    int maxGood = std::max(nGood[0], std::max(nGood[1], std::max(nGood[2], nGood[3])));
    int nMinGood = std::max(static_cast<int>(0.9 * N), minTriangulated);
    int nsimilar = 0;
    for (int k = 0; k < 4; k++)
        if (nGood[k] > 0.7 * maxGood) nsimilar++;
    if (maxGood < nMinGood || nsimilar > 1) return -1;
    for (int k = 0; k < 4; k++)  // the else-if chain: the first equal to maxGood decides alone
        if (maxGood == nGood[k]) return parallax[k] > minParallax ? k : -1;
    return -1;
}

int RuleH(const int* nGoods, const float* parallax, int N, float minParallax, int minTriangulated) {
    int bestGood = 0;
    int secondBestGood = 0;
    int bestSolutionIdx = -1;
    float bestParallax = -1;
    for (size_t i = 0; i < 8; i++) {
        int nGood = nGoods[i];
        if (nGood > bestGood) {
            secondBestGood = bestGood;
            bestGood = nGood;
            bestSolutionIdx = i;
            bestParallax = parallax[i];
        } else if (nGood > secondBestGood)
            secondBestGood = nGood;
    }
    if (secondBestGood < 0.75 * bestGood && bestParallax >= minParallax && bestGood > minTriangulated &&
        bestGood > 0.9 * N)
        return bestSolutionIdx;
    return -1;
}

// The 4 motions of ReconstructF in the order CheckRT sees them.  Returns n_motion = 4.
int MotionF(const float* F21, const float* K, float* vR, float* vt) {
    float tmp[9], E21[9];
    gemm_general(K, true, F21, false, 3, 1.0, tmp);  // K.t()*F21: GEMM_1_T
    mul3(tmp, K, E21);
    float R1[9], R2[9], t1[3], t2[3];
    DecomposeE(E21, R1, R2, t1);
    negate(t1, 3, t2);
    const float* Rs[4] = {R1, R2, R1, R2};
    const float* ts[4] = {t1, t1, t2, t2};
    for (int k = 0; k < 4; k++) {
        std::memcpy(vR + 9 * k, Rs[k], 36);
        std::memcpy(vt + 3 * k, ts[k], 12);
    }
    return 4;
}

// The 8 motions of ReconstructH (Faugeras), or 0 when the singular values fail the gate.  vn is
// computed by the reference and never read: not modelled.  d: the three singular values.
int MotionH(const float* H21, const float* K, float* vR, float* vt, float* d) {
    float invK[9], tmp[9], A[9];
    inv3(K, invK);
    mul3(invK, H21, tmp);
    mul3(tmp, K, A);
    float w[3], U[9], Vt[9];
    SVDecomp(A, 3, 3, w, U, Vt);
    float s = det3(U) * det3(Vt);
    float d1 = w[0];
    float d2 = w[1];
    float d3 = w[2];
    if (d) d[0] = d1, d[1] = d2, d[2] = d3;
    if (d1 / d2 < 1.00001 || d2 / d3 < 1.00001) return 0;
    // (the contraction of the reference build: d1*d1 is not shared, each difference is one fmsub)
    const float d22 = d2 * d2, d33 = d3 * d3, d13 = d1 * d3;
    const float n12 = fmaf(d1, d1, -d22), n13 = fmaf(d1, d1, -d33), n23 = d22 - d33;
    float aux1 = sqrtf(n12 / n13);
    float aux3 = sqrtf(n23 / n13);
    float x1[] = {aux1, aux1, -aux1, -aux1};
    float x3[] = {aux3, -aux3, aux3, -aux3};
    float aux_stheta = sqrtf(n12 * n23) / ((d1 + d3) * d2);
    float ctheta = (d22 + d13) / ((d1 + d3) * d2);
    float stheta[] = {aux_stheta, -aux_stheta, -aux_stheta, aux_stheta};
    for (int i = 0; i < 4; i++) {
        float Rp[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        Rp[0] = ctheta;
        Rp[2] = -stheta[i];
        Rp[6] = stheta[i];
        Rp[8] = ctheta;
        mul3_alpha(U, Rp, s, tmp);  // R = s*U*Rp*Vt: gemm(U, Rp, alpha = s), then * Vt
        mul3(tmp, Vt, vR + 9 * i);
        float tp[3] = {x1[i], 0, -x3[i]};
        scale(tp, 3, d1 - d3, tp);  // tp *= d1-d3
        float t[3];
        for (int r = 0; r < 3; r++) {  // U*tp: gemm's short path, 3 x 3 by 3 x 1
            float a = U[3 * r] * tp[0] + U[3 * r + 1] * tp[1] + U[3 * r + 2] * tp[2];
            t[r] = (float)((double)a * 1.0);
        }
        scale(t, 3, 1. / ocv::norm3(t), vt + 3 * i);
    }
    float aux_sphi = sqrtf(n12 * n23) / ((d1 - d3) * d2);
    float cphi = (d13 - d22) / ((d1 - d3) * d2);
    float sphi[] = {aux_sphi, -aux_sphi, -aux_sphi, aux_sphi};
    for (int i = 0; i < 4; i++) {
        float Rp[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        Rp[0] = cphi;
        Rp[2] = sphi[i];
        Rp[4] = -1;
        Rp[6] = sphi[i];
        Rp[8] = -cphi;
        mul3_alpha(U, Rp, s, tmp);
        mul3(tmp, Vt, vR + 9 * (4 + i));
        float tp[3] = {x1[i], 0, x3[i]};
        scale(tp, 3, d1 + d3, tp);  // tp *= d1+d3
        float t[3];
        for (int r = 0; r < 3; r++) {
            float a = U[3 * r] * tp[0] + U[3 * r + 1] * tp[1] + U[3 * r + 2] * tp[2];
            t[r] = (float)((double)a * 1.0);
        }
        scale(t, 3, 1. / ocv::norm3(t), vt + 3 * (4 + i));
    }
    return 8;
}

}  // namespace

extern "C" {

int initializer_reconstruct_model_rule_f(const int32_t* nGood, const float* parallax, int N, float minParallax,
                                         int minTriangulated) {
    return RuleF(nGood, parallax, N, minParallax, minTriangulated);
}
int initializer_reconstruct_model_rule_h(const int32_t* nGood, const float* parallax, int N, float minParallax,
                                         int minTriangulated) {
    return RuleH(nGood, parallax, N, minParallax, minTriangulated);
}
// Triangulate on one correspondence with two 3 x 4 projection matrices
void initializer_reconstruct_model_triangulate(const float* kp1, const float* kp2, const float* P1, const float* P2,
                                               float* x3D) {
    Triangulate(kp1, kp2, P1, P2, x3D);
}
void initializer_reconstruct_model_decompose_e(const float* E, float* R1, float* R2, float* t) {
    DecomposeE(E, R1, R2, t);
}
// The motion hypotheses alone: R (8 x 9), t (8 x 3), d (3 singular values, H only; may be NULL)
int initializer_reconstruct_model_motions(const float* M21, int use_h, const float* K4, float* vR, float* vt, float* d) {
    float K[9];
    make_K(K4, K);
    return use_h ? MotionH(M21, K, vR, vt, d) : MotionF(M21, K, vR, vt);
}

// Inputs as orb_initializer_reconstruct, keypoints as n x 2 floats.  Outputs (any may be NULL) as
// there, plus hyp_P3D (8 x n1 x 3), hyp_good (8 x n1) and hyp_err (8 x n1 x 2): vP3D, vbGood and the two
// squared reprojection errors of every hypothesis.
// Returns -22 for a matches12 entry outside [-1, n2).
int initializer_reconstruct_model(const float* kps1_xy, int n1, const float* kps2_xy, int n2, const int32_t* matches12,
                                  const float* M21, int use_h, const uint8_t* inliers, const float* K4, float sigma,
                                  float minParallax, int minTriangulated, int acos_variant, int32_t* ok, float* R21,
                                  float* t21, float* P3D, uint8_t* triangulated, int32_t* n_motion, float* motion_R,
                                  float* motion_t, int32_t* n_good, float* cos_parallax, float* parallax_deg,
                                  int32_t* best, int32_t* n_inliers, float* hyp_P3D, uint8_t* hyp_good,
                                  float* hyp_err) {
    std::vector<std::pair<int, int>> mvMatches12;
    for (int i = 0; i < n1; i++) {
        if (matches12[i] < -1 || matches12[i] >= n2) return -22;
        if (matches12[i] >= 0) mvMatches12.push_back(std::make_pair(i, matches12[i]));
    }
    int N = 0;
    for (size_t i = 0, iend = mvMatches12.size(); i < iend; i++)
        if (inliers[i]) N++;
    float K[9];
    make_K(K4, K);
    const float mSigma2 = sigma * sigma;
    const float th2 = 4.0 * mSigma2;
    float vR[72], vt[24];
    std::fill(vR, vR + 72, 0.0f);
    std::fill(vt, vt + 24, 0.0f);
    const int nm = use_h ? MotionH(M21, K, vR, vt, nullptr) : MotionF(M21, K, vR, vt);
    int nGood[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    float par[8], cs[8];
    for (int k = 0; k < 8; k++) par[k] = 0, cs[k] = std::nanf("");
    std::vector<float> P((size_t)8 * 3 * std::max(n1, 1), 0.0f);
    std::vector<uint8_t> G((size_t)8 * std::max(n1, 1), 0);
    std::vector<float> Er((size_t)8 * 2 * std::max(n1, 1), std::nanf(""));
    for (int k = 0; k < nm; k++) {
        CheckOut c = CheckRT(vR + 9 * k, vt + 3 * k, kps1_xy, n1, kps2_xy, mvMatches12, inliers, K,
                             P.data() + (size_t)k * 3 * n1, th2, G.data() + (size_t)k * n1, acos_variant,
                             Er.data() + (size_t)k * 2 * n1);
        nGood[k] = c.nGood;
        par[k] = c.parallax;
        cs[k] = c.cosSel;
    }
    int b = -1;
    if (nm == 4) b = RuleF(nGood, par, N, minParallax, minTriangulated);
    if (nm == 8) b = RuleH(nGood, par, N, minParallax, minTriangulated);
    if (ok) *ok = b >= 0;
    if (best) *best = b;
    if (n_inliers) *n_inliers = N;
    if (n_motion) *n_motion = nm;
    if (motion_R) std::memcpy(motion_R, vR, sizeof(vR));
    if (motion_t) std::memcpy(motion_t, vt, sizeof(vt));
    if (n_good) std::memcpy(n_good, nGood, sizeof(nGood));
    if (cos_parallax) std::memcpy(cos_parallax, cs, sizeof(cs));
    if (parallax_deg) std::memcpy(parallax_deg, par, sizeof(par));
    if (R21) std::fill(R21, R21 + 9, 0.0f);
    if (t21) std::fill(t21, t21 + 3, 0.0f);
    if (P3D) std::fill(P3D, P3D + 3 * (size_t)n1, 0.0f);
    if (triangulated) std::fill(triangulated, triangulated + n1, 0);
    if (b >= 0) {
        if (R21) std::memcpy(R21, vR + 9 * b, 36);
        if (t21) std::memcpy(t21, vt + 3 * b, 12);
        if (P3D && n1) std::memcpy(P3D, P.data() + (size_t)b * 3 * n1, 12 * (size_t)n1);
        if (triangulated && n1) std::memcpy(triangulated, G.data() + (size_t)b * n1, n1);
    }
    if (hyp_P3D && n1) std::memcpy(hyp_P3D, P.data(), 4 * (size_t)8 * 3 * n1);
    if (hyp_good && n1) std::memcpy(hyp_good, G.data(), (size_t)8 * n1);
    if (hyp_err && n1) std::memcpy(hyp_err, Er.data(), 4 * (size_t)8 * 2 * n1);
    return 0;
}

}  // extern "C"

#ifdef INITIALIZER_RECONSTRUCT_MODEL_MAIN
// Stand-alone run for the sanitizers: argv[1] = a file of int32 n1, n2, use_h, then K4, sigma (5
// floats), the 9 floats of the model, n1 x 2 and n2 x 2 floats, n1 matches, n1 mask bytes (by match
// ordinal, the tail unused).  Prints the decision and a checksum.
int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hdr[3];
    float cal[5], M[9];
    if (std::fread(hdr, 4, 3, f) != 3 || std::fread(cal, 4, 5, f) != 5 || std::fread(M, 4, 9, f) != 9) return 2;
    const int n1 = hdr[0], n2 = hdr[1], use_h = hdr[2];
    std::vector<float> k1(2 * (size_t)n1), k2(2 * (size_t)n2), P3D(3 * (size_t)n1);
    std::vector<int32_t> m12(n1);
    std::vector<uint8_t> inl(n1), tri(n1);
    if (std::fread(k1.data(), 4, k1.size(), f) != k1.size() || std::fread(k2.data(), 4, k2.size(), f) != k2.size() ||
        std::fread(m12.data(), 4, m12.size(), f) != m12.size() || std::fread(inl.data(), 1, inl.size(), f) != inl.size())
        return 2;
    std::fclose(f);
    int32_t ok = 0, best = -1, nm = 0, ng[8], N = 0;
    float R[9], t[3], mR[72], mt[24], cs[8], pd[8];
    int r = initializer_reconstruct_model(k1.data(), n1, k2.data(), n2, m12.data(), M, use_h, inl.data(), cal, cal[4],
                                          1.0f, 50, 0, &ok, R, t, P3D.data(), tri.data(), &nm, mR, mt, ng, cs, pd, &best,
                                          &N, nullptr, nullptr, nullptr);
    double sum = 0;
    for (float v : P3D) sum += std::fabs(v);
    std::printf("initializer reconstruct model: status %d ok %d best %d n_motion %d N %d checksum %.17g\n", r, (int)ok,
                (int)best, (int)nm, (int)N, sum);
    return r ? 1 : 0;
}
#endif
