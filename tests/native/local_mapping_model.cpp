// CPU model of csrc/orb_localmap.hip and of orb_update_normal_and_depth: LocalMapping::CreateNewMapPoints'
// neighbour-loop body and ComputeF12 (src/LocalMapping.cc:256-391, 474-491), KeyFrame::ComputeSceneMedianDepth
// (src/KeyFrame.cc:659-689) and MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:273-312) of the reference,
// restated statement for statement, with the OpenCV 2.4 expressions they are written in restated as read
// (DESIGN.md §20 lists every one).  No OpenCV 2.4 source or binary is at hand: parity with a real build is
// unpinned.  The SVD, inv() and the 3 x 3 short product are those of initializer_ransac_model.cpp, included
// below and not copied; norm, dot, subtract and A*x+t are oracle/ocv_ops.cpp's.  Built -ffp-contract=off; the
// three fused multiply-adds per image that g++ -O3 -march=native makes of the reprojection lines are written
// out as fmaf (scripts/contraction_check_local_mapping.sh).  Shares nothing with the .hip files.
// -DLOCAL_MAPPING_MODEL_MAIN adds a main() for the sanitizer run.
#include "initializer_ransac_model.cpp"

#include <algorithm>

#include "../../oracle/ocv_ops.h"

namespace {

// gemm with a transpose flag leaves the 2 <= len <= 4 path for GEMMSingleMul_<float, double>: one double
// accumulator per element, k ascending, times alpha, narrowed.  d = alpha * a * b.t(), 3 x 3.
void gemm_abt(const float* a, const float* b, double alpha, float* d) {
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double s0 = 0;
            for (int k = 0; k < 3; k++) s0 += (double)a[i * 3 + k] * (double)b[j * 3 + k];
            d[i * 3 + j] = (float)(s0 * alpha);
        }
}

// GetCameraCenter: Ow = -Rcw.t()*tcw, one gemm, GEMM_1_T, alpha = -1
void Center(const float* T, float* Ow) {
    for (int i = 0; i < 3; i++) {
        double s0 = 0;
        for (int k = 0; k < 3; k++) s0 += (double)T[k * 3 + i] * (double)T[9 + k];
        Ow[i] = (float)(s0 * -1.0);
    }
}

void make_K(const float* K4, float* K) {
    const float k[9] = {K4[0], 0, K4[2], 0, K4[1], K4[3], 0, 0, 1};
    std::memcpy(K, k, sizeof(k));
}

void ComputeF12(const float* R1w, const float* t1w, const float* R2w, const float* t2w, const float* K1_4,
                const float* K2_4, float* F12) {
    float R12[9];
    gemm_abt(R1w, R2w, 1.0, R12);  // R1w*R2w.t()
    // -R1w*R2w.t()*t2w+t1w: (-R1w)*R2w.t() is gemm(R1w, R2w, -1, GEMM_2_T), evaluated; then (M*t2w)+t1w
    // is one gemm(M, t2w, 1, t1w, 1)
    float M[9], t12[3];
    gemm_abt(R1w, R2w, -1.0, M);
    ocv::gemm3_add(M, t2w, t1w, t12);
    const float t12x[9] = {0, -t12[2], t12[1], t12[2], 0, -t12[0], -t12[1], t12[0], 0};  // SkewSymmetricMatrix
    float K1[9], K2[9], K1t[9], iK1t[9], iK2[9], a[9], b[9];
    make_K(K1_4, K1);
    make_K(K2_4, K2);
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) K1t[r * 3 + c] = K1[c * 3 + r];  // K1.t(), evaluated by inv()
    inv3(K1t, iK1t);
    inv3(K2, iK2);
    mul3(iK1t, t12x, a);  // K1.t().inv()*t12x*R12*K2.inv(), left to right, the short path
    mul3(a, R12, b);
    mul3(b, iK2, F12);
}

// a NaN sorts after every number (std::sort is undefined with a NaN under operator<)
bool nan_last(float a, float b) { return a < b || (!std::isnan(a) && std::isnan(b)); }

// ComputeSceneMedianDepth(q): the number of depths; *depth = NaN when there is none
int SceneMedianDepth(const float* T, const float* mp_pos, const uint8_t* has_mp, int n, int q, float* depth) {
    std::vector<float> vDepths;
    const float* Rcw2 = T + 6;
    float zcw = T[11];
    for (int i = 0; i < n; i++)
        if (has_mp[i]) {
            float z = ocv::dot3(Rcw2, mp_pos + 3 * (size_t)i) + zcw;
            vDepths.push_back(z);
        }
    *depth = std::nanf("");
    if (vDepths.empty()) return 0;
    std::sort(vDepths.begin(), vDepths.end(), nan_last);
    *depth = vDepths[(vDepths.size() - 1) / q];
    return (int)vDepths.size();
}

// M / s: MatOp_AddEx with alpha = 1./s -> convertTo(m, type, alpha, 0): x * (float)alpha + (float)0
void scale(const float* x, int n, double alpha, float* out) {
    const float a = (float)alpha, b = (float)0.0;
    for (int i = 0; i < n; i++) out[i] = x[i] * a + b;
}

// The 4 x 4 system of lines 310-325: rows from the two normalised points and the two 3 x 4 poses
// (row-major 3 x 4), the decomposition, vt.row(3).  Returns false when x3D.at<float>(3) == 0.
bool Triangulate4(const float* xn1, const float* xn2, const float* Tcw1, const float* Tcw2, float* x3D) {
    float A[16];
    // A.row(r) = xn*Tcw.row(2) - Tcw.row(r): MatOp_AddEx(a, b, alpha = xn, beta = -1) -> addWeighted_<float, double>
    const float xs[4] = {xn1[0], xn1[1], xn2[0], xn2[1]};
    const float* Ts[4] = {Tcw1, Tcw1, Tcw2, Tcw2};
    for (int r = 0; r < 4; r++)
        for (int j = 0; j < 4; j++)
            A[r * 4 + j] = (float)((double)Ts[r][8 + j] * (double)xs[r] + (double)Ts[r][(r & 1) * 4 + j] * -1.0 + 0.0);
    float w[4], u[16], vt[16];
    SVDecomp(A, 4, 4, w, u, vt);
    if (vt[15] == 0) return false;
    scale(vt + 12, 3, 1. / (double)vt[15], x3D);  // x3D.rowRange(0,3)/x3D.at<float>(3)
    return true;
}

struct Cam {
    float Rcw[9], Rwc[9], tcw[3], Tcw[12], Ow[3];
    float fx, fy, cx, cy, invfx, invfy;
    const float* sf;
    const float* s2;
    int nlevels;
    float ScaleFactor(int o) const { return sf[std::min(std::max(o, 0), nlevels - 1)]; }
    float Sigma2(int o) const { return s2[std::min(std::max(o, 0), nlevels - 1)]; }
};

Cam make_cam(const float* T, const float* Ow, const float* K4, const float* sf, const float* s2, int nlevels) {
    Cam c;
    std::memcpy(c.Rcw, T, 36);
    std::memcpy(c.tcw, T + 9, 12);
    for (int r = 0; r < 3; r++) {
        for (int k = 0; k < 3; k++) {
            c.Rwc[r * 3 + k] = T[k * 3 + r];
            c.Tcw[r * 4 + k] = T[r * 3 + k];
        }
        c.Tcw[r * 4 + 3] = T[9 + r];
    }
    std::memcpy(c.Ow, Ow, 12);
    c.fx = K4[0], c.fy = K4[1], c.cx = K4[2], c.cy = K4[3];
    c.invfx = 1.0f / c.fx;
    c.invfy = 1.0f / c.fy;
    c.sf = sf, c.s2 = s2, c.nlevels = nlevels;
    return c;
}

// Rwc*xn: gemm's short path, 3 x 3 by 3 x 1
void mulv(const float* A, const float* x, float* out) {
    for (int i = 0; i < 3; i++) {
        float t = A[3 * i] * x[0] + A[3 * i + 1] * x[1] + A[3 * i + 2] * x[2];
        out[i] = (float)((double)t * 1.0);
    }
}

// One match of lines 293-391.  plain: the reprojection lines without their fused multiply-adds.
// dbg (6, may be NULL): the two squared errors, ratioDist, ratioOctave, z1, z2 where computed, NaN before.
int TriangulateOne(const Cam& c1, const Cam& c2, const float* kp1, int octave1, const float* kp2, int octave2,
                   float ratioFactor, bool plain, float* cosOut, float* x3Dout, float* dbg) {
    x3Dout[0] = x3Dout[1] = x3Dout[2] = 0;
    if (dbg) std::fill(dbg, dbg + 6, std::nanf(""));
    const float xn1[3] = {(kp1[0] - c1.cx) * c1.invfx, (kp1[1] - c1.cy) * c1.invfy, 1.0};
    float ray1[3];
    mulv(c1.Rwc, xn1, ray1);
    const float xn2[3] = {(kp2[0] - c2.cx) * c2.invfx, (kp2[1] - c2.cy) * c2.invfy, 1.0};
    float ray2[3];
    mulv(c2.Rwc, xn2, ray2);
    const float cosParallaxRays = ocv::dot3(ray1, ray2) / (ocv::norm3(ray1) * ocv::norm3(ray2));
    *cosOut = cosParallaxRays;
    if (cosParallaxRays < 0 || cosParallaxRays > 0.9998) return 2;
    float x3D[3];
    if (!Triangulate4(xn1, xn2, c1.Tcw, c2.Tcw, x3D)) return 3;
    std::memcpy(x3Dout, x3D, 12);
    float z1 = ocv::dot3(c1.Rcw + 6, x3D) + c1.tcw[2];
    if (dbg) dbg[4] = z1;
    if (z1 <= 0) return 4;
    float z2 = ocv::dot3(c2.Rcw + 6, x3D) + c2.tcw[2];
    if (dbg) dbg[5] = z2;
    if (z2 <= 0) return 5;
    float sigmaSquare1 = c1.Sigma2(octave1);
    float x1 = ocv::dot3(c1.Rcw, x3D) + c1.tcw[0];
    float y1 = ocv::dot3(c1.Rcw + 3, x3D) + c1.tcw[1];
    float invz1 = 1.0 / z1;
    float u1 = plain ? c1.fx * x1 * invz1 + c1.cx : fmaf(c1.fx * x1, invz1, c1.cx);
    float v1 = plain ? c1.fy * y1 * invz1 + c1.cy : fmaf(c1.fy * y1, invz1, c1.cy);
    float errX1 = u1 - kp1[0];
    float errY1 = v1 - kp1[1];
    // (the reference build rounds errY*errY and fuses errX*errX into the sum, as in CheckRT)
    const float e1 = plain ? errX1 * errX1 + errY1 * errY1 : fmaf(errX1, errX1, errY1 * errY1);
    if (dbg) dbg[0] = e1;
    if (e1 > 5.991 * sigmaSquare1) return 6;
    float sigmaSquare2 = c2.Sigma2(octave2);
    float x2 = ocv::dot3(c2.Rcw, x3D) + c2.tcw[0];
    float y2 = ocv::dot3(c2.Rcw + 3, x3D) + c2.tcw[1];
    float invz2 = 1.0 / z2;
    float u2 = plain ? c2.fx * x2 * invz2 + c2.cx : fmaf(c2.fx * x2, invz2, c2.cx);
    float v2 = plain ? c2.fy * y2 * invz2 + c2.cy : fmaf(c2.fy * y2, invz2, c2.cy);
    float errX2 = u2 - kp2[0];
    float errY2 = v2 - kp2[1];
    const float e2 = plain ? errX2 * errX2 + errY2 * errY2 : fmaf(errX2, errX2, errY2 * errY2);
    if (dbg) dbg[1] = e2;
    if (e2 > 5.991 * sigmaSquare2) return 7;
    float normal1[3], normal2[3];
    ocv::sub3(x3D, c1.Ow, normal1);
    float dist1 = ocv::norm3(normal1);
    ocv::sub3(x3D, c2.Ow, normal2);
    float dist2 = ocv::norm3(normal2);
    if (dist1 == 0 || dist2 == 0) return 8;
    float ratioDist = dist1 / dist2;
    float ratioOctave = c1.ScaleFactor(octave1) / c2.ScaleFactor(octave2);
    if (dbg) dbg[2] = ratioDist, dbg[3] = ratioOctave;
    if (ratioDist * ratioFactor < ratioOctave || ratioDist > ratioOctave * ratioFactor) return 9;
    return 1;
}

}  // namespace

extern "C" {

void local_mapping_model_compute_f12(const float* R1w, const float* t1w, const float* R2w, const float* t2w,
                                     const float* K1, const float* K2, float* F12) {
    ComputeF12(R1w, t1w, R2w, t2w, K1, K2, F12);
}

void local_mapping_model_center(const float* pose12, float* Ow) { Center(pose12, Ow); }

int local_mapping_model_median(const float* pose12, const float* mp_pos, const uint8_t* has_mp, int n, int q,
                               float* depth) {
    return SceneMedianDepth(pose12, mp_pos, has_mp, n, q, depth);
}

// the point of one normalised correspondence and two 3 x 4 poses; 0 when the fourth coordinate is 0
int local_mapping_model_triangulate4(const float* xn1, const float* xn2, const float* Tcw1, const float* Tcw2,
                                     float* x3D) {
    return Triangulate4(xn1, xn2, Tcw1, Tcw2, x3D) ? 1 : 0;
}

// Inputs as orb_create_new_map_points with the keypoints as n x 2 floats and n octaves, poses as 12 floats
// (Rcw row-major, tcw), Ow 3 each, K 4 each, tables of nlevels floats.  mp_pos2 / has_mp2 NULL: no gate.
// Outputs (any may be NULL) as there, plus dbg (n1 x 6): the two squared reprojection errors, ratioDist,
// ratioOctave, z1, z2 of every match that got as far as computing them, NaN elsewhere.  variant 2: the
// reprojection lines without their fused multiply-adds.  Returns -22 for a match12 entry outside
// [-1, n2) or a gate on a keyframe without a MapPoint.
int local_mapping_model_create(const float* kps1_xy, const int32_t* oct1, int n1, const float* kps2_xy,
                               const int32_t* oct2, int n2, const int32_t* match12, const float* pose1, const float* Ow1,
                               const float* pose2, const float* Ow2, const float* K1, const float* K2, const float* sf1,
                               const float* s21, int nl1, const float* sf2, const float* s22, int nl2,
                               const float* mp_pos2, const uint8_t* has_mp2, int variant, float* x3d, uint8_t* status,
                               float* cos_rays, int32_t* n_new, int32_t* new_idx1, int32_t* new_idx2, int32_t* skipped,
                               float* median_depth, float* dbg) {
    std::vector<std::pair<int, int>> vMatchedIndices;
    for (int i = 0; i < n1; i++) {
        if (match12[i] < -1 || match12[i] >= n2) return -22;
        if (match12[i] >= 0) vMatchedIndices.push_back(std::make_pair(i, match12[i]));
    }
    if (x3d) std::fill(x3d, x3d + 3 * (size_t)n1, 0.0f);
    if (status) std::fill(status, status + n1, 0);
    if (cos_rays) std::fill(cos_rays, cos_rays + n1, std::nanf(""));
    if (new_idx1) std::fill(new_idx1, new_idx1 + n1, -1);
    if (new_idx2) std::fill(new_idx2, new_idx2 + n1, -1);
    if (dbg) std::fill(dbg, dbg + 6 * (size_t)n1, std::nanf(""));
    if (n_new) *n_new = 0;
    if (skipped) *skipped = 0;
    if (median_depth) *median_depth = std::nanf("");
    const Cam c1 = make_cam(pose1, Ow1, K1, sf1, s21, nl1), c2 = make_cam(pose2, Ow2, K2, sf2, s22, nl2);
    const float ratioFactor = 1.5f * sf1[1];  // 1.5f*mpCurrentKeyFrame->GetScaleFactor(): mvScaleFactors[1]
    if (mp_pos2) {
        float vBaseline[3];
        ocv::sub3(c2.Ow, c1.Ow, vBaseline);
        const float baseline = ocv::norm3(vBaseline);
        float medianDepthKF2;
        if (SceneMedianDepth(pose2, mp_pos2, has_mp2, n2, 2, &medianDepthKF2) == 0) return -22;
        if (median_depth) *median_depth = medianDepthKF2;
        const float ratioBaselineDepth = baseline / medianDepthKF2;
        if (ratioBaselineDepth < 0.01) {
            if (skipped) *skipped = 1;
            return 0;
        }
    }
    int nn = 0;
    for (size_t ikp = 0, iendkp = vMatchedIndices.size(); ikp < iendkp; ikp++) {
        const int idx1 = vMatchedIndices[ikp].first;
        const int idx2 = vMatchedIndices[ikp].second;
        float cs, p[3], d[6];
        const int st = TriangulateOne(c1, c2, kps1_xy + 2 * idx1, oct1[idx1], kps2_xy + 2 * idx2, oct2[idx2], ratioFactor,
                                      variant == 2, &cs, p, d);
        if (status) status[idx1] = (uint8_t)st;
        if (cos_rays) cos_rays[idx1] = cs;
        if (x3d) std::memcpy(x3d + 3 * (size_t)idx1, p, 12);
        if (dbg) std::memcpy(dbg + 6 * (size_t)idx1, d, 24);
        if (st == 1) {
            if (new_idx1) new_idx1[nn] = idx1;
            if (new_idx2) new_idx2[nn] = idx2;
            nn++;
        }
    }
    if (n_new) *n_new = nn;
    return 0;
}

void local_mapping_model_update_normal_and_depth(int M, const int32_t* offsets, const float* obs_Ow, const float* pos,
                                                 const float* ref_Ow, const int32_t* ref_level, const float* sf,
                                                 int nLevels, float* normal_out, float* dmin, float* dmax) {
    for (int m = 0; m < M; m++) {
        const float* Pos = pos + 3 * (size_t)m;
        float normal[3] = {0, 0, 0};
        int n = 0;
        for (int r = offsets[m]; r < offsets[m + 1]; r++) {
            float normali[3];
            ocv::sub3(Pos, obs_Ow + 3 * (size_t)r, normali);
            // normal = normal + normali/cv::norm(normali): MatOp_AddEx(normali, normal, alpha = 1./norm, beta = 1)
            // -> addWeighted_<float, double>
            const double alpha = 1. / ocv::norm3(normali);
            for (int k = 0; k < 3; k++) normal[k] = (float)((double)normali[k] * alpha + (double)normal[k] * 1.0 + 0.0);
            n++;
        }
        float PC[3];
        ocv::sub3(Pos, ref_Ow + 3 * (size_t)m, PC);
        const float dist = ocv::norm3(PC);
        const int level = std::min(std::max(ref_level[m], 0), nLevels - 1);
        const float scaleFactor = sf[1];
        const float levelScaleFactor = sf[level];
        dmin[m] = (1.0f / scaleFactor) * dist / levelScaleFactor;
        dmax[m] = scaleFactor * dist * sf[nLevels - 1 - level];
        scale(normal, 3, 1. / n, normal_out + 3 * (size_t)m);  // normal/n
    }
}

}  // extern "C"

#ifdef LOCAL_MAPPING_MODEL_MAIN
// Stand-alone run for the sanitizers: a seeded two-view scene built here (no input file), every entry
// point called once, including a keyframe without a match and a point without an observation.  Prints
// the status histogram and a checksum.
int main() {
    unsigned long long s = 88172645463325252ull;
    auto rnd = [&]() {
        s ^= s << 13, s ^= s >> 7, s ^= s << 17;
        return (float)((s >> 11) * (1.0 / 9007199254740992.0));
    };
    const int n = 200, nl = 8;
    float sf[8], s2[8];
    sf[0] = s2[0] = 1;
    for (int i = 1; i < nl; i++) sf[i] = sf[i - 1] * 1.2f, s2[i] = sf[i] * sf[i];
    const float K[4] = {520.9f, 521.0f, 325.1f, 249.7f};
    const float T1[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
    const float T2[12] = {0.9950042f, 0, 0.0998334f, 0, 1, 0, -0.0998334f, 0, 0.9950042f, -0.5f, 0.02f, 0.01f};
    float O1[3], O2[3];
    Center(T1, O1);
    Center(T2, O2);
    std::vector<float> k1(2 * n), k2(2 * n), P(3 * n), x3d(3 * n), cs(n), dbg(6 * n);
    std::vector<int32_t> o1(n), o2(n), m12(n), a1(n), a2(n);
    std::vector<uint8_t> st(n), has(n, 1);
    for (int i = 0; i < n; i++) {
        const float z = 2 + 6 * rnd(), u = 30 + 580 * rnd(), v = 30 + 420 * rnd();
        const float X[3] = {(u - K[2]) / K[0] * z, (v - K[3]) / K[1] * z, z};
        std::memcpy(&P[3 * i], X, 12);
        float Y[3];
        ocv::gemm3_add(T2, X, T2 + 9, Y);
        k1[2 * i] = u + rnd() - 0.5f, k1[2 * i + 1] = v + rnd() - 0.5f;
        k2[2 * i] = K[0] * Y[0] / Y[2] + K[2] + 8 * (rnd() - 0.5f) * (i % 7 == 0);
        k2[2 * i + 1] = K[1] * Y[1] / Y[2] + K[3];
        o1[i] = (int)(rnd() * 3), o2[i] = (int)(rnd() * 3);
        m12[i] = i % 5 == 4 ? -1 : i;
    }
    int32_t nn = 0, sk = 0;
    float med = 0, F[9];
    int r = local_mapping_model_create(k1.data(), o1.data(), n, k2.data(), o2.data(), n, m12.data(), T1, O1, T2, O2, K, K,
                                       sf, s2, nl, sf, s2, nl, P.data(), has.data(), 0, x3d.data(), st.data(), cs.data(),
                                       &nn, a1.data(), a2.data(), &sk, &med, dbg.data());
    std::fill(m12.begin(), m12.end(), -1);
    r |= local_mapping_model_create(k1.data(), o1.data(), n, k2.data(), o2.data(), 0, m12.data(), T1, O1, T2, O2, K, K, sf,
                                    s2, nl, sf, s2, nl, nullptr, nullptr, 2, nullptr, nullptr, nullptr, nullptr, nullptr,
                                    nullptr, nullptr, nullptr, nullptr);
    ComputeF12(T1, T1 + 9, T2, T2 + 9, K, K, F);
    int hist[10] = {0};
    for (int i = 0; i < n; i++) hist[st[i]]++;
    std::vector<int32_t> off = {0, 0, 1, 3, n}, lev = {0, 7, 3, 99};
    std::vector<float> ow(3 * n), nrm(12), dmn(4), dmx(4);
    for (float& v : ow) v = rnd() - 0.5f;
    local_mapping_model_update_normal_and_depth(4, off.data(), ow.data(), P.data(), P.data() + 12, lev.data(), sf, nl,
                                                nrm.data(), dmn.data(), dmx.data());
    double sum = med;
    for (float v : x3d) sum += std::fabs(v);
    for (float v : F) sum += std::fabs(v);
    for (int i = 3; i < 12; i++) sum += std::fabs(nrm[i]) + (i < 4 ? 0 : 0);
    for (int i = 0; i < 4; i++) sum += dmn[i] + dmx[i];
    std::printf("local mapping model: status %d n_new %d skipped %d median %.9g\n", r, (int)nn, (int)sk, med);
    std::printf("  codes:");
    for (int k = 0; k < 10; k++) std::printf(" %d", hist[k]);
    std::printf("\n  checksum %.17g\n", sum);
    return r ? 1 : 0;
}
#endif
