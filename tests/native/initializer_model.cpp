// CPU model of orb_initializer_check: Initializer::CheckHomography (reference
// src/Initializer.cc:303-386), CheckFundamental (388-466) and the best-of loops of FindHomography /
// FindFundamental (146-169, 197-220), restated statement for statement.  Built -ffp-contract=off;
// the fused multiply-adds that g++ -O3 -march=native makes of the reference's expressions
// (scripts/contraction_check_initializer.sh) are written as std::fma.  1.0/(float) stays the
// reference's double division rounded to float.  Single-threaded; scripts/initializer_timing.py
// also times it.
#include <cmath>
#include <cstdint>
#include <utility>
#include <vector>

namespace {

struct Model {
    const float* k1;  // n1 x 2 (pt.x, pt.y of mvKeys1)
    const float* k2;  // n2 x 2
    std::vector<std::pair<int, int>> mvMatches12;
    float sigma;
};

float CheckHomography(const Model& M, const float* H21, const float* H12, std::vector<uint8_t>& vbMatchesInliers,
                      float* terms) {
    const int N = (int)M.mvMatches12.size();
    const float h11 = H21[0], h12 = H21[1], h13 = H21[2], h21 = H21[3], h22 = H21[4], h23 = H21[5], h31 = H21[6],
                h32 = H21[7], h33 = H21[8];
    const float h11inv = H12[0], h12inv = H12[1], h13inv = H12[2], h21inv = H12[3], h22inv = H12[4], h23inv = H12[5],
                h31inv = H12[6], h32inv = H12[7], h33inv = H12[8];
    vbMatchesInliers.resize(N);
    float score = 0;
    const float th = 5.991;
    const float invSigmaSquare = 1.0 / (M.sigma * M.sigma);
    for (int i = 0; i < N; i++) {
        bool bIn = true;
        const float u1 = M.k1[2 * M.mvMatches12[i].first], v1 = M.k1[2 * M.mvMatches12[i].first + 1];
        const float u2 = M.k2[2 * M.mvMatches12[i].second], v2 = M.k2[2 * M.mvMatches12[i].second + 1];
        // x2in1 = H12*x2
        const float w2in1inv = 1.0 / (std::fma(h31inv, u2, h32inv * v2) + h33inv);
        const float pu2 = std::fma(h11inv, u2, h12inv * v2) + h13inv;
        const float pv2 = std::fma(h21inv, u2, h22inv * v2) + h23inv;
        const float du1 = std::fma(-pu2, w2in1inv, u1);  // u1 - u2in1, the product never rounded
        const float dv1 = std::fma(-pv2, w2in1inv, v1);
        const float squareDist1 = std::fma(du1, du1, dv1 * dv1);
        const float chiSquare1 = squareDist1 * invSigmaSquare;
        float t1 = 0.0f, t2 = 0.0f;
        if (chiSquare1 > th)
            bIn = false;
        else {
            t1 = th - chiSquare1;
            score += t1;
        }
        // x1in2 = H21*x1
        const float w1in2inv = 1.0 / (std::fma(h31, u1, h32 * v1) + h33);
        const float pu1 = std::fma(h11, u1, h12 * v1) + h13;
        const float pv1 = std::fma(h21, u1, h22 * v1) + h23;
        const float du2 = std::fma(-pu1, w1in2inv, u2);
        const float dv2 = std::fma(-pv1, w1in2inv, v2);
        const float squareDist2 = std::fma(du2, du2, dv2 * dv2);
        const float chiSquare2 = squareDist2 * invSigmaSquare;
        if (chiSquare2 > th)
            bIn = false;
        else {
            t2 = th - chiSquare2;
            score += t2;
        }
        vbMatchesInliers[i] = bIn;
        if (terms) {
            terms[2 * i] = t1;
            terms[2 * i + 1] = t2;
        }
    }
    return score;
}

float CheckFundamental(const Model& M, const float* F21, std::vector<uint8_t>& vbMatchesInliers, float* terms) {
    const int N = (int)M.mvMatches12.size();
    const float f11 = F21[0], f12 = F21[1], f13 = F21[2], f21 = F21[3], f22 = F21[4], f23 = F21[5], f31 = F21[6],
                f32 = F21[7], f33 = F21[8];
    vbMatchesInliers.resize(N);
    float score = 0;
    const float th = 3.841;
    const float thScore = 5.991;
    const float invSigmaSquare = 1.0 / (M.sigma * M.sigma);
    for (int i = 0; i < N; i++) {
        bool bIn = true;
        const float u1 = M.k1[2 * M.mvMatches12[i].first], v1 = M.k1[2 * M.mvMatches12[i].first + 1];
        const float u2 = M.k2[2 * M.mvMatches12[i].second], v2 = M.k2[2 * M.mvMatches12[i].second + 1];
        // l2 = F21 x1 = (a2, b2, c2)
        const float a2 = std::fma(f11, u1, f12 * v1) + f13;
        const float b2 = std::fma(f21, u1, f22 * v1) + f23;
        const float c2 = std::fma(f31, u1, f32 * v1) + f33;
        const float num2 = std::fma(a2, u2, b2 * v2) + c2;
        const float squareDist1 = num2 * num2 / std::fma(a2, a2, b2 * b2);
        const float chiSquare1 = squareDist1 * invSigmaSquare;
        float t1 = 0.0f, t2 = 0.0f;
        if (chiSquare1 > th)
            bIn = false;
        else {
            t1 = thScore - chiSquare1;
            score += t1;
        }
        // l1 = x2t F21 = (a1, b1, c1)
        const float a1 = std::fma(f11, u2, f21 * v2) + f31;
        const float b1 = std::fma(f12, u2, f22 * v2) + f32;
        const float c1 = std::fma(f13, u2, f23 * v2) + f33;
        const float num1 = std::fma(a1, u1, b1 * v1) + c1;
        const float squareDist2 = num1 * num1 / std::fma(a1, a1, b1 * b1);
        const float chiSquare2 = squareDist2 * invSigmaSquare;
        if (chiSquare2 > th)
            bIn = false;
        else {
            t2 = thScore - chiSquare2;
            score += t2;
        }
        vbMatchesInliers[i] = bIn;
        if (terms) {
            terms[2 * i] = t1;
            terms[2 * i + 1] = t2;
        }
    }
    return score;
}

}  // namespace

extern "C" {

// Inputs as orb_initializer_check, keypoints as n x 2 floats.  Outputs (any may be NULL): scores
// [n_hyp], best index / score, inlier masks [n1, N written], *n_matches = N, and the accepted terms
// of every hypothesis, terms_* [n_hyp][2 * n1] with 2 N written per row (a rejected term is 0).
// Returns -22 for a matches12 entry outside [-1, n2).
int initializer_model_check(const float* kps1_xy, int n1, const float* kps2_xy, int n2, const int32_t* matches12,
                            float sigma, int n_hyp, const float* H21, const float* H12, const float* F21,
                            float* scores_h, float* scores_f, int32_t* best_h, float* best_score_h, uint8_t* inliers_h,
                            int32_t* best_f, float* best_score_f, uint8_t* inliers_f, int32_t* n_matches,
                            float* terms_h, float* terms_f) {
    Model M{kps1_xy, kps2_xy, {}, sigma};
    for (int i = 0; i < n1; i++) {  // Initializer.cc:54-63
        if (matches12[i] < -1 || matches12[i] >= n2) return -22;
        if (matches12[i] >= 0) M.mvMatches12.push_back(std::make_pair(i, matches12[i]));
    }
    const int N = (int)M.mvMatches12.size();
    if (n_matches) *n_matches = N;
    std::vector<uint8_t> vbCurrentInliers(N, 0);
    if (H21 && H12) {  // FindHomography, Initializer.cc:135-169
        float score = 0.0;
        int best = -1;
        std::vector<uint8_t> vbMatchesInliers(N, 0);
        for (int it = 0; it < n_hyp; it++) {
            const float currentScore = CheckHomography(M, H21 + 9 * it, H12 + 9 * it, vbCurrentInliers,
                                                       terms_h ? terms_h + (size_t)it * 2 * n1 : nullptr);
            if (scores_h) scores_h[it] = currentScore;
            if (currentScore > score) {
                best = it;
                vbMatchesInliers = vbCurrentInliers;
                score = currentScore;
            }
        }
        if (best_h) *best_h = best;
        if (best_score_h) *best_score_h = score;
        if (inliers_h)
            for (int i = 0; i < N; i++) inliers_h[i] = vbMatchesInliers[i];
    }
    if (F21) {  // FindFundamental, Initializer.cc:186-220
        float score = 0.0;
        int best = -1;
        std::vector<uint8_t> vbMatchesInliers(N, 0);
        for (int it = 0; it < n_hyp; it++) {
            const float currentScore =
                CheckFundamental(M, F21 + 9 * it, vbCurrentInliers, terms_f ? terms_f + (size_t)it * 2 * n1 : nullptr);
            if (scores_f) scores_f[it] = currentScore;
            if (currentScore > score) {
                best = it;
                vbMatchesInliers = vbCurrentInliers;
                score = currentScore;
            }
        }
        if (best_f) *best_f = best;
        if (best_score_f) *best_score_f = score;
        if (inliers_f)
            for (int i = 0; i < N; i++) inliers_f[i] = vbMatchesInliers[i];
    }
    return 0;
}

}  // extern "C"
