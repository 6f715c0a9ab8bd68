// CPU model of orb_pnp_compute_hypotheses / orb_pnp_compute_pose_n / orb_pnp_ransac: PnPsolver::iterate
// and Refine (reference src/PnPsolver.cc:137-277) restated statement for statement, with the sampler
// on a real std::vector (it shares nothing with the closed-form mapping of the kernels) and
// CheckInliers (280-311) as DESIGN.md §12 states its arithmetic.  EPnP's compute_pose and the OpenCV
// 2.4 routines under it are csrc/orb_epnp_math.h compiled for the host with plain arrays: the one
// statement of that arithmetic.  pnp_solver_model_stages exports what every step of
// compute_pose left behind and pnp_solver_model_jacobi_svd runs the Jacobi SVD on a caller's matrix;
// tests/test_epnp_stages.py holds each to tests/epnp_reference.py, a numpy float64 EPnP written from
// the construction that shares no statement with the header.  Built -ffp-contract=off, the fused
// multiply-adds written out.  Every call can export the bitmask of the branches it visited.
// Single-threaded; scripts/pnp_solver_timing.py also times it.  -DPNP_SOLVER_MODEL_MAIN adds a main()
// for the sanitizer run.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../orbslam_jpminipc_amd/csrc/orb_epnp_math.h"

namespace {

using namespace orb_epnp;

struct PtsHost {  // pws, us, alphas, pcs of the reference (PnPsolver.cc:314-345)
    static constexpr bool STORED = true;
    int n;
    double *pws, *us, *alphas, *pcs;
    int size() const { return n; }
    double pw(int i, int j) const { return pws[3 * i + j]; }
    double u(int i, int j) const { return us[2 * i + j]; }
    double& alpha(int i, int c) { return alphas[4 * i + c]; }
    double& pc(int i, int j) { return pcs[3 * i + j]; }
};

struct Solver {
    int N = 0;
    const float *p3d = nullptr, *p2d = nullptr;
    std::vector<float> mvMaxError;
    double fu = 0, fv = 0, uc = 0, vc = 0;
    std::vector<double> pws, us, alphas, pcs;
    int number_of_correspondences = 0;
    double mRi[3][3], mti[3];
    std::vector<uint8_t> mvbInliersi;
    int mnInliersi = 0;
    unsigned br = 0;

    void reset_correspondences() {
        number_of_correspondences = 0;
        pws.clear(), us.clear();
    }
    void add_correspondence(double X, double Y, double Z, double u, double v) {
        pws.push_back(X), pws.push_back(Y), pws.push_back(Z);
        us.push_back(u), us.push_back(v);
        number_of_correspondences++;
    }
    void add_index(int idx) {
        add_correspondence(p3d[3 * idx], p3d[3 * idx + 1], p3d[3 * idx + 2], p2d[2 * idx], p2d[2 * idx + 1]);
    }
    double compute_pose(double R[3][3], double t[3]) {
        const int n = number_of_correspondences;
        alphas.assign((size_t)4 * n, 0.0);
        pcs.assign((size_t)3 * n, 0.0);
        double wk[WK_DOUBLES];
        Epnp<Mat<1>, PtsHost> e;
        e.wk = Mat<1>{wk};
        e.pt = PtsHost{n, pws.data(), us.data(), alphas.data(), pcs.data()};
        e.fu = fu, e.fv = fv, e.uc = uc, e.vc = vc;
        e.br = 0;
        const double r = orb_epnp::compute_pose(e, &R[0][0], t);
        br |= e.br;
        return r;
    }
    // compute_pose's steps in compute_pose's order, each one's result copied out (any pointer may be
    // NULL).  Only the header's functions are called; the one thing written here is the strict `<` of
    // PnPsolver.cc:478-484 on the three errors, which the caller compares with compute_pose itself.
    // br[0]: control points, barycentric coordinates and the 12 x 12; br[1..3]: find_betas_approx_N,
    // gauss_newton and compute_R_and_t of N = 1, 2, 3; br[4]: all of them with BR_N2 / BR_N3.
    void stages(double* o_cws, double* o_ci, double* o_alphas, double* o_ut, double* o_w, double* o_l, double* o_rho,
                double* o_betas0, double* o_betas, double* o_R, double* o_t, double* o_rep, int32_t* o_N,
                uint32_t* o_br) {
        const int n = number_of_correspondences;
        alphas.assign((size_t)4 * n, 0.0);
        pcs.assign((size_t)3 * n, 0.0);
        double wk[WK_DOUBLES];
        Epnp<Mat<1>, PtsHost> e;
        e.wk = Mat<1>{wk};
        e.pt = PtsHost{n, pws.data(), us.data(), alphas.data(), pcs.data()};
        e.fu = fu, e.fv = fv, e.uc = uc, e.vc = vc;
        e.br = 0;
        uint32_t brs[5] = {0, 0, 0, 0, 0};
        choose_control_points(e);
        if (o_cws) std::memcpy(o_cws, e.cws, sizeof(e.cws));
        compute_barycentric_coordinates(e);
        if (o_ci) std::memcpy(o_ci, e.ci, sizeof(e.ci));
        if (o_alphas && n) std::memcpy(o_alphas, alphas.data(), sizeof(double) * 4 * n);
        mtm_svd(e);
        if (o_ut) std::memcpy(o_ut, wk, sizeof(double) * 144);
        if (o_w) std::memcpy(o_w, wk + WK_W, sizeof(double) * 12);
        brs[0] = e.br;
        double l_6x10[6 * 10], rho[6];
        compute_L_6x10(e, l_6x10);
        compute_rho(e, rho);
        if (o_l) std::memcpy(o_l, l_6x10, sizeof(l_6x10));
        if (o_rho) std::memcpy(o_rho, rho, sizeof(rho));
        double rep[3];
        for (int k = 0; k < 3; k++) {
            double Betas[4], Rk[9], tk[3];
            e.br = 0;
            if (k == 0) find_betas_approx_1(e, l_6x10, rho, Betas);
            if (k == 1) find_betas_approx_2(e, l_6x10, rho, Betas);
            if (k == 2) find_betas_approx_3(e, l_6x10, rho, Betas);
            if (o_betas0) std::memcpy(o_betas0 + 4 * k, Betas, sizeof(Betas));
            gauss_newton(l_6x10, rho, Betas, e.br);
            if (o_betas) std::memcpy(o_betas + 4 * k, Betas, sizeof(Betas));
            rep[k] = compute_R_and_t(e, Betas, Rk, tk);
            if (o_R) std::memcpy(o_R + 9 * k, Rk, sizeof(Rk));
            if (o_t) std::memcpy(o_t + 3 * k, tk, sizeof(tk));
            if (o_rep) o_rep[k] = rep[k];
            brs[1 + k] = e.br;
        }
        int N = 1;
        if (rep[1] < rep[0]) N = 2;
        if (rep[2] < rep[N - 1]) N = 3;
        if (o_N) *o_N = N;
        brs[4] = brs[0] | brs[1] | brs[2] | brs[3] | (N == 2 ? BR_N2 : 0u) | (N == 3 ? BR_N3 : 0u);
        if (o_br) std::memcpy(o_br, brs, sizeof(brs));
        br |= brs[4];
    }
    // PnPsolver.cc:280-311 as the reference build contracts it
    void CheckInliers() {
        mnInliersi = 0;
        for (int i = 0; i < N; i++) {
            const float X = p3d[3 * i], Y = p3d[3 * i + 1], Z = p3d[3 * i + 2];
            auto row = [&](int r) {
                return std::fma(mRi[r][2], (double)Z, std::fma(mRi[r][0], (double)X, mRi[r][1] * (double)Y)) + mti[r];
            };
            float Xc = (float)row(0);
            float Yc = (float)row(1);
            float invZc = (float)(1 / row(2));
            double ue = std::fma(fu * (double)Xc, (double)invZc, uc);
            double ve = std::fma(fv * (double)Yc, (double)invZc, vc);
            float distX = (float)((double)p2d[2 * i] - ue);
            float distY = (float)((double)p2d[2 * i + 1] - ve);
            float error2 = std::fmaf(distX, distX, distY * distY);
            if (error2 < mvMaxError[i]) {
                mvbInliersi[i] = 1;
                mnInliersi++;
            } else
                mvbInliersi[i] = 0;
        }
    }
};

int RandomInt(int r, int min, int max) {  // DUtils/Random.cpp:47-50 on rand()'s value r
    int d = max - min + 1;
    return int(((double)r / ((double)2147483647 + 1.0)) * d) + min;
}

// the four draws of one iteration (PnPsolver.cc:160-173)
void draw_set(int N, const int32_t* r, int32_t* set) {
    std::vector<size_t> vAvailableIndices((size_t)N);
    for (int i = 0; i < N; i++) vAvailableIndices[i] = i;
    vAvailableIndices.reserve((size_t)N + 1);
    for (short i = 0; i < 4; ++i) {
        int randi = RandomInt(r[i] < 0 ? 0 : r[i], 0, vAvailableIndices.size() - 1);
        int idx = vAvailableIndices[randi];
        set[i] = idx;
        // [idx] may lie at or past the end: the reference writes into the vector's spare capacity
        if ((size_t)idx < vAvailableIndices.size()) vAvailableIndices[idx] = vAvailableIndices.back();
        vAvailableIndices.pop_back();
    }
}

void pack_mask(const std::vector<uint8_t>& in, int N, uint64_t* words) {
    const int W = (N + 63) / 64;
    for (int w = 0; w < W; w++) words[w] = 0;
    for (int i = 0; i < N; i++)
        if (in[i]) words[i >> 6] |= 1ull << (i & 63);
}

void to_pose(const double R[3][3], const double t[3], float* pose) {  // convertTo(CV_32F), Rcw row-major then tcw
    for (int k = 0; k < 9; k++) pose[k] = (float)R[k / 3][k % 3];
    for (int k = 0; k < 3; k++) pose[9 + k] = (float)t[k];
}

}  // namespace

extern "C" {

int pnp_solver_model_random_int(int r, int d) { return RandomInt(r, 0, d - 1); }

int pnp_solver_model_sets(int N, int n_hyp, const int32_t* rand31, int32_t* sets) {
    if (N < 4) return -22;
    for (int h = 0; h < n_hyp; h++) draw_set(N, rand31 + 4 * h, sets + 4 * h);
    return 0;
}

// the closed-form mapping of the kernels (csrc/orb_epnp_math.h minimal_set<K>), K = 3 or 4
int pnp_solver_model_mapping(int K, int N, int n_hyp, const int32_t* rand31, int32_t* sets) {
    if (N < K || (K != 3 && K != 4)) return -22;
    for (int h = 0; h < n_hyp; h++) {
        int idx[4];
        if (K == 3)
            minimal_set<3>(rand31 + 3 * h, N, idx);
        else
            minimal_set<4>(rand31 + 4 * h, N, idx);
        for (int k = 0; k < K; k++) sets[K * h + k] = idx[k];
    }
    return 0;
}

// qr_solve on a 6 x 4 (A and b are overwritten as the reference overwrites them); x as given when it
// returns early.  Returns the branch mask.
unsigned pnp_solver_model_qr_solve(double* A, double* b, double* x) {
    unsigned br = 0;
    qr_solve(A, b, x, br);
    return br;
}

// compute_pose on the n correspondences sel[0..n_sel) (or all n in order when sel is NULL) of p3d
// (n x 3 floats) / p2d (n x 2).  K = fu fv uc vc.  Returns the branch mask.
unsigned pnp_solver_model_compute_pose(int n, const float* p3d, const float* p2d, const double* K, int n_sel,
                                       const int32_t* sel, double* R, double* t, double* rep_error) {
    Solver s;
    s.N = n, s.p3d = p3d, s.p2d = p2d;
    s.fu = K[0], s.fv = K[1], s.uc = K[2], s.vc = K[3];
    s.reset_correspondences();
    for (int i = 0; i < (sel ? n_sel : n); i++) s.add_index(sel ? sel[i] : i);
    double Rm[3][3], tm[3];
    const double e = s.compute_pose(Rm, tm);
    std::memcpy(R, Rm, sizeof(Rm));
    std::memcpy(t, tm, sizeof(tm));
    if (rep_error) *rep_error = e;
    return s.br;
}

// The stages of the same call (Solver::stages): cws 4 x 3, ci 3 x 3, alphas n_used x 4, ut 12 x 12 and
// w 12 as mtm_svd left them, l_6x10 6 x 10, rho 6, then for N = 1, 2, 3 the betas after
// find_betas_approx_N (betas0, 3 x 4) and after gauss_newton (betas, 3 x 4), R (3 x 9), t (3 x 3) and the
// reprojection error (3) of compute_R_and_t; N_sel is the N the strict `<` picks, br 5 branch masks.
// Returns the whole mask, which is compute_pose's.
unsigned pnp_solver_model_stages(int n, const float* p3d, const float* p2d, const double* K, int n_sel,
                                 const int32_t* sel, double* cws, double* ci, double* alphas, double* ut, double* w,
                                 double* l_6x10, double* rho, double* betas0, double* betas, double* R, double* t,
                                 double* rep_error, int32_t* N_sel, uint32_t* br) {
    Solver s;
    s.N = n, s.p3d = p3d, s.p2d = p2d;
    s.fu = K[0], s.fv = K[1], s.uc = K[2], s.vc = K[3];
    s.reset_correspondences();
    for (int i = 0; i < (sel ? n_sel : n); i++) s.add_index(sel ? sel[i] : i);
    s.stages(cws, ci, alphas, ut, w, l_6x10, rho, betas0, betas, R, t, rep_error, N_sel, br);
    return s.br;
}

// jacobi_svd on a caller's matrix: At is n1 rows of m (overwritten: the first n become the left
// singular vectors), W n singular values, Vt n x n (written when want_vt).  Returns the branch mask.
unsigned pnp_solver_model_jacobi_svd(int m, int n, int n1, int want_vt, double* At, double* W, double* Vt) {
    unsigned br = 0;
    jacobi_svd(Mat<1>{At}, m, Mat<1>{W}, Mat<1>{Vt}, want_vt != 0, n, m, n, n1, br);
    return br;
}

// PnPsolver::iterate over n_hyp iterations (the caller's max(mRansacMaxIts - mnIterations,
// nIterations)), every iteration carried out whether or not an earlier Refine succeeded, so that every
// per-iteration array is full; first_refined is where iterate would have returned.
// Exactly one of sets / rand31 (n_hyp x 4).  Outputs (any may be NULL): counts, masks (n_hyp x W
// words), best_at, first_ok as the consensus model's; R (n_hyp x 9), t (n_hyp x 3), rep_error,
// sets_out, branches per hypothesis; refined_counts (the count of Refine at the iterations that
// replaced the best, -1 elsewhere), refined_R / refined_t (NaN elsewhere), first_refined, pose (12
// floats), pose_mask (W words), pose_inliers.  Returns -22 for bad arguments.
int pnp_solver_model_ransac(int n, const float* p3d, const float* p2d, const float* sigma2, float th2,
                            const double* K, int n_hyp, const int32_t* sets, const int32_t* rand31, int min_inliers,
                            int best_in, int32_t* counts, uint64_t* masks, int32_t* best_at, int32_t* first_ok,
                            double* R, double* t, double* rep_error, int32_t* sets_out, uint32_t* branches,
                            int32_t* refined_counts, double* refined_R, double* refined_t, int32_t* first_refined,
                            float* pose, uint64_t* pose_mask, int32_t* pose_inliers, int32_t* refine_calls) {
    if ((sets != nullptr) == (rand31 != nullptr) || min_inliers < 4 || n < 0 || n_hyp < 1) return -22;
    const int N = n, W = (N + 63) / 64;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    Solver s;
    s.N = N, s.p3d = p3d, s.p2d = p2d;
    s.fu = K[0], s.fv = K[1], s.uc = K[2], s.vc = K[3];
    s.mvMaxError.resize(N);
    for (int i = 0; i < N; i++) s.mvMaxError[i] = sigma2[i] * th2;
    s.mvbInliersi.assign(N, 0);
    const int mRansacMinInliers = min_inliers;
    int mnBestInliers = best_in, holder = best_in > 0 ? -2 : -1, fok = -1, fref = -1, ncalls = 0;
    std::vector<uint8_t> mvbBestInliers(N, 0), mvbRefinedInliers;
    float mBestTcw[12], mRefinedTcw[12];
    for (int k = 0; k < 12; k++) mBestTcw[k] = mRefinedTcw[k] = std::numeric_limits<float>::quiet_NaN();
    int mnRefinedInliers = 0;
    if (pose)
        for (int k = 0; k < 12; k++) pose[k] = std::numeric_limits<float>::quiet_NaN();
    if (pose_mask)
        for (int w = 0; w < W; w++) pose_mask[w] = 0;
    if (pose_inliers) *pose_inliers = 0;

    const bool bNoMore = N < mRansacMinInliers;  // PnPsolver.cc:145-149: nothing is generated
    for (int h = 0; h < n_hyp; h++) {
        int32_t set[4] = {0, 0, 0, 0};
        double Rz[9] = {0}, tz[3] = {0}, rep = 0;
        s.br = 0;
        if (refined_counts) refined_counts[h] = -1;
        if (refined_R)
            for (int k = 0; k < 9; k++) refined_R[9 * h + k] = nan;
        if (refined_t)
            for (int k = 0; k < 3; k++) refined_t[3 * h + k] = nan;
        if (!bNoMore) {
            if (sets) {
                for (int k = 0; k < 4; k++) {
                    if (sets[4 * h + k] < 0 || sets[4 * h + k] >= N) return -22;
                    set[k] = sets[4 * h + k];
                }
            } else
                draw_set(N, rand31 + 4 * h, set);
            s.reset_correspondences();
            for (int k = 0; k < 4; k++) s.add_index(set[k]);
            rep = s.compute_pose(s.mRi, s.mti);
            std::memcpy(Rz, s.mRi, sizeof(Rz));
            std::memcpy(tz, s.mti, sizeof(tz));
            s.CheckInliers();
        } else {
            s.mnInliersi = 0;
            s.mvbInliersi.assign(N, 0);
        }
        if (counts) counts[h] = s.mnInliersi;
        if (masks) pack_mask(s.mvbInliersi, N, masks + (size_t)h * W);
        if (R) std::memcpy(R + 9 * h, Rz, sizeof(Rz));
        if (t) std::memcpy(t + 3 * h, tz, sizeof(tz));
        if (rep_error) rep_error[h] = rep;
        if (sets_out) std::memcpy(sets_out + 4 * h, set, sizeof(set));

        if (s.mnInliersi >= mRansacMinInliers) {  // :181
            if (fok < 0) fok = h;
            bool replaced = false;
            if (s.mnInliersi > mnBestInliers) {  // :184
                mvbBestInliers = s.mvbInliersi;
                mnBestInliers = s.mnInliersi;
                to_pose(s.mRi, s.mti, mBestTcw);
                holder = h;
                replaced = true;
            }
            // Refine (:232-277) on mvbBestInliers.  When the best is still an earlier call's, its mask
            // is not known here: the call has nothing to refine (the caller's earlier call did it).
            if (holder >= 0) {
                ncalls++;
                s.reset_correspondences();
                for (int i = 0; i < N; i++)
                    if (mvbBestInliers[i]) s.add_index(i);
                s.compute_pose(s.mRi, s.mti);
                s.CheckInliers();
                mnRefinedInliers = s.mnInliersi;
                mvbRefinedInliers = s.mvbInliersi;
                if (replaced) {
                    if (refined_counts) refined_counts[h] = mnRefinedInliers;
                    if (refined_R) std::memcpy(refined_R + 9 * h, s.mRi, 72);
                    if (refined_t) std::memcpy(refined_t + 3 * h, s.mti, 24);
                } else if (refined_counts && refined_counts[holder] != mnRefinedInliers)
                    return -1;  // a repeated Refine of the same mask must repeat its result
                if (s.mnInliersi > mRansacMinInliers) {  // :264, strict
                    to_pose(s.mRi, s.mti, mRefinedTcw);
                    if (fref < 0) {
                        fref = h;
                        if (pose) std::memcpy(pose, mRefinedTcw, sizeof(mRefinedTcw));
                        if (pose_mask) pack_mask(mvbRefinedInliers, N, pose_mask);
                        if (pose_inliers) *pose_inliers = mnRefinedInliers;
                    }
                }
            }
        }
        if (branches) branches[h] = s.br;
        if (best_at) best_at[h] = holder;
    }
    if (fref < 0 && mnBestInliers >= mRansacMinInliers) {  // :213-226
        if (pose_inliers) *pose_inliers = mnBestInliers;
        if (holder >= 0) {
            if (pose) std::memcpy(pose, mBestTcw, sizeof(mBestTcw));
            if (pose_mask) pack_mask(mvbBestInliers, N, pose_mask);
        }
    }
    if (first_ok) *first_ok = fok;
    if (first_refined) *first_refined = fref;
    if (refine_calls) *refine_calls = ncalls;
    return 0;
}

}  // extern "C"

#ifdef PNP_SOLVER_MODEL_MAIN
// Stand-alone run for the sanitizers: drives the model over synthetic general sets and the
// degenerate ones (coplanar, repeated, four identical, behind the camera, NaN) and prints the union
// of the branch masks.
int main() {
    const double K[4] = {500, 500, 320, 240};
    unsigned all = 0;
    uint64_t st = 88172645463325252ull;
    auto rnd = [&]() {
        st ^= st << 13, st ^= st >> 7, st ^= st << 17;
        return (double)(st >> 11) / 9007199254740992.0;
    };
    for (int c = 0; c < 400; c++) {
        const int n = c < 300 ? 4 : 4 + c % 60;
        std::vector<float> p3(3 * n), p2(2 * n);
        for (int i = 0; i < n; i++) {
            double X = rnd() * 4 - 2, Y = rnd() * 4 - 2, Z = rnd() * 4 + (c % 7 == 0 ? -2 : 2);
            if (c % 11 == 1) Z = 3;                       // coplanar
            if (c % 13 == 2 && i) X = p3[0], Y = p3[1], Z = p3[2];  // identical
            if (c % 17 == 3 && i == 1) X = p3[0], Y = p3[1], Z = p3[2];  // repeated
            p3[3 * i] = (float)X, p3[3 * i + 1] = (float)Y, p3[3 * i + 2] = (float)Z;
            const double Zc = Z + 4;
            p2[2 * i] = (float)(K[2] + K[0] * (X + 0.3) / Zc + (c % 5 == 0 ? rnd() * 40 : 0));
            p2[2 * i + 1] = (float)(K[3] + K[1] * (Y - 0.2) / Zc + (c % 5 == 0 ? rnd() * 40 : 0));
        }
        if (c % 19 == 4) p3[1] = std::numeric_limits<float>::quiet_NaN();
        double R[9], t[3], e;
        const unsigned cb = pnp_solver_model_compute_pose(n, p3.data(), p2.data(), K, 0, nullptr, R, t, &e);
        all |= cb;
        // the same input stage by stage (its mask must be compute_pose's), with and without outputs, then
        // the Jacobi SVD alone on what the stages exported; none of these adds to `all`
        std::vector<double> al(4 * n);
        double cws[12], ci[9], ut[144], w[12], l[60], rho[6], b0[12], b[12], R3[27], t3[9], e3[3];
        int32_t N;
        uint32_t br5[5];
        const unsigned sb = pnp_solver_model_stages(n, p3.data(), p2.data(), K, 0, nullptr, cws, ci, al.data(), ut, w, l,
                                                    rho, b0, b, R3, t3, e3, &N, br5);
        const unsigned nb = pnp_solver_model_stages(n, p3.data(), p2.data(), K, 0, nullptr, nullptr, nullptr, nullptr,
                                                    nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                                    nullptr, nullptr, nullptr);
        if (sb != cb || nb != cb || sb != br5[4] || N < 1 || N > 3) {
            std::printf("stages: mask 0x%x / 0x%x against compute_pose's 0x%x, N %d\n", sb, nb, cb, (int)N);
            return 2;
        }
        double w12[12], vt12[144], a65[30], w5[5], vt5[25];
        pnp_solver_model_jacobi_svd(12, 12, 12, c & 1, ut, w12, vt12);
        for (int k = 0; k < 30; k++) a65[k] = l[k];
        pnp_solver_model_jacobi_svd(6, 5, 5, 1, a65, w5, vt5);
        pnp_solver_model_jacobi_svd(3, 3, 3, 1, ci, w5, vt5);
    }
    {  // a whole RANSAC, with the sampler on the vector
        const int n = 40, n_hyp = 50;
        std::vector<float> p3(3 * n), p2(2 * n), s2(n, 1.0f);
        std::vector<int32_t> r31(4 * n_hyp), cnt(n_hyp), bat(n_hyp), so(4 * n_hyp), rc(n_hyp);
        for (int i = 0; i < n; i++) {
            double X = rnd() * 4 - 2, Y = rnd() * 4 - 2, Z = rnd() * 4 + 2;
            p3[3 * i] = (float)X, p3[3 * i + 1] = (float)Y, p3[3 * i + 2] = (float)Z;
            p2[2 * i] = (float)(K[2] + K[0] * X / Z), p2[2 * i + 1] = (float)(K[3] + K[1] * Y / Z);
        }
        for (auto& v : r31) v = (int32_t)(rnd() * 2147483647.0);
        r31[0] = 2147483647, r31[1] = 2147483647, r31[2] = 2147483647, r31[3] = 2147483647;
        std::vector<uint64_t> m(n_hyp), pm(1);
        std::vector<double> R(9 * n_hyp), t(3 * n_hyp);
        int32_t fo, fr, pi;
        float pose[12];
        const int r = pnp_solver_model_ransac(n, p3.data(), p2.data(), s2.data(), 5.991f, K, n_hyp, nullptr, r31.data(),
                                              8, 0, cnt.data(), m.data(), bat.data(), &fo, R.data(), t.data(), nullptr,
                                              so.data(), nullptr, rc.data(), nullptr, nullptr, &fr, pose, pm.data(), &pi,
                                              nullptr);
        std::printf("ransac: status %d first_ok %d first_refined %d inliers %d\n", r, fo, fr, pi);
        if (r) return 1;
    }
    std::printf("pnp solver model: branches 0x%x of 0x%x\n", all, (unsigned)BR_ALL);
    return 0;
}
#endif
