// g2o_math_host.cpp — csrc/orb_g2o_math.h compiled as plain C++ (build/libg2o_math_host.so).
//
// The functions of that header marked ORB_G2O_FN use only correctly rounded operations, so what a
// host compiler makes of them (-ffp-contract=off, as the library) gives the bits the kernels give.
// tests/test_g2o_math_host.py compares them byte for byte with the CPU models, which restate the
// same g2o / Eigen pieces independently (run-time indices, no template).  The LDLT cases live here,
// so that the test and the stand-alone sanitizer run (-DG2O_MATH_HOST_MAIN) solve the same systems.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../orbslam_jpminipc_amd/csrc/orb_g2o_math.h"

namespace {

constexpr int N_FIXED = 7;     // the hand-made systems of ldlt_case
constexpr int N_RANDOM = 200;  // J^T J + lambda I

// uniform in [-1, 1), a 64-bit LCG's top 53 bits
double next_unit(uint64_t& s) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(s >> 11) * (1.0 / 4503599627370496.0) - 1.0;
}

void set_sym(double* H, int N, int i, int j, double v) { H[N * i + j] = H[N * j + i] = v; }

// H = diag(d) with small, all different off-diagonal entries: the pivot order is that of d
void diag_plus(double* H, int N, const double* d, double off) {
    for (int i = 0; i < N; ++i)
        for (int j = i; j < N; ++j) set_sym(H, N, i, j, i == j ? d[i] : off * (1 + i + 2 * j));
}

template <int N>
int solve(const double* H, const double* b, double lambda, double* x) {
    double tri[N * (N + 1) / 2], A[N * N];
    int c = 0;
    for (int j = 0; j < N; ++j)
        for (int k = j; k < N; ++k) tri[c++] = H[N * j + k];
    lm_damped<N>(tri, lambda, A);
    return ldlt<N>(A, b, x) ? 1 : 0;
}

}  // namespace

extern "C" {

int g2o_ldlt_case_count() { return N_FIXED + N_RANDOM; }

// System `idx` for N = 6 or 7: H (N x N, symmetric), b (N) and the damping; 0 when there is none.
int g2o_ldlt_case(int N, int idx, double* H, double* b, double* lambda) {
    if ((N != 6 && N != 7) || idx < 0 || idx >= N_FIXED + N_RANDOM) return 0;
    std::memset(H, 0, sizeof(double) * N * N);
    for (int i = 0; i < N; ++i) b[i] = 0.5 * (i + 1) * (i % 2 ? -1 : 1);
    *lambda = 0.0;
    double d[7];
    switch (idx) {
    case 0:  // the largest remaining diagonal is last at every step: N-1, N-2, ..., 1, N
        for (int i = 0; i < N; ++i) d[i] = i == N - 1 ? N : N - 1 - i;
        diag_plus(H, N, d, 1e-3);
        return 1;
    case 1:  // two equal largest diagonals, at 1 and 3
        for (int i = 0; i < N; ++i) d[i] = i == 1 || i == 3 ? 3 : 1 + 0.125 * i;
        diag_plus(H, N, d, 1e-3);
        return 1;
    case 2: {  // v v' for v = (2, 1, 1) under larger pivots: two exact zero pivots after elimination
        const double v[3] = {2, 1, 1};
        for (int i = 0; i < N - 3; ++i) H[(N + 1) * i] = 8 + i;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) H[N * (N - 3 + i) + (N - 3 + j)] = v[i] * v[j];
        return 1;
    }
    case 3:  // negative definite
        for (int i = 0; i < N; ++i) d[i] = -(2.0 + i);
        diag_plus(H, N, d, 1e-3);
        return 1;
    case 4:  // indefinite: the negative diagonal is met after positive ones
        for (int i = 0; i < N; ++i) d[i] = i == 2 ? -1 : 2.0 + i;
        diag_plus(H, N, d, 1e-3);
        return 1;
    case 5:  // all zero: sign 0, accepted
        return 1;
    case 6:  // indefinite with the largest |a_ii| negative: the first pivot is the negative one
        for (int i = 0; i < N; ++i) d[i] = i == 4 ? -9 : 1.0 + i;
        diag_plus(H, N, d, 1e-3);
        return 1;
    default: {
        const int r = idx - N_FIXED;
        uint64_t s = 0x9E3779B97F4A7C15ull * (uint64_t)(r + 1) + (uint64_t)N;
        const int M = 10;
        double J[10 * 7];
        for (int k = 0; k < M * N; ++k) J[k] = next_unit(s);
        for (int i = 0; i < N; ++i) {
            for (int j = i; j < N; ++j) {
                double a = 0;
                for (int m = 0; m < M; ++m) a += J[N * m + i] * J[N * m + j];
                set_sym(H, N, i, j, a);
            }
            b[i] = next_unit(s);
        }
        const double lambdas[3] = {0.0, 1e-8, 1.0};
        *lambda = lambdas[r % 3];
        return 1;
    }
    }
}

// ldlt<N> of lm_damped<N>(upper triangle of H, lambda): 1 solved, 0 refused (x untouched), -1 bad N
int g2o_solve(int N, const double* H, const double* b, double lambda, double* x) {
    return N == 6 ? solve<6>(H, b, lambda, x) : N == 7 ? solve<7>(H, b, lambda, x) : -1;
}
void g2o_quat_from_matrix(const double* m9, double* q4) { quat_from_matrix(m9, q4); }
void g2o_matrix_from_quat(const double* q4, double* R9) { matrix_from_quat(q4, R9); }
void g2o_rotate(const double* q4, const double* v3, double* o3) { rotate(q4, v3, o3); }
void g2o_quat_mul(const double* a4, const double* b4, double* o4) { quat_mul(a4, b4, o4); }
void g2o_huber(double e, double delta, double* rho2) { huber(e, delta, delta * delta, &rho2[0], &rho2[1]); }

}  // extern "C"

#ifdef G2O_MATH_HOST_MAIN
// Stand-alone run for the sanitizers: every LDLT case at both dimensions.
int main() {
    int solved = 0, refused = 0;
    for (int N = 6; N <= 7; ++N)
        for (int idx = 0; idx < g2o_ldlt_case_count(); ++idx) {
            double H[49], b[7], lambda, x[7];
            if (!g2o_ldlt_case(N, idx, H, b, &lambda)) return 1;
            for (int k = 0; k < 7; ++k) x[k] = -777.0;
            const int ok = g2o_solve(N, H, b, lambda, x);
            if (ok < 0) return 1;
            if (!ok)
                for (int k = 0; k < N; ++k)
                    if (x[k] != -777.0) return 2;  // a refusal leaves x alone
            if (x[6] != -777.0 && N == 6) return 3;
            ok ? ++solved : ++refused;
        }
    std::printf("g2o_math_host: %d solved, %d refused\n", solved, refused);
    return refused == 6 ? 0 : 4;  // cases 3, 4 and 6 at both dimensions
}
#endif
