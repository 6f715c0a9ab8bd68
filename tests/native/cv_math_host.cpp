// cv_math_host.cpp — csrc/orb_cv_math.h compiled as plain C++ (build/libcv_math_host.so).
//
// The header uses only correctly rounded operations, so what a host compiler makes of it
// (-ffp-contract=off, as the library) gives the bits the kernels give.  tests/test_cv_math_host.py
// compares every function byte for byte with oracle/ocv_ops.cpp (linked in here and exported as
// ocv_*) or with numpy scalar restatements.  The same source is a program for the sanitizers
// (-DCV_MATH_HOST_MAIN): every function on heap buffers of exactly the sizes it may touch.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../oracle/ocv_ops.h"
#include "../../orbslam_jpminipc_amd/csrc/orb_cv_math.h"

using orb_cv::M3;

extern "C" {

void cvm_gemm3_add(const float* A, const float* x, const float* t, float* o) { orb_cv::gemm3_add(A, x, t, o); }
// the strided form: A with `stride` floats per row, t with `tstride`, explicit alpha / beta
void cvm_gemm3_add_strided(const float* A, int stride, const float* t, int tstride, const float* x, double alpha,
                           double beta, float* o) {
    orb_cv::gemm3_add(A, stride, t, tstride, x[0], x[1], x[2], o, alpha, beta);
}
float cvm_gemm_out(float t, double alpha, float c, double beta) { return orb_cv::gemm_out(t, alpha, c, beta); }
void cvm_sub3(const float* a, const float* b, float* o) { orb_cv::sub3(a, b, o); }
double cvm_norm3(const float* v) { return orb_cv::norm3(v); }
double cvm_dot3(const float* a, const float* b) { return orb_cv::dot3(a, b); }
float cvm_scale(float x, double alpha) { return orb_cv::scale(x, alpha); }
void cvm_scale3(const float* x, double alpha, float* o) { orb_cv::scale3(x, alpha, o); }
float cvm_add_weighted(float a, double alpha, float b, double beta) { return orb_cv::add_weighted(a, alpha, b, beta); }
void cvm_camera_centre(const float* R, const float* t, float* O) { orb_cv::camera_centre(R, t, O); }
void cvm_mul3(const float* a, const float* b, float* o) {
    const M3 d = orb_cv::mul3(orb_cv::load3x3(a), orb_cv::load3x3(b));
    std::memcpy(o, d.m, sizeof d.m);
}
void cvm_mul3_alpha(const float* a, const float* b, double alpha, float* o) {
    const M3 d = orb_cv::mul3_alpha(orb_cv::load3x3(a), orb_cv::load3x3(b), alpha);
    std::memcpy(o, d.m, sizeof d.m);
}
void cvm_gemm3(int ta, int tb, const float* a, const float* b, double alpha, float* o) {
    const M3 A = orb_cv::load3x3(a), B = orb_cv::load3x3(b);
    const M3 d = ta ? (tb ? orb_cv::gemm3<true, true>(A, B, alpha) : orb_cv::gemm3<true, false>(A, B, alpha))
                    : (tb ? orb_cv::gemm3<false, true>(A, B, alpha) : orb_cv::gemm3<false, false>(A, B, alpha));
    std::memcpy(o, d.m, sizeof d.m);
}
double cvm_det3(const float* a) { return orb_cv::det3(orb_cv::load3x3(a)); }
void cvm_inv3(const float* a, float* o) {
    const M3 d = orb_cv::inv3(orb_cv::load3x3(a));
    std::memcpy(o, d.m, sizeof d.m);
}
void cvm_neg3x3(const float* a, float* o) {
    const M3 d = orb_cv::neg3x3(orb_cv::load3x3(a));
    std::memcpy(o, d.m, sizeof d.m);
}
float cvm_hypot_f(float a, float b) { return orb_cv::cv_hypot(a, b); }
double cvm_hypot_d(double a, double b) { return orb_cv::cv_hypot(a, b); }

// oracle/ocv_ops.cpp, the independent statement of four of them
void ocv_gemm3_add(const float* A, const float* x, const float* t, float* o) { ocv::gemm3_add(A, x, t, o); }
void ocv_sub3(const float* a, const float* b, float* o) { ocv::sub3(a, b, o); }
double ocv_norm3(const float* v) { return ocv::norm3(v); }
double ocv_dot3(const float* a, const float* b) { return ocv::dot3(a, b); }

}  // extern "C"

#ifdef CV_MATH_HOST_MAIN
namespace {

// uniform in [-4, 4), a 64-bit LCG's top 24 bits
float next_f(uint64_t& s) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (float)(s >> 40) * (8.0f / 16777216.0f) - 4.0f;
}

// `n` floats on the heap, exactly: a read or write past them is the sanitizer's to report
std::vector<float> rnd(uint64_t& s, int n) {
    std::vector<float> v(n);
    for (float& e : v) e = next_f(s);
    return v;
}

bool same(const void* a, const void* b, size_t n) { return std::memcmp(a, b, n) == 0; }

}  // namespace

// Stand-alone run for the sanitizers: every function, the four that oracle/ocv_ops.cpp states compared
// with it on the way.
int main() {
    uint64_t s = 0x9E3779B97F4A7C15ull;
    int status = 0, cases = 0;
    double sink = 0;
    for (int it = 0; it < 300; ++it, ++cases) {
        const std::vector<float> A = rnd(s, 9), B = rnd(s, 9), x = rnd(s, 3), t = rnd(s, 3);
        const std::vector<float> A4 = rnd(s, 11), t4 = rnd(s, 9);  // stride 4: the last row ends at [10], t at [8]
        std::vector<float> o3(3), r3(3), o9(9);
        cvm_gemm3_add(A.data(), x.data(), t.data(), o3.data());
        ocv_gemm3_add(A.data(), x.data(), t.data(), r3.data());
        if (!same(o3.data(), r3.data(), 12)) status = 1;
        cvm_sub3(x.data(), t.data(), o3.data());
        ocv_sub3(x.data(), t.data(), r3.data());
        if (!same(o3.data(), r3.data(), 12)) status = 2;
        const double n = cvm_norm3(x.data()), nr = ocv_norm3(x.data());
        if (!same(&n, &nr, 8)) status = 3;
        const double d = cvm_dot3(x.data(), t.data()), dr = ocv_dot3(x.data(), t.data());
        if (!same(&d, &dr, 8)) status = 4;
        cvm_gemm3_add_strided(A4.data(), 4, t4.data(), 4, x.data(), -(double)x[0], 1.0, o3.data());
        cvm_scale3(x.data(), 1. / n, o3.data());
        cvm_camera_centre(A.data(), t.data(), o3.data());
        cvm_mul3(A.data(), B.data(), o9.data());
        cvm_mul3_alpha(A.data(), B.data(), (double)t[0], o9.data());
        for (int f = 0; f < 4; ++f) cvm_gemm3(f >> 1, f & 1, A.data(), B.data(), f & 1 ? -1.0 : 1.0, o9.data());
        cvm_inv3(A.data(), o9.data());
        cvm_neg3x3(A.data(), o9.data());
        sink += cvm_det3(A.data()) + o9[8] + o3[2] + cvm_scale(x[0], 0.1) + cvm_add_weighted(x[0], n, x[1], -1.0) +
                cvm_gemm_out(x[0], 1.0, x[1], 1.0) + cvm_hypot_f(x[0], x[1]) + cvm_hypot_d(n, d);
    }
    const float z[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    std::vector<float> o9(9, 1.0f);
    cvm_inv3(z, o9.data());
    for (float e : o9)
        if (e != 0.0f) status = 5;
    if (cvm_hypot_f(0.0f, 0.0f) != 0.0f || cvm_hypot_d(0.0, 0.0) != 0.0) status = 6;
    if (cvm_scale(0.0f, 1. / 0.) == cvm_scale(0.0f, 1. / 0.)) status = 7;  // 0 * inf: NaN
    std::printf("cv_math_host: %d cases, status %d (%g)\n", cases, status, sink != sink ? 0.0 : 1.0);
    return status;
}
#endif
