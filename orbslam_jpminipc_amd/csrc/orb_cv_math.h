// orb_cv_math.h — OpenCV 2.4's arithmetic on CV_32F 3-vectors and 3 x 3 matrices as the reference's
// cv::Mat expressions evaluate it (DESIGN.md §FP policy, §12, §16, §18, §20), shared by every unit
// that restates such an expression: orb_match.hip, orb_mappoint.hip, orb_solvers.hip,
// orb_sim3opt.hip, orb_initializer.hip, orb_localmap.hip; cv_hypot also by orb_jacobi_svd.h and
// orb_epnp_math.h.
//
// One definition of each operation.  The units that include it are built -ffp-contract=off; where a
// value is rounded to float and in what order a sum is taken is the contract, and each comment
// states it.  Only + - * /, sqrt, fabs, comparisons and conversions, all correctly rounded on the
// host and on the device: the same source compiled by a plain C++ compiler gives the same bits
// (tests/native/cv_math_host.cpp pins them against oracle/ocv_ops.cpp and numpy restatements).
#pragma once

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define ORB_CV_FN __host__ __device__ __forceinline__
#else
#define ORB_CV_FN inline __attribute__((always_inline))
#endif

namespace orb_cv {

ORB_CV_FN float cv_sqrt(float x) { return __builtin_sqrtf(x); }
ORB_CV_FN double cv_sqrt(double x) { return __builtin_sqrt(x); }
ORB_CV_FN float cv_abs(float x) { return __builtin_fabsf(x); }
ORB_CV_FN double cv_abs(double x) { return __builtin_fabs(x); }

// lapack.cpp's own hypot (found before libm's inside namespace cv), in the type of the decomposition
template <typename T>
ORB_CV_FN T cv_hypot(T a, T b) {
    a = cv_abs(a);
    b = cv_abs(b);
    if (a > b) {
        b /= a;
        return a * cv_sqrt(1 + b * b);
    }
    if (b > 0) {
        a /= b;
        return b * cv_sqrt(1 + a * a);
    }
    return 0;
}

// ---- 3-vectors ------------------------------------------------------------------------------------

// What gemm's 2 <= len <= 4 path stores for the float row sum t: (float)((double)t*alpha + (double)c*beta)
ORB_CV_FN float gemm_out(float t, double alpha, float c, double beta) {
    return (float)((double)t * alpha + (double)c * beta);
}

// alpha*A*x + beta*t, MatExpr -> gemm(A, x, alpha, t, beta), flags 0, the 2 <= len <= 4 path: the row
// sum in float, left to right, then gemm_out.  A has `stride` floats per row, t `tstride` per element.
ORB_CV_FN void gemm3_add(const float* A, int stride, const float* t, int tstride, float x0, float x1, float x2,
                         float* o, double alpha = 1.0, double beta = 1.0) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float ti = A[i * stride] * x0 + A[i * stride + 1] * x1 + A[i * stride + 2] * x2;
        o[i] = gemm_out(ti, alpha, t[i * tstride], beta);
    }
}

// A*x + t of a row-major 3 x 3 and two 3 x 1: alpha = beta = 1
ORB_CV_FN void gemm3_add(const float* A, const float* x, const float* t, float* o) {
    gemm3_add(A, 3, t, 1, x[0], x[1], x[2], o);
}

// a - b: cv::subtract, float
ORB_CV_FN void sub3(const float* a, const float* b, float* o) {
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = a[k] - b[k];
}

// cv::norm(v, NORM_L2) of a 3 x 1: normL2Sqr<float, double> (s = 0; s += (double)v_k * v_k, k ascending), sqrt
ORB_CV_FN double norm3(const float* v) {
    double s = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) s += (double)v[k] * (double)v[k];
    return cv_sqrt(s);
}

// Mat::dot of two 3 x 1: dotProd_<float> (r = 0; r += (double)a_k * b_k, k ascending)
ORB_CV_FN double dot3(const float* a, const float* b) {
    double r = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) r += (double)a[k] * (double)b[k];
    return r;
}

// MatExpr alpha*m, m/s, m *= s: convertTo -> cvtScale_<float, float, float>, scale and shift narrowed
// to float before the multiply: x * (float)alpha + (float)0
ORB_CV_FN float scale(float x, double alpha) {
    const float a = (float)alpha, shift = (float)0.0;
    return x * a + shift;
}
ORB_CV_FN void scale3(const float* x, double alpha, float* o) {
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = scale(x[k], alpha);
}

// One element of MatExpr a*alpha + b*beta: addWeighted_<float, double>(a, alpha, b, beta, 0), all in double
ORB_CV_FN float add_weighted(float a, double alpha, float b, double beta) {
    return (float)((double)a * alpha + (double)b * beta + 0.0);
}

// -R.t()*t, the camera centre: one gemm, GEMM_1_T, alpha = -1; the general path (one double
// accumulator, k ascending, then alpha)
ORB_CV_FN void camera_centre(const float* R, const float* t, float* O) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        double s0 = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) s0 += (double)R[k * 3 + i] * (double)t[k];
        O[i] = (float)(s0 * -1.0);
    }
}

// ---- 3 x 3, row-major ------------------------------------------------------------------------------

struct M3 {
    float m[9];
};

ORB_CV_FN M3 load3x3(const float* p) {
    M3 d;
#pragma unroll
    for (int k = 0; k < 9; ++k) d.m[k] = p[k];
    return d;
}

// A*B, gemm's 2 <= len <= 4 path, alpha = 1, no C: the float row sum, left to right ((float)((double)t * 1.0) is t)
ORB_CV_FN M3 mul3(const M3& a, const M3& b) {
    M3 d;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            d.m[3 * i + j] = a.m[3 * i] * b.m[j] + a.m[3 * i + 1] * b.m[3 + j] + a.m[3 * i + 2] * b.m[6 + j];
    return d;
}

// (alpha*A)*B: the short path with alpha, (float)((double)t * alpha)
ORB_CV_FN M3 mul3_alpha(const M3& a, const M3& b, double alpha) {
    M3 d = mul3(a, b);
#pragma unroll
    for (int k = 0; k < 9; ++k) d.m[k] = (float)((double)d.m[k] * alpha);
    return d;
}

// gemm with a transpose flag: not the short path but GEMMSingleMul_<float, double>, one double
// accumulator per element, k ascending, then alpha, narrowed once
template <bool TA, bool TB>
ORB_CV_FN M3 gemm3(const M3& a, const M3& b, double alpha) {
    M3 d;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double s0 = 0;
#pragma unroll
            for (int k = 0; k < 3; ++k)
                s0 += (double)(TA ? a.m[k * 3 + i] : a.m[i * 3 + k]) * (double)(TB ? b.m[j * 3 + k] : b.m[k * 3 + j]);
            d.m[i * 3 + j] = (float)(s0 * alpha);
        }
    return d;
}

// a*b - c*d of floats, in double
ORB_CV_FN double det2(float a, float b, float c, float d) { return (double)a * (double)b - (double)c * (double)d; }

// cv::determinant of a 3 x 3 CV_32F (lapack.cpp's det3): expansion along row 0, in double
ORB_CV_FN double det3(const M3& s) {
    const float* m = s.m;
    return (double)m[0] * det2(m[4], m[8], m[5], m[7]) - (double)m[1] * det2(m[3], m[8], m[5], m[6]) +
           (double)m[2] * det2(m[3], m[7], m[4], m[6]);
}

// Mat::inv() of a 3 x 3 CV_32F (DECOMP_LU's closed form): the cofactors times 1/det in double, each
// narrowed once; nine zeros when det == 0
ORB_CV_FN M3 inv3(const M3& s) {
    const float* m = s.m;
    double d = det3(s);
    M3 D;
    if (d != 0.) {
        d = 1. / d;
        D.m[0] = (float)(det2(m[4], m[8], m[5], m[7]) * d);
        D.m[1] = (float)(det2(m[2], m[7], m[1], m[8]) * d);
        D.m[2] = (float)(det2(m[1], m[5], m[2], m[4]) * d);
        D.m[3] = (float)(det2(m[5], m[6], m[3], m[8]) * d);
        D.m[4] = (float)(det2(m[0], m[8], m[2], m[6]) * d);
        D.m[5] = (float)(det2(m[2], m[3], m[0], m[5]) * d);
        D.m[6] = (float)(det2(m[3], m[7], m[4], m[6]) * d);
        D.m[7] = (float)(det2(m[1], m[6], m[0], m[7]) * d);
        D.m[8] = (float)(det2(m[0], m[4], m[1], m[3]) * d);
    } else {
#pragma unroll
        for (int k = 0; k < 9; ++k) D.m[k] = 0.0f;
    }
    return D;
}

// -M of a Mat: subtract(Scalar(0), M)
ORB_CV_FN M3 neg3x3(const M3& a) {
    M3 d;
#pragma unroll
    for (int k = 0; k < 9; ++k) d.m[k] = 0.0f - a.m[k];
    return d;
}

}  // namespace orb_cv
