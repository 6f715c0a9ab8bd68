// orb_jacobi_svd.h — OpenCV 2.4's JacobiSVDImpl_<float> as read, on one lane's
// column of LDS.  Device code shared by orb_initializer.hip (ComputeH21 / ComputeF21, DecomposeE,
// ReconstructH, Triangulate) and orb_localmap.hip (CreateNewMapPoints' triangulation): one text, so
// the two units cannot drift apart.  The scalar arithmetic (hypot, addWeighted) is csrc/orb_cv_math.h's.
#pragma once
#include <hip/hip_runtime.h>

#include "orb_cv_math.h"

constexpr int HY_MAX_FILL_TRIES = 16;                       // OpenCV's fill-in `while` has no bound; §16

// JacobiSVDImpl_<float> on the lane's column of LDS: A = At, N rows of M (N1 rows when the rows
// past N are filled in), V = Vt (N x N) when HASV, W = N doubles.  Element e of a region is at
// [e * 64].  N1 == 0 leaves the rows of At as the sort left them (ComputeH21 reads only Vt).
template <int M, int N, int N1, bool HASV>
__device__ void hy_jacobi(float* A, float* V, double* W) {
    const float eps = 1.1920928955078125e-7f * 10;  // FLT_EPSILON * 10
    const double minval = 1.17549435082228750797e-38;  // FLT_MIN
#pragma unroll 1
    for (int i = 0; i < N; ++i) {
        double sd = 0;
        for (int k = 0; k < M; ++k) {
            const float t = A[(i * M + k) * 64];
            sd += (double)t * t;
        }
        W[i * 64] = sd;
        if (HASV)
            for (int k = 0; k < N; ++k) V[(i * N + k) * 64] = k == i ? 1.0f : 0.0f;
    }
#pragma unroll 1
    for (int iter = 0; iter < 30; ++iter) {  // max(m, 30) with m <= 16
        bool changed = false;
#pragma unroll 1
        for (int i = 0; i < N - 1; ++i)
#pragma unroll 1
            for (int j = i + 1; j < N; ++j) {
                float* Ai = A + i * M * 64;
                float* Aj = A + j * M * 64;
                double a = W[i * 64], p = 0, b = W[j * 64];
                for (int k = 0; k < M; ++k) p += (double)Ai[k * 64] * (double)Aj[k * 64];
                if (fabs(p) <= (double)eps * __builtin_sqrt(a * b)) continue;
                p *= 2;
                const double beta = a - b, gamma = orb_cv::cv_hypot(p, beta);
                float c, s;
                if (beta < 0) {
                    const double delta = (gamma - beta) * 0.5;
                    s = (float)__builtin_sqrt(delta / gamma);
                    c = (float)(p / (gamma * (double)s * 2));
                } else {
                    c = (float)__builtin_sqrt((gamma + beta) / (gamma * 2));
                    s = (float)(p / (gamma * (double)c * 2));
                }
                a = b = 0;
                for (int k = 0; k < M; ++k) {
                    const float x = Ai[k * 64], y = Aj[k * 64];
                    const float t0 = c * x + s * y;
                    const float t1 = -s * x + c * y;
                    Ai[k * 64] = t0;
                    Aj[k * 64] = t1;
                    a += (double)t0 * t0;
                    b += (double)t1 * t1;
                }
                W[i * 64] = a;
                W[j * 64] = b;
                changed = true;
                if (HASV) {
                    float* Vi = V + i * N * 64;
                    float* Vj = V + j * N * 64;
                    for (int k = 0; k < N; ++k) {
                        const float x = Vi[k * 64], y = Vj[k * 64];
                        Vi[k * 64] = c * x + s * y;
                        Vj[k * 64] = -s * x + c * y;
                    }
                }
            }
        if (!changed) break;
    }
#pragma unroll 1
    for (int i = 0; i < N; ++i) {
        double sd = 0;
        for (int k = 0; k < M; ++k) {
            const float t = A[(i * M + k) * 64];
            sd += (double)t * t;
        }
        W[i * 64] = __builtin_sqrt(sd);
    }
    // descending selection sort, the first of equal values wins; rows of At and Vt follow
#pragma unroll 1
    for (int i = 0; i < N - 1; ++i) {
        int j = i;
        for (int k = i + 1; k < N; ++k)
            if (W[j * 64] < W[k * 64]) j = k;
        if (i != j) {
            const double t = W[i * 64];
            W[i * 64] = W[j * 64];
            W[j * 64] = t;
            for (int k = 0; k < M; ++k) {
                const float x = A[(i * M + k) * 64];
                A[(i * M + k) * 64] = A[(j * M + k) * 64];
                A[(j * M + k) * 64] = x;
            }
            if (HASV)
                for (int k = 0; k < N; ++k) {
                    const float x = V[(i * N + k) * 64];
                    V[(i * N + k) * 64] = V[(j * N + k) * 64];
                    V[(j * N + k) * 64] = x;
                }
        }
    }
    if (N1 == 0) return;
    unsigned long long state = 0x12345678ull;  // RNG rng(0x12345678), seeded per call
#pragma unroll 1
    for (int i = 0; i < N1; ++i) {
        float* Ai = A + i * M * 64;
        double sd = i < N ? W[i * 64] : 0;
        int tries = 0;
        while (sd <= minval && tries++ < HY_MAX_FILL_TRIES) {
            const float val0 = (float)(1. / M);
            for (int k = 0; k < M; ++k) {
                state = (unsigned long long)(unsigned)state * 4164903690u + (unsigned)(state >> 32);
                Ai[k * 64] = ((unsigned)state & 256u) != 0 ? val0 : -val0;
            }
#pragma unroll 1
            for (int it = 0; it < 2; ++it)
#pragma unroll 1
                for (int j = 0; j < i; ++j) {
                    const float* Aj = A + j * M * 64;
                    sd = 0;
                    for (int k = 0; k < M; ++k) sd += (double)(Ai[k * 64] * Aj[k * 64]);
                    float asum = 0;
                    for (int k = 0; k < M; ++k) {
                        const float t = (float)((double)Ai[k * 64] - sd * (double)Aj[k * 64]);
                        Ai[k * 64] = t;
                        asum += fabsf(t);
                    }
                    asum = asum != 0.0f ? 1.0f / asum : 0.0f;  // (a NaN sum is "true": 1/NaN)
                    for (int k = 0; k < M; ++k) Ai[k * 64] *= asum;
                }
            sd = 0;
            for (int k = 0; k < M; ++k) {
                const float t = Ai[k * 64];
                sd += (double)t * t;
            }
            sd = __builtin_sqrt(sd);
        }
        const float s = (float)(1 / sd);
        for (int k = 0; k < M; ++k) Ai[k * 64] *= s;
    }
}

// ---- Triangulate (Initializer.cc:734-751, LocalMapping.cc:304-320) ---------------------------------
// The lane's column of a wave's TRI_WAVE_BYTES of LDS: At and Vt (4 x 4 floats each), then W (4
// doubles), element e of a region at [e * 64].
constexpr int TRI_WAVE_BYTES = 32 * 64 * 4 + 4 * 64 * 8;
struct TriColumn {
    float *At, *Vt;
    double* W;
    __device__ __forceinline__ TriColumn(uint8_t* wave_base, int lane)
        : At((float*)wave_base + lane), Vt(At + 16 * 64), W((double*)(wave_base + 32 * 64 * 4) + lane) {}
};

// A.row(r) = xs[r]*P.row(2) - P.row(r & 1) with P = Pa for r < 2 and Pb after (row-major 3 x 4), each
// element one addWeighted; the SVD of A on the column (the work matrix is the transpose); vr = vt.row(3)
__device__ __forceinline__ void triangulate_vt3(const float* Pa, const float* Pb, const float* xs, const TriColumn& c,
                                                float* vr) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float* P = r < 2 ? Pa : Pb;
            c.At[(j * 4 + r) * 64] = orb_cv::add_weighted(P[8 + j], (double)xs[r], P[(r & 1) * 4 + j], -1.0);
        }
    hy_jacobi<4, 4, 0, true>(c.At, c.Vt, c.W);
#pragma unroll
    for (int k = 0; k < 4; ++k) vr[k] = c.Vt[(12 + k) * 64];
}
