// CPU model of orb_initializer_compute_hypotheses: everything of Initializer::Initialize (reference
// src/Initializer.cc:44-221) that comes before CheckHomography / CheckFundamental: mvMatches12, the
// minimal sets (80-95), Normalize (747-793), ComputeH21 / ComputeF21 (224-301) and the
// T2inv*Hn*T1, H21i.inv(), T2t*Fn*T1 products, restated statement for statement, with the OpenCV 2.4
// routines they call (modules/core/src/lapack.cpp: _SVDcompute, JacobiSVDImpl_<float>, its own
// hypot, invert's 3x3 closed form; matmul.cpp: gemm's 2 <= len <= 4 path) restated as read.  No
// OpenCV 2.4 source or binary is at hand: parity with a real build is unpinned.
// Built -ffp-contract=off (a distro OpenCV 2.4 has no FMA; the reference's own statements here offer
// no contraction, §16).  Shares nothing with csrc/orb_initializer.hip.  The scoring that follows is
// tests/native/initializer_model.cpp.  Single-threaded; scripts/initializer_ransac_timing.py also
// times it.  -DINITIALIZER_RANSAC_MODEL_MAIN adds a main() for the sanitizer run.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

namespace {

// ---- OpenCV 2.4, as read -----------------------------------------------------------------------

// lapack.cpp's own hypot: unqualified lookup inside namespace cv finds it before libm's
template <typename _Tp>
inline _Tp cv_hypot(_Tp a, _Tp b) {
    a = std::abs(a);
    b = std::abs(b);
    if (a > b) {
        b /= a;
        return a * std::sqrt(1 + b * b);
    }
    if (b > 0) {
        a /= b;
        return b * std::sqrt(1 + a * a);
    }
    return 0;
}

struct RNG {  // cv::RNG::next
    uint64_t state;
    explicit RNG(uint64_t s) : state(s) {}
    unsigned next() {
        state = (uint64_t)(unsigned)state * 4164903690U + (unsigned)(state >> 32);
        return (unsigned)state;
    }
};

// The fill-in `while` has no bound in OpenCV; the model and the kernel give up after this many
// draws of a random row and leave the row as the last try made it.
const int MAX_FILL_TRIES = 16;

// JacobiSVDImpl_<float>(At, astep, _W, Vt, vstep, m, n, n1, minval = FLT_MIN, eps = FLT_EPSILON*10).
// At: n1 rows of m (stride astep floats), the first n orthogonalised; Vt: n x n or NULL.
// `signs`, when given, receives the sign of every value the generator hands out (+1 / -1).
void JacobiSVDImpl(float* At, int astep, float* _W, float* Vt, int vstep, int m, int n, int n1,
                   std::vector<int>* signs = nullptr) {
    const double minval = FLT_MIN;
    const float eps = FLT_EPSILON * 10;
    std::vector<double> Wbuf(n);
    double* W = Wbuf.data();
    int i, j, k, iter, max_iter = std::max(m, 30);
    float c, s;
    double sd;

    for (i = 0; i < n; i++) {
        for (k = 0, sd = 0; k < m; k++) {
            float t = At[i * astep + k];
            sd += (double)t * t;
        }
        W[i] = sd;
        if (Vt) {
            for (k = 0; k < n; k++) Vt[i * vstep + k] = 0;
            Vt[i * vstep + i] = 1;
        }
    }

    for (iter = 0; iter < max_iter; iter++) {
        bool changed = false;
        for (i = 0; i < n - 1; i++)
            for (j = i + 1; j < n; j++) {
                float *Ai = At + i * astep, *Aj = At + j * astep;
                double a = W[i], p = 0, b = W[j];
                for (k = 0; k < m; k++) p += (double)Ai[k] * Aj[k];
                if (std::abs(p) <= eps * std::sqrt((double)a * b)) continue;
                p *= 2;
                double beta = a - b, gamma = cv_hypot((double)p, beta);
                if (beta < 0) {
                    double delta = (gamma - beta) * 0.5;
                    s = (float)std::sqrt(delta / gamma);
                    c = (float)(p / (gamma * s * 2));
                } else {
                    c = (float)std::sqrt((gamma + beta) / (gamma * 2));
                    s = (float)(p / (gamma * c * 2));
                }
                a = b = 0;
                for (k = 0; k < m; k++) {
                    float t0 = c * Ai[k] + s * Aj[k];
                    float t1 = -s * Ai[k] + c * Aj[k];
                    Ai[k] = t0;
                    Aj[k] = t1;
                    a += (double)t0 * t0;
                    b += (double)t1 * t1;
                }
                W[i] = a;
                W[j] = b;
                changed = true;
                if (Vt) {
                    float *Vi = Vt + i * vstep, *Vj = Vt + j * vstep;
                    for (k = 0; k < n; k++) {
                        float t0 = c * Vi[k] + s * Vj[k];
                        float t1 = -s * Vi[k] + c * Vj[k];
                        Vi[k] = t0;
                        Vj[k] = t1;
                    }
                }
            }
        if (!changed) break;
    }

    for (i = 0; i < n; i++) {
        for (k = 0, sd = 0; k < m; k++) {
            float t = At[i * astep + k];
            sd += (double)t * t;
        }
        W[i] = std::sqrt(sd);
    }

    for (i = 0; i < n - 1; i++) {
        j = i;
        for (k = i + 1; k < n; k++)
            if (W[j] < W[k]) j = k;
        if (i != j) {
            std::swap(W[i], W[j]);
            if (Vt) {
                for (k = 0; k < m; k++) std::swap(At[i * astep + k], At[j * astep + k]);
                for (k = 0; k < n; k++) std::swap(Vt[i * vstep + k], Vt[j * vstep + k]);
            }
        }
    }

    for (i = 0; i < n; i++) _W[i] = (float)W[i];
    if (!Vt) return;

    RNG rng(0x12345678);
    for (i = 0; i < n1; i++) {
        sd = i < n ? W[i] : 0;
        int tries = 0;
        while (sd <= minval && tries++ < MAX_FILL_TRIES) {
            // a zero singular value: a random vector, its projections on the earlier rows taken
            // off twice, normalised
            const float val0 = (float)(1. / m);
            for (k = 0; k < m; k++) {
                float val = (rng.next() & 256) != 0 ? val0 : -val0;
                if (signs) signs->push_back(val > 0 ? 1 : -1);
                At[i * astep + k] = val;
            }
            for (iter = 0; iter < 2; iter++)
                for (j = 0; j < i; j++) {
                    sd = 0;
                    for (k = 0; k < m; k++) sd += At[i * astep + k] * At[j * astep + k];
                    float asum = 0;
                    for (k = 0; k < m; k++) {
                        float t = (float)(At[i * astep + k] - sd * At[j * astep + k]);
                        At[i * astep + k] = t;
                        asum += std::abs(t);
                    }
                    asum = asum ? 1 / asum : 0;
                    for (k = 0; k < m; k++) At[i * astep + k] *= asum;
                }
            sd = 0;
            for (k = 0; k < m; k++) {
                float t = At[i * astep + k];
                sd += (double)t * t;
            }
            sd = std::sqrt(sd);
        }
        s = (float)(1 / sd);
        for (k = 0; k < m; k++) At[i * astep + k] *= s;
    }
}

// cv::SVDecomp(A, w, u, vt, MODIFY_A | FULL_UV) on a rows x cols CV_32F (_SVDcompute): w (min
// floats), u (rows x rows) and vt (cols x cols), row-major.  u is filled only when asked for.
void SVDecomp(const float* A, int rows, int cols, float* w, float* u, float* vt, std::vector<int>* signs = nullptr) {
    int m = rows, n = cols;
    bool at = false;
    if (m < n) {
        std::swap(m, n);
        at = true;
    }
    const int urows = m;  // FULL_UV
    std::vector<float> temp_u((size_t)urows * m, 0.0f), temp_v((size_t)n * n);  // temp_a = its first n rows
    if (!at) {
        for (int r = 0; r < rows; r++)
            for (int c = 0; c < cols; c++) temp_u[(size_t)c * m + r] = A[r * cols + c];  // transpose(src, temp_a)
    } else {
        for (int r = 0; r < rows; r++)
            for (int c = 0; c < cols; c++) temp_u[(size_t)r * m + c] = A[r * cols + c];  // src.copyTo(temp_a)
    }
    JacobiSVDImpl(temp_u.data(), m, w, temp_v.data(), n, m, n, urows, signs);
    if (!at) {
        if (u)
            for (int r = 0; r < m; r++)
                for (int c = 0; c < m; c++) u[r * m + c] = temp_u[(size_t)c * m + r];  // transpose(temp_u, _u)
        std::memcpy(vt, temp_v.data(), sizeof(float) * n * n);
    } else {
        if (u)
            for (int r = 0; r < n; r++)
                for (int c = 0; c < n; c++) u[r * n + c] = temp_v[(size_t)c * n + r];  // transpose(temp_v, _u)
        std::memcpy(vt, temp_u.data(), sizeof(float) * m * m);
    }
}

// A * B, 3x3 CV_32F: gemm's 2 <= len <= 4 path with alpha = 1 and no C (oracle/ocv_ops.h states it)
void mul3(const float* a, const float* b, float* d) {
    float out[9];
    for (int i = 0; i < 3; i++, a += 3) {
        float t0 = a[0] * b[0] + a[1] * b[3] + a[2] * b[6];
        float t1 = a[0] * b[1] + a[1] * b[4] + a[2] * b[7];
        float t2 = a[0] * b[2] + a[1] * b[5] + a[2] * b[8];
        out[3 * i + 0] = (float)((double)t0 * 1.0);
        out[3 * i + 1] = (float)((double)t1 * 1.0);
        out[3 * i + 2] = (float)((double)t2 * 1.0);
    }
    std::memcpy(d, out, sizeof(out));
}

// Mat::inv() of a 3x3 CV_32F (invert, DECOMP_LU, n == 3)
#define Sf(y, x) S[(y)*3 + (x)]
void inv3(const float* S, float* D) {
    double d = Sf(0, 0) * ((double)Sf(1, 1) * Sf(2, 2) - (double)Sf(1, 2) * Sf(2, 1)) -
               Sf(0, 1) * ((double)Sf(1, 0) * Sf(2, 2) - (double)Sf(1, 2) * Sf(2, 0)) +
               Sf(0, 2) * ((double)Sf(1, 0) * Sf(2, 1) - (double)Sf(1, 1) * Sf(2, 0));  // det3
    if (d != 0.) {
        float t[9];
        d = 1. / d;
        t[0] = (float)(((double)Sf(1, 1) * Sf(2, 2) - (double)Sf(1, 2) * Sf(2, 1)) * d);
        t[1] = (float)(((double)Sf(0, 2) * Sf(2, 1) - (double)Sf(0, 1) * Sf(2, 2)) * d);
        t[2] = (float)(((double)Sf(0, 1) * Sf(1, 2) - (double)Sf(0, 2) * Sf(1, 1)) * d);
        t[3] = (float)(((double)Sf(1, 2) * Sf(2, 0) - (double)Sf(1, 0) * Sf(2, 2)) * d);
        t[4] = (float)(((double)Sf(0, 0) * Sf(2, 2) - (double)Sf(0, 2) * Sf(2, 0)) * d);
        t[5] = (float)(((double)Sf(0, 2) * Sf(1, 0) - (double)Sf(0, 0) * Sf(1, 2)) * d);
        t[6] = (float)(((double)Sf(1, 0) * Sf(2, 1) - (double)Sf(1, 1) * Sf(2, 0)) * d);
        t[7] = (float)(((double)Sf(0, 1) * Sf(2, 0) - (double)Sf(0, 0) * Sf(2, 1)) * d);
        t[8] = (float)(((double)Sf(0, 0) * Sf(1, 1) - (double)Sf(0, 1) * Sf(1, 0)) * d);
        std::memcpy(D, t, sizeof(t));
    } else
        for (int k = 0; k < 9; k++) D[k] = 0;
}
#undef Sf

// ---- Initializer.cc ----------------------------------------------------------------------------

struct Point2f {
    float x, y;
};

// DUtils::Random::RandomInt(min, max) on the value r that rand() returned (Random.cpp:47-50)
int RandomInt(int r, int min, int max) {
    int d = max - min + 1;
    return int(((double)r / ((double)2147483647 + 1.0)) * d) + min;
}

void Normalize(const float* keys_xy, int N, std::vector<Point2f>& vNormalizedPoints, float* T) {
    float meanX = 0;
    float meanY = 0;
    vNormalizedPoints.resize(N);
    for (int i = 0; i < N; i++) {
        meanX += keys_xy[2 * i];
        meanY += keys_xy[2 * i + 1];
    }
    meanX = meanX / N;
    meanY = meanY / N;
    float meanDevX = 0;
    float meanDevY = 0;
    for (int i = 0; i < N; i++) {
        vNormalizedPoints[i].x = keys_xy[2 * i] - meanX;
        vNormalizedPoints[i].y = keys_xy[2 * i + 1] - meanY;
        meanDevX += std::abs(vNormalizedPoints[i].x);
        meanDevY += std::abs(vNormalizedPoints[i].y);
    }
    meanDevX = meanDevX / N;
    meanDevY = meanDevY / N;
    float sX = 1.0 / meanDevX;
    float sY = 1.0 / meanDevY;
    for (int i = 0; i < N; i++) {
        vNormalizedPoints[i].x = vNormalizedPoints[i].x * sX;
        vNormalizedPoints[i].y = vNormalizedPoints[i].y * sY;
    }
    for (int k = 0; k < 9; k++) T[k] = (k % 4 == 0) ? 1.0f : 0.0f;  // eye(3, 3, CV_32F)
    T[0] = sX;
    T[4] = sY;
    T[2] = -meanX * sX;
    T[5] = -meanY * sY;
}

void ComputeH21(const Point2f* vP1, const Point2f* vP2, float* H, std::vector<int>* signs = nullptr) {
    const int N = 8;
    float A[2 * N * 9];
    for (int i = 0; i < N; i++) {
        const float u1 = vP1[i].x;
        const float v1 = vP1[i].y;
        const float u2 = vP2[i].x;
        const float v2 = vP2[i].y;
        float* r0 = A + (2 * i) * 9;
        float* r1 = A + (2 * i + 1) * 9;
        r0[0] = 0.0;
        r0[1] = 0.0;
        r0[2] = 0.0;
        r0[3] = -u1;
        r0[4] = -v1;
        r0[5] = -1;
        r0[6] = v2 * u1;
        r0[7] = v2 * v1;
        r0[8] = v2;
        r1[0] = u1;
        r1[1] = v1;
        r1[2] = 1;
        r1[3] = 0.0;
        r1[4] = 0.0;
        r1[5] = 0.0;
        r1[6] = -u2 * u1;
        r1[7] = -u2 * v1;
        r1[8] = -u2;
    }
    float w[9], vt[81];
    SVDecomp(A, 2 * N, 9, w, nullptr, vt, signs);
    std::memcpy(H, vt + 8 * 9, 9 * sizeof(float));  // vt.row(8).reshape(0, 3)
}

// Fpre: vt.row(8) of the first decomposition, before the rank-2 enforcement (may be NULL)
void ComputeF21(const Point2f* vP1, const Point2f* vP2, float* F, float* Fpre_out, std::vector<int>* signs = nullptr) {
    const int N = 8;
    float A[N * 9];
    for (int i = 0; i < N; i++) {
        const float u1 = vP1[i].x;
        const float v1 = vP1[i].y;
        const float u2 = vP2[i].x;
        const float v2 = vP2[i].y;
        float* r = A + i * 9;
        r[0] = u2 * u1;
        r[1] = u2 * v1;
        r[2] = u2;
        r[3] = v2 * u1;
        r[4] = v2 * v1;
        r[5] = v2;
        r[6] = u1;
        r[7] = v1;
        r[8] = 1;
    }
    float w8[8], vt9[81];
    SVDecomp(A, N, 9, w8, nullptr, vt9, signs);
    float Fpre[9];
    std::memcpy(Fpre, vt9 + 8 * 9, sizeof(Fpre));
    if (Fpre_out) std::memcpy(Fpre_out, Fpre, sizeof(Fpre));
    float w[3], u[9], vt[9];
    SVDecomp(Fpre, 3, 3, w, u, vt, signs);
    w[2] = 0;
    const float D[9] = {w[0], 0, 0, 0, w[1], 0, 0, 0, w[2]};  // Mat::diag(w)
    float uD[9];
    mul3(u, D, uD);
    mul3(uD, vt, F);
}

}  // namespace

extern "C" {

// The minimal sets of Initializer.cc:80-95 for N matches from n_hyp x 8 rand() values.
// Returns -22 for N < 8 (the reference would pop from an empty vector) or a negative draw.
int initializer_ransac_model_sets(int N, int n_hyp, const int32_t* rand31, int32_t* sets) {
    if (N < 8) return -22;
    std::vector<size_t> vAllIndices, vAvailableIndices;
    for (int i = 0; i < N; i++) vAllIndices.push_back(i);
    for (int it = 0; it < n_hyp; it++) {
        vAvailableIndices = vAllIndices;
        for (size_t j = 0; j < 8; j++) {
            if (rand31[it * 8 + j] < 0) return -22;
            int randi = RandomInt(rand31[it * 8 + j], 0, vAvailableIndices.size() - 1);
            int idx = vAvailableIndices[randi];
            sets[it * 8 + j] = idx;
            vAvailableIndices[randi] = vAvailableIndices.back();
            vAvailableIndices.pop_back();
        }
    }
    return 0;
}

// Inputs as orb_initializer_compute_hypotheses, keypoints as n x 2 floats; either `sets` (n_hyp x
// 8 match ordinals) or `rand31` (n_hyp x 8).  Outputs (any may be NULL): H21, H12, F21, Hn, Fn,
// Fpre n_hyp x 9; T1, T2 9 floats; sets_out n_hyp x 8; *n_matches = N.  With N < 8 the hypothesis
// and set rows are zeros (T1 / T2 are still written).  Returns -22 for a matches12 entry outside
// [-1, n2), a negative draw or a set entry outside [0, N).
int initializer_ransac_model_hypotheses(const float* kps1_xy, int n1, const float* kps2_xy, int n2,
                                        const int32_t* matches12, int n_hyp, const int32_t* sets,
                                        const int32_t* rand31, float* H21, float* H12, float* F21, float* Hn_out,
                                        float* Fn_out, float* Fpre_out, float* T1_out, float* T2_out,
                                        int32_t* sets_out, int32_t* n_matches) {
    std::vector<std::pair<int, int>> mvMatches12;
    for (int i = 0; i < n1; i++) {  // Initializer.cc:54-63
        if (matches12[i] < -1 || matches12[i] >= n2) return -22;
        if (matches12[i] >= 0) mvMatches12.push_back(std::make_pair(i, matches12[i]));
    }
    const int N = (int)mvMatches12.size();
    if (n_matches) *n_matches = N;
    std::vector<Point2f> vPn1, vPn2;
    float T1[9], T2[9], T2inv[9], T2t[9];
    Normalize(kps1_xy, n1, vPn1, T1);
    Normalize(kps2_xy, n2, vPn2, T2);
    inv3(T2, T2inv);
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) T2t[r * 3 + c] = T2[c * 3 + r];
    if (T1_out) std::memcpy(T1_out, T1, sizeof(T1));
    if (T2_out) std::memcpy(T2_out, T2, sizeof(T2));
    float* outs[6] = {H21, H12, F21, Hn_out, Fn_out, Fpre_out};
    if (N < 8) {
        for (float* o : outs)
            if (o) std::memset(o, 0, sizeof(float) * 9 * n_hyp);
        if (sets_out) std::memset(sets_out, 0, sizeof(int32_t) * 8 * n_hyp);
        return 0;
    }
    std::vector<int32_t> mvSets((size_t)n_hyp * 8);
    if (sets) {
        for (int k = 0; k < n_hyp * 8; k++) {
            if (sets[k] < 0 || sets[k] >= N) return -22;
            mvSets[k] = sets[k];
        }
    } else if (int r = initializer_ransac_model_sets(N, n_hyp, rand31, mvSets.data()))
        return r;
    if (sets_out) std::memcpy(sets_out, mvSets.data(), sizeof(int32_t) * 8 * n_hyp);
    Point2f vPn1i[8], vPn2i[8];
    for (int it = 0; it < n_hyp; it++) {
        for (size_t j = 0; j < 8; j++) {
            int idx = mvSets[it * 8 + j];
            vPn1i[j] = vPn1[mvMatches12[idx].first];
            vPn2i[j] = vPn2[mvMatches12[idx].second];
        }
        float Hn[9], tmp[9], H21i[9], H12i[9];
        ComputeH21(vPn1i, vPn2i, Hn);
        mul3(T2inv, Hn, tmp);  // H21i = T2inv*Hn*T1
        mul3(tmp, T1, H21i);
        inv3(H21i, H12i);
        float Fn[9], Fpre[9], F21i[9];
        ComputeF21(vPn1i, vPn2i, Fn, Fpre);
        mul3(T2t, Fn, tmp);  // F21i = T2t*Fn*T1
        mul3(tmp, T1, F21i);
        const float* vals[6] = {H21i, H12i, F21i, Hn, Fn, Fpre};
        for (int o = 0; o < 6; o++)
            if (outs[o]) std::memcpy(outs[o] + 9 * it, vals[o], 9 * sizeof(float));
    }
    return 0;
}

// ComputeH21 / ComputeF21 on 8 given (already normalised) correspondences p1, p2 (8 x 2 floats).
// signs: capacity n_signs ints, the generator's signs in draw order; returns how many were drawn.
int initializer_ransac_model_compute(const float* p1, const float* p2, float* Hn, float* Fn, float* Fpre,
                                     int32_t* signs, int n_signs) {
    std::vector<int> sg;
    ComputeH21((const Point2f*)p1, (const Point2f*)p2, Hn, nullptr);
    ComputeF21((const Point2f*)p1, (const Point2f*)p2, Fn, Fpre, &sg);
    for (int k = 0; k < (int)sg.size() && k < n_signs; k++) signs[k] = sg[k];
    return (int)sg.size();
}

void initializer_ransac_model_inv3(const float* S, float* D) { inv3(S, D); }
void initializer_ransac_model_mul3(const float* a, const float* b, float* d) { mul3(a, b, d); }
// cv::SVDecomp of a rows x cols matrix: w, u (rows x rows, may be NULL), vt (cols x cols)
void initializer_ransac_model_svd(const float* A, int rows, int cols, float* w, float* u, float* vt) {
    SVDecomp(A, rows, cols, w, u, vt);
}

}  // extern "C"

#ifdef INITIALIZER_RANSAC_MODEL_MAIN
// Stand-alone run for the sanitizers: argv[1] = a file of int32 n1, n2, n_hyp, then n1 x 2 and
// n2 x 2 floats, n1 matches, n_hyp x 8 draws.  Prints a checksum of the hypotheses.
int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hdr[3];
    if (std::fread(hdr, 4, 3, f) != 3) return 2;
    const int n1 = hdr[0], n2 = hdr[1], n_hyp = hdr[2];
    std::vector<float> k1(2 * (size_t)n1), k2(2 * (size_t)n2);
    std::vector<int32_t> m12(n1), r31((size_t)n_hyp * 8), sets((size_t)n_hyp * 8);
    if (std::fread(k1.data(), 4, k1.size(), f) != k1.size() || std::fread(k2.data(), 4, k2.size(), f) != k2.size() ||
        std::fread(m12.data(), 4, m12.size(), f) != m12.size() || std::fread(r31.data(), 4, r31.size(), f) != r31.size())
        return 2;
    std::fclose(f);
    std::vector<float> H21(9 * (size_t)n_hyp), H12(H21), F21(H21), Hn(H21), Fn(H21), Fp(H21);
    float T1[9], T2[9];
    int32_t N = 0;
    int r = initializer_ransac_model_hypotheses(k1.data(), n1, k2.data(), n2, m12.data(), n_hyp, nullptr, r31.data(),
                                                H21.data(), H12.data(), F21.data(), Hn.data(), Fn.data(), Fp.data(),
                                                T1, T2, sets.data(), &N);
    double sum = 0;
    for (size_t k = 0; k < H21.size(); k++) sum += std::fabs(H21[k]) + std::fabs(H12[k]) + std::fabs(F21[k]);
    std::printf("initializer ransac model: status %d N %d checksum %.17g\n", r, (int)N, sum);
    return r ? 1 : 0;
}
#endif
