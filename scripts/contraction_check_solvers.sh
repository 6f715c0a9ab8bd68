#!/bin/bash
# Evidence for the FMA contraction pattern that csrc/orb_solvers.hip and
# tests/native/solvers_model.cpp write explicitly: the expression SHAPES of
# PnPsolver::CheckInliers (PnPsolver.cc:280-311) and of the lines of Sim3Solver::Project /
# FromCameraToImage that sit in the reference's own translation unit (Sim3Solver.cc:392-396,
# 412-416; the cv::Mat products, differences and dot() around them are OpenCV's binary and are
# not contracted), re-typed as minimal loops over pre-gathered values, compiled as the reference
# build compiles them (g++ -O3 -march=native, CMakeLists.txt:13; -mavx2 -mfma here) and
# disassembled.
# Read (AT&T operand order, destination last): vfmadd231sd A,B,C = C + A*B; vfmadd213sd M,A,B =
# A*B + M (into B); vfmadd132sd M,A,B = B*M + A (into B); the ss forms likewise in float.
set -e
T=$(mktemp -d)
cat > $T/shapes.cpp <<'CPP'
struct P3 { float x, y, z; };
struct P2 { float x, y; };
struct PnP {
    double R[3][3], t[3];
    double uc, vc, fu, fv;
    int pnp_check(const P3* w, const P2* p, const float* maxerr, int N, bool* in) {
        int cnt = 0;
        for (int i = 0; i < N; i++) {
            P3 W = w[i];
            P2 I = p[i];
            float Xc = R[0][0] * W.x + R[0][1] * W.y + R[0][2] * W.z + t[0];
            float Yc = R[1][0] * W.x + R[1][1] * W.y + R[1][2] * W.z + t[1];
            float invZc = 1 / (R[2][0] * W.x + R[2][1] * W.y + R[2][2] * W.z + t[2]);
            double ue = uc + fu * Xc * invZc;
            double ve = vc + fv * Yc * invZc;
            float distX = I.x - ue;
            float distY = I.y - ve;
            float error2 = distX * distX + distY * distY;
            if (error2 < maxerr[i]) {
                in[i] = true;
                cnt++;
            } else
                in[i] = false;
        }
        return cnt;
    }
};
int pnp_entry(PnP* s, const P3* w, const P2* p, const float* maxerr, int N, bool* in) {
    return s->pnp_check(w, p, maxerr, N, in);
}
// P: the 3-vector that came out of cv::Mat arithmetic; out: the two values pushed into a Mat_<float>
void sim3_to_image(const P3* P, int N, float fx, float fy, float cx, float cy, P2* out) {
    for (int i = 0; i < N; i++) {
        float invz = 1 / (P[i].z);
        float x = P[i].x * invz;
        float y = P[i].y * invz;
        out[i].x = fx * x + cx;
        out[i].y = fy * y + cy;
    }
}
// the bound of Sim3Solver.cc:87-88 pushed into a std::vector<size_t>, and the compare of line 351
unsigned long sim3_bound(float sigma2) { return 9.210 * sigma2; }
bool sim3_less(float err, unsigned long bound) { return err < bound; }
CPP
g++ -O3 -mavx2 -mfma -fno-tree-vectorize -c -o $T/shapes.o $T/shapes.cpp
objdump -d --no-show-raw-insn -C $T/shapes.o | grep -E "^[0-9a-f]+ <|vfm|vfnm|vmul|vadd|vsub|vdiv|vcvt|vcomis|vucomis|vxor"
echo "--- sim3_to_image as the vectoriser leaves it (packed forms, same contraction) ---"
g++ -O3 -mavx2 -mfma -c -o $T/shapes_v.o $T/shapes.cpp
objdump -d --no-show-raw-insn -C $T/shapes_v.o | awk '/<sim3_to_image/,/<sim3_bound/' | grep -E "^[0-9a-f]+ <|vfm|vfnm|vmul|vdiv|vrcp"
rm -rf $T
