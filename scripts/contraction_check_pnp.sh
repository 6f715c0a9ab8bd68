#!/bin/bash
# Evidence for the FMA contraction pattern that csrc/orb_epnp_math.h writes explicitly: the
# expression SHAPES of the EPnP functions that sit in the reference's own translation unit
# (PnPsolver.cc:347-922; the cvMulTransposed / cvSVD / cvInvert / cvSolve calls between them are
# OpenCV's binary and are not contracted), re-typed as minimal functions over plain arrays, compiled
# as the reference build compiles them (g++ -O3 -march=native, CMakeLists.txt:13; -mavx2 -mfma here)
# and disassembled, one function per shape so that the listing can be read against DESIGN.md §17.
# Read (AT&T operand order, destination last): vfmadd231sd A,B,C = C + A*B; vfmadd213sd M,A,B =
# A*B + M (into B); vfmadd132sd M,A,B = B*M + A (into B); vfnmadd* = the same with the product
# negated; the pd forms are the same operations on 2 or 4 values at once.
set -e
T=$(mktemp -d)
cat > $T/shapes.cpp <<'CPP'
#include <cmath>
// dot / dist2 (PnPsolver.cc:509-520): three products, two additions
double shape_dot(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
double shape_dist2(const double* p, const double* q) {
    return (p[0] - q[0]) * (p[0] - q[0]) + (p[1] - q[1]) * (p[1] - q[1]) + (p[2] - q[2]) * (p[2] - q[2]);
}
// choose_control_points :379: c0 + k*u
double shape_cw(double c0, double k, double u) { return c0 + k * u; }
// compute_barycentric_coordinates :400-404
void shape_alpha(const double* ci, const double* pi, const double* c0, double* a) {
    for (int j = 0; j < 3; j++)
        a[1 + j] = ci[3 * j] * (pi[0] - c0[0]) + ci[3 * j + 1] * (pi[1] - c0[1]) + ci[3 * j + 2] * (pi[2] - c0[2]);
    a[0] = 1.0f - a[1] - a[2] - a[3];
}
// compute_ccs :434 and compute_pcs :445
void shape_ccs(double* ccs, double beta, const double* v) {
    for (int j = 0; j < 12; j++) ccs[j] += beta * v[j];
}
double shape_pc(const double* a, const double* c0, const double* c1, const double* c2, const double* c3) {
    return a[0] * c0[0] + a[1] * c1[0] + a[2] * c2[0] + a[3] * c3[0];
}
// reprojection_error :528-535
double shape_reproj(const double* R, const double* t, const double* pw, double fu, double fv, double uc, double vc,
                    double u, double v) {
    double Xc = shape_dot(R, pw) + t[0];
    double Yc = shape_dot(R + 3, pw) + t[1];
    double inv_Zc = 1.0 / (shape_dot(R + 6, pw) + t[2]);
    double ue = uc + fu * Xc * inv_Zc;
    double ve = vc + fv * Yc * inv_Zc;
    return std::sqrt((u - ue) * (u - ue) + (v - ve) * (v - ve));
}
// estimate_R_and_t :574-576, :586-588, :596
void shape_abt(double* abt, const double* pc, const double* pc0, const double* pw, const double* pw0) {
    for (int j = 0; j < 3; j++) {
        abt[3 * j] += (pc[j] - pc0[j]) * (pw[0] - pw0[0]);
        abt[3 * j + 1] += (pc[j] - pc0[j]) * (pw[1] - pw0[1]);
        abt[3 * j + 2] += (pc[j] - pc0[j]) * (pw[2] - pw0[2]);
    }
}
double shape_det(const double R[3][3]) {
    return R[0][0] * R[1][1] * R[2][2] + R[0][1] * R[1][2] * R[2][0] + R[0][2] * R[1][0] * R[2][1] -
           R[0][2] * R[1][1] * R[2][0] - R[0][1] * R[1][0] * R[2][2] - R[0][0] * R[1][2] * R[2][1];
}
double shape_t(double pc0, const double* R, const double* pw0) { return pc0 - shape_dot(R, pw0); }
// compute_A_and_b_gauss_newton :791-808
void shape_gn(const double* rowL, const double* betas, const double* rho, double* rowA, double* b) {
    rowA[0] = 2 * rowL[0] * betas[0] + rowL[1] * betas[1] + rowL[3] * betas[2] + rowL[6] * betas[3];
    rowA[1] = rowL[1] * betas[0] + 2 * rowL[2] * betas[1] + rowL[4] * betas[2] + rowL[7] * betas[3];
    rowA[2] = rowL[3] * betas[0] + rowL[4] * betas[1] + 2 * rowL[5] * betas[2] + rowL[8] * betas[3];
    rowA[3] = rowL[6] * betas[0] + rowL[7] * betas[1] + rowL[8] * betas[2] + 2 * rowL[9] * betas[3];
    *b = rho[0] - (rowL[0] * betas[0] * betas[0] + rowL[1] * betas[0] * betas[1] + rowL[2] * betas[1] * betas[1] +
                   rowL[3] * betas[0] * betas[2] + rowL[4] * betas[1] * betas[2] + rowL[5] * betas[2] * betas[2] +
                   rowL[6] * betas[0] * betas[3] + rowL[7] * betas[1] * betas[3] + rowL[8] * betas[2] * betas[3] +
                   rowL[9] * betas[3] * betas[3]);
}
// qr_solve :864-888, :896-906, :916-920: the scaled column's square sum, the column dot, the two updates
double shape_qr_norm(double* col, int nc, int nr, double inv_eta) {
    double sum = 0.0;
    for (int i = 0; i < nr; i++) {
        *col *= inv_eta;
        sum += *col * *col;
        col += nc;
    }
    return sum;
}
double shape_qr_dot(const double* col, int nc, int nr, int jk) {
    double sum = 0;
    for (int i = 0; i < nr; i++) {
        sum += *col * col[jk];
        col += nc;
    }
    return sum;
}
void shape_qr_update(double* col, int nc, int nr, int jk, double tau) {
    for (int i = 0; i < nr; i++) {
        col[jk] -= tau * *col;
        col += nc;
    }
}
CPP
g++ -O3 -mavx2 -mfma -fno-tree-vectorize -c -o $T/shapes.o $T/shapes.cpp
objdump -d --no-show-raw-insn -C $T/shapes.o | grep -E "^[0-9a-f]+ <|vfm|vfnm|vmul|vadd|vsub|vdiv|vsqrt|vxor"
rm -rf $T
