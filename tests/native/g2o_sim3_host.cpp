// g2o_sim3_host.cpp — the Sim3 part of csrc/orb_g2o_math.h compiled as plain C++
// (build/libg2o_sim3_host.so): struct Sim3 with its map, inverse, product, the conversions from and to a
// pose, the 3 x 3 LU solve and log().  tests/test_essential_graph_model.py pins them against the
// statement of the same functions that tests/native/essential_graph_model.cpp writes from g2o's sources.
// Sims are eight doubles: q (x y z w), t, s.
#include <cstring>

#include "../../orbslam_jpminipc_amd/csrc/orb_g2o_math.h"

static Sim3 ld(const double* p) {
    Sim3 S;
    std::memcpy(&S, p, sizeof S);
    return S;
}
static void st(const Sim3& S, double* p) { std::memcpy(p, &S, sizeof S); }

extern "C" {

void s3h_from_pose(const float* Tcw, double* o) { st(sim3_from_pose(Tcw), o); }
void s3h_to_pose(const double* s, double* M) { sim3_to_pose(ld(s), M); }
void s3h_mul(const double* a, const double* b, double* o) { st(sim3_mul(ld(a), ld(b)), o); }
void s3h_inverse(const double* a, double* o) { st(sim3_inverse(ld(a)), o); }
void s3h_map(const double* a, const double* X, double* o) { sim3_map(ld(a), X, o); }
void s3h_lu3_solve(const double* W, const double* t, double* x) { lu3_solve(W, t, x); }
int s3h_log(const double* a, double* res) {
    Sim3LogTrace tr;
    sim3_log(ld(a), res, &tr);
    return tr.branch;
}

}  // extern "C"
