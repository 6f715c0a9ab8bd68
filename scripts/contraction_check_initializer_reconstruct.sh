#!/bin/bash
# Which fused multiply-adds the reference build (g++ -O3 -march=native, CMakeLists.txt:13; -mavx2
# -mfma here) makes of the scalar float expressions of CheckRT (Initializer.cc:796-905),
# ReconstructH (606-614, 649-651) and DecomposeE (907-927), DESIGN.md §18.  Each statement group is
# re-typed as one function over plain floats (`at(i)` stands for Mat::at<float>, a load), compiled
# as the reference is and disassembled per function.  The fusions found are written as explicit
# fmaf in tests/native/initializer_reconstruct_model.cpp and csrc/orb_initializer.hip, which are
# built -ffp-contract=off.  cv::Mat expressions (K*P2, R*p+t, t/norm(t), ...) are OpenCV's own code
# and are taken as built without FMA (oracle/ocv_ops.h).  DecomposeE has no scalar float
# arithmetic of its own (three stores into W and Mat expressions): nothing to compile.
# `acos(x)*180/CV_PI` is compiled as Initializer.cc sees it: <cmath> comes in through the OpenCV
# headers and `using namespace std` through Frame.h -> ORBVocabulary.h -> TemplatedVocabulary.h, so
# the unqualified `acos` on a float binds std::acos(float); the call printed for `parallax` shows
# the libm symbol (acosf), then `*180` in float and `/CV_PI` in double.
set -e
T=$(mktemp -d)
cat > $T/rec.cpp <<'CPP'
#include <cmath>
#include <vector>
#include <algorithm>
#define CV_PI 3.1415926535897932384626433832795
using namespace std;
struct Pt { float x, y; };
// CheckRT 866-870 / 877-881: one image's reprojection and squared error
float reproj(float fx, float fy, float cx, float cy, const float* at, Pt kp) {
    float im1x, im1y;
    float invZ1 = 1.0 / at[2];
    im1x = fx * at[0] * invZ1 + cx;
    im1y = fy * at[1] * invZ1 + cy;
    float squareError1 = (im1x - kp.x) * (im1x - kp.x) + (im1y - kp.y) * (im1y - kp.y);
    return squareError1;
}
// CheckRT 852: dot is Mat::dot's double, dist1 / dist2 floats
float cosp(double dot, float dist1, float dist2) {
    float cosParallax = dot / (dist1 * dist2);
    return cosParallax;
}
// CheckRT 492 / 701: the th2 argument
float th2(float mSigma2) { return 4.0 * mSigma2; }
// CheckRT 899
float parallax(const vector<float>& vCosParallax, size_t idx) {
    float p = acos(vCosParallax[idx]) * 180 / CV_PI;
    return p;
}
// ReconstructH 595
bool gate(float d1, float d2, float d3) { return d1 / d2 < 1.00001 || d2 / d3 < 1.00001; }
// ReconstructH 606-614
void auxs(float d1, float d2, float d3, float* o) {
    float aux1 = sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3));
    float aux3 = sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
    float aux_stheta = sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2);
    float ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
    o[0] = aux1;
    o[1] = aux3;
    o[2] = aux_stheta;
    o[3] = ctheta;
}
// ReconstructH 649-651
void auxp(float d1, float d2, float d3, float* o) {
    float aux_sphi = sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2);
    float cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
    o[0] = aux_sphi;
    o[1] = cphi;
}
// ReconstructH 606-651 as one function, as the reference has them (common subexpressions shared)
void auxall(float d1, float d2, float d3, float* o) {
    float aux1 = sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3));
    float aux3 = sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
    float aux_stheta = sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2);
    float ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
    float aux_sphi = sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2);
    float cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
    o[0] = aux1;
    o[1] = aux3;
    o[2] = aux_stheta;
    o[3] = ctheta;
    o[4] = aux_sphi;
    o[5] = cphi;
}
CPP
g++ -std=c++11 -O3 -mavx2 -mfma -c -o $T/rec.o $T/rec.cpp
objdump -d -r -C --no-show-raw-insn $T/rec.o > $T/rec.txt
echo "fused multiply-adds in all: $(grep -cE 'vfn?m(add|sub)' $T/rec.txt || true)"
awk '/^[0-9a-f]+ <.*>:$/ { fn = $2 } /vfn?m(add|sub)|vmulss|vsubss|vaddss|vdivs[sd]|vsqrts[sd]|R_X86_64_PLT32/ { print fn, $0 }' $T/rec.txt |
    sed 's/^\(<[^>]*>:\) *[0-9a-f]*:\s*/\1 /'
rm -rf $T
