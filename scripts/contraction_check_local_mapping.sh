#!/bin/bash
# Which fused multiply-adds the reference build (g++ -O3 -march=native, CMakeLists.txt:13; -mavx2
# -mfma here) makes of the scalar float expressions of LocalMapping::CreateNewMapPoints
# (LocalMapping.cc:246-249, 300-304, 329-373) and MapPoint::UpdateNormalAndDepth (MapPoint.cc:300-309),
# DESIGN.md §20.  Each statement group is written as one function over plain floats (a `dot` argument
# stands for Mat::dot's double, `at` for Mat::at<float>, a load), compiled as the reference is and
# disassembled per function.  The fusions found are written as explicit fmaf in
# tests/native/local_mapping_model.cpp, csrc/orb_localmap.hip and csrc/orb_mappoint.hip, which are
# built -ffp-contract=off.  cv::Mat expressions (Rwc*xn, the rows of A, x3D/w, normal + normali/n, ...)
# are OpenCV's own code and are taken as built without FMA (oracle/ocv_ops.h).
set -e
T=$(mktemp -d)
cat > $T/lm.cpp <<'CPP'
struct Pt { float x, y; };
// 300 / 302: the two first entries of xn
void xn(Pt pt, float cx, float cy, float invfx, float invfy, float* o) {
    o[0] = (pt.x - cx) * invfx;
    o[1] = (pt.y - cy) * invfy;
}
// 246-247, 249
void consts(float fx, float fy, float scaleFactor, float* o) {
    const float invfx = 1.0f / fx;
    const float invfy = 1.0f / fy;
    const float ratioFactor = 1.5f * scaleFactor;
    o[0] = invfx, o[1] = invfy, o[2] = ratioFactor;
}
// 304, 306: dot and the norms are doubles
bool parallax(double dot, double n1, double n2, float* out) {
    const float cosParallaxRays = dot / (n1 * n2);
    *out = cosParallaxRays;
    return cosParallaxRays < 0 || cosParallaxRays > 0.9998;
}
// 329-330: a depth and its gate
bool depth(double dot, float t, float* z) {
    float z1 = dot + t;
    *z = z1;
    return z1 <= 0;
}
// 338-347: one image's reprojection and its gate
bool reproj(float fx, float fy, float cx, float cy, double dotx, double doty, float tx, float ty, float z1, Pt kp,
            float sigmaSquare1) {
    float x1 = dotx + tx;
    float y1 = doty + ty;
    float invz1 = 1.0 / z1;
    float u1 = fx * x1 * invz1 + cx;
    float v1 = fy * y1 * invz1 + cy;
    float errX1 = u1 - kp.x;
    float errY1 = v1 - kp.y;
    return (errX1 * errX1 + errY1 * errY1) > 5.991 * sigmaSquare1;
}
// 363-373: the distances are cv::norm's doubles
int ratio(double n1, double n2, float sf1, float sf2, float ratioFactor) {
    float dist1 = n1;
    float dist2 = n2;
    if (dist1 == 0 || dist2 == 0) return 8;
    float ratioDist = dist1 / dist2;
    float ratioOctave = sf1 / sf2;
    if (ratioDist * ratioFactor < ratioOctave || ratioDist > ratioOctave * ratioFactor) return 9;
    return 1;
}
// LocalMapping.cc 260-264
bool baseline(double nb, float medianDepthKF2) {
    const float baseline = nb;
    const float ratioBaselineDepth = baseline / medianDepthKF2;
    return ratioBaselineDepth < 0.01;
}
// KeyFrame.cc 681
float mediandepth(double dot, float zcw) {
    float z = dot + zcw;
    return z;
}
// MapPoint.cc 300, 308-309
void distances(double n, float scaleFactor, float levelScaleFactor, float topScaleFactor, float* o) {
    const float dist = n;
    o[0] = (1.0f / scaleFactor) * dist / levelScaleFactor;
    o[1] = scaleFactor * dist * topScaleFactor;
}
CPP
g++ -std=c++11 -O3 -mavx2 -mfma -c -o $T/lm.o $T/lm.cpp
objdump -d -r -C --no-show-raw-insn $T/lm.o > $T/lm.txt
echo "fused multiply-adds in all: $(grep -cE 'vfn?m(add|sub)' $T/lm.txt || true)"
awk '/^[0-9a-f]+ <.*>:$/ { fn = $2 } /vfn?m(add|sub)|vmuls[sd]|vsubss|vadds[sd]|vdivs[sd]|vsqrts[sd]|R_X86_64_PLT32/ { print fn, $0 }' $T/lm.txt |
    sed 's/^\(<[^>]*>:\) *[0-9a-f]*:\s*/\1 /'
rm -rf $T
