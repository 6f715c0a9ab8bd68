#!/bin/bash
# Evidence that Initializer::Normalize (Initializer.cc:747-793) offers the reference build no FMA
# contraction: the function re-typed over plain arrays, compiled as the reference build compiles it
# (g++ -O3 -march=native, CMakeLists.txt:13; -mavx2 -mfma here) and disassembled.  Every product
# is stored or is the only operation of its statement, so no vfmadd* / vfnmadd* / vfmsub* may
# appear; the script prints their count (expected 0) and the multiplies it does find.
# The same holds by reading for ComputeH21 / ComputeF21 (224-301: every product is stored into A)
# and the set loop (80-95: integers); the OpenCV routines they call are taken as built without FMA
# (oracle/ocv_ops.h).
set -e
T=$(mktemp -d)
cat > $T/normalize.cpp <<'CPP'
#include <cmath>
#include <cstdlib>
#include <vector>
using namespace std;
struct KeyPoint { struct { float x, y; } pt; float size, angle, response; int octave, class_id; };
struct Point2f { float x, y; };
void Normalize(const vector<KeyPoint>& vKeys, vector<Point2f>& vNormalizedPoints, float* T) {
    float meanX = 0;
    float meanY = 0;
    const int N = vKeys.size();
    vNormalizedPoints.resize(N);
    for (int i = 0; i < N; i++) {
        meanX += vKeys[i].pt.x;
        meanY += vKeys[i].pt.y;
    }
    meanX = meanX / N;
    meanY = meanY / N;
    float meanDevX = 0;
    float meanDevY = 0;
    for (int i = 0; i < N; i++) {
        vNormalizedPoints[i].x = vKeys[i].pt.x - meanX;
        vNormalizedPoints[i].y = vKeys[i].pt.y - meanY;
        meanDevX += abs(vNormalizedPoints[i].x);
        meanDevY += abs(vNormalizedPoints[i].y);
    }
    meanDevX = meanDevX / N;
    meanDevY = meanDevY / N;
    float sX = 1.0 / meanDevX;
    float sY = 1.0 / meanDevY;
    for (int i = 0; i < N; i++) {
        vNormalizedPoints[i].x = vNormalizedPoints[i].x * sX;
        vNormalizedPoints[i].y = vNormalizedPoints[i].y * sY;
    }
    for (int k = 0; k < 9; k++) T[k] = k % 4 == 0;
    T[0] = sX;
    T[4] = sY;
    T[2] = -meanX * sX;
    T[5] = -meanY * sY;
}
CPP
g++ -std=c++11 -O3 -mavx2 -mfma -c -o $T/normalize.o $T/normalize.cpp
objdump -d --no-show-raw-insn $T/normalize.o > $T/normalize.txt
echo "fused multiply-adds: $(grep -cE 'vfn?m(add|sub)' $T/normalize.txt || true)"
echo "multiplies:"
grep -E 'vmul(ss|ps)' $T/normalize.txt | sed 's/^ *[0-9a-f]*:\s*/    /' | sort | uniq -c
rm -rf $T
