// orb_rot_hist.h — the rotation-consistency filter of the reference's matchers (rotHist,
// ComputeThreeMaxima and the removal pass, e.g. ORBmatcher.cc:664-676, 491-512, 1748-1789), shared
// by every kernel that applies it: k_resolve and k_resolve_fix (orb_match.hip), k_bow_pairs
// (orb_bow.hip), k_match_init (orb_sfi.hip).
//
// One definition of the bin and of the three maxima.  Float +, *, a compare and roundf only, no
// contraction (-ffp-contract=off): the same source compiled by a plain C++ compiler gives the same
// ints (tests/native/rot_hist_host.cpp pins them against the oracle's rot_bin and the Python
// restatement of tests/test_matcher_oracle.py).
#pragma once
#include <math.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define ORB_ROT_FN __host__ __device__ __forceinline__
#else
#define ORB_ROT_FN inline __attribute__((always_inline))
#endif

namespace orb_rot {

constexpr int HISTO_LENGTH = 30;  // ORBmatcher.cc:42

// The histogram bin of a pair's rotation a1 - a2 (ORBmatcher.cc:668-675): factor = 1.0f / HISTO_LENGTH,
// round() half away from zero, bin HISTO_LENGTH wraps to 0.
ORB_ROT_FN int rot_bin(float a1, float a2) {
    float rot = a1 - a2;
    if (rot < 0.0f) rot += 360.0f;
    int bin = (int)roundf(rot * (1.0f / HISTO_LENGTH));
    if (bin == HISTO_LENGTH) bin = 0;
    return bin;
}

// ComputeThreeMaxima (ORBmatcher.cc:1748-1789) on the bins' counts: the strict > insertion scan in
// bin order (an equal count never displaces an earlier bin, an empty bin is never chosen), then the
// second and third maximum dropped when below 0.1f of the first, compared in float.  ind[0..2] = the
// kept bins, -1 where there is none.
ORB_ROT_FN void three_maxima(const int* hist, int* ind) {
    int max1 = 0, max2 = 0, max3 = 0, ind1 = -1, ind2 = -1, ind3 = -1;
    for (int i = 0; i < HISTO_LENGTH; ++i) {
        const int s = hist[i];
        if (s > max1) {
            max3 = max2;
            max2 = max1;
            max1 = s;
            ind3 = ind2;
            ind2 = ind1;
            ind1 = i;
        } else if (s > max2) {
            max3 = max2;
            max2 = s;
            ind3 = ind2;
            ind2 = i;
        } else if (s > max3) {
            max3 = s;
            ind3 = i;
        }
    }
    if (max2 < 0.1f * (float)max1) {
        ind2 = -1;
        ind3 = -1;
    } else if (max3 < 0.1f * (float)max1) {
        ind3 = -1;
    }
    ind[0] = ind1;
    ind[1] = ind2;
    ind[2] = ind3;
}

}  // namespace orb_rot
