// sim3_optimizer_facade.cpp — gpu::Optimizer::OptimizeSim3 (include/orb_slam_gpu.hpp) driven through
// the C ABI the way LoopClosing::ComputeSim3 drives Optimizer::OptimizeSim3(mpCurrentKF, pKF,
// vpMapPointMatches, gScm, 10) and then reads the matches and gScm (reference
// src/LoopClosing.cc:340-350).  Input: a binary file written by tests/test_gpu_sim3_optimization.py:
//   int32 n1, n2, nlev | 4 floats K1 | 4 floats K2 | float th2 | 13 floats S12 |
//   n1 x 28-byte keypoints of KF1 | n2 x 28-byte keypoints of KF2 | nlev floats invLevelSigma2 |
//   nlev floats levelSigma2 | n1 int32 vpMatches1 (i2 or -1) | n1 x 3 floats P3D1c | n1 x 3 floats P3D2c
// Output:
//   SIM3OPT inliers=<return value> matched=<slots still >= 0> hash=<fnv of the slots' state> bad=<nBad> more=<nMoreIterations>
//   S12 <13 floats as hex bit patterns>
// and "sim3 optimizer facade OK".  The test compares the lines with the CPU model's answer.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/orb_slam_gpu.hpp"

template <class T>
static bool rd(std::FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hdr[3];
    float K1[4], K2[4], th2, S12[13];
    if (std::fread(hdr, 4, 3, f) != 3 || std::fread(K1, 4, 4, f) != 4 || std::fread(K2, 4, 4, f) != 4 ||
        std::fread(&th2, 4, 1, f) != 1 || std::fread(S12, 4, 13, f) != 13)
        return 2;
    const int n1 = hdr[0], n2 = hdr[1], nlev = hdr[2];
    std::vector<orb_keypoint_t> keys1, keys2;
    std::vector<float> inv, sig, p1, p2;
    std::vector<int> matches;
    if (!rd(f, keys1, n1) || !rd(f, keys2, n2) || !rd(f, inv, nlev) || !rd(f, sig, nlev) || !rd(f, matches, n1) ||
        !rd(f, p1, (size_t)n1 * 3) || !rd(f, p2, (size_t)n1 * 3))
        return 2;
    std::fclose(f);
    try {
        ORB_SLAM::gpu::FrameView KF1{keys1.data(), nullptr, n1, {0, 0, 0, 0}};
        ORB_SLAM::gpu::FrameView KF2{keys2.data(), nullptr, n2, {0, 0, 0, 0}};
        orb_sim3_opt_info_t info;
        const int n = ORB_SLAM::gpu::Optimizer::OptimizeSim3(KF1, KF2, inv, sig, K1, K2, matches, p1, p2, S12, th2, 0,
                                                             &info);
        unsigned h = 2166136261u;
        int set = 0;
        for (size_t i = 0; i < matches.size(); ++i) {
            h = (h ^ (matches[i] >= 0 ? 1u : 0u)) * 16777619u;
            set += matches[i] >= 0 ? 1 : 0;
        }
        std::printf("SIM3OPT inliers=%d matched=%d hash=%08x bad=%d more=%d\n", n, set, h, info.n_bad,
                    info.more_iterations);
        std::printf("S12");
        for (int k = 0; k < 13; ++k) {
            uint32_t u;
            std::memcpy(&u, &S12[k], 4);
            std::printf(" %08x", u);
        }
        std::printf("\n");
    } catch (const std::exception& e) {
        std::printf("FAIL exception: %s\n", e.what());
        return 2;
    }
    std::printf("sim3 optimizer facade OK\n");
    return 0;
}
