// optimizer_facade.cpp — gpu::Optimizer::PoseOptimization (include/orb_slam_gpu.hpp) driven through
// the C ABI the way Tracking drives Optimizer::PoseOptimization(&mCurrentFrame) and then reads
// mvbOutlier and mTcw (reference src/Tracking.cc:611-625).  Input: a binary file written by
// tests/test_gpu_pose_optimization.py:
//   int32 nk, nlev | 4 floats K | 12 floats Tcw | nk x 28-byte keypoints | nlev floats invLevelSigma2 |
//   nk u8 hasMP | nk x 3 floats worldPos
// Output:
//   POSEOPT inliers=<return value> flags=<set bits of mvbOutlier> hash=<fnv of mvbOutlier> rounds=<rounds>
//   TCW <12 floats as hex bit patterns>
// and "optimizer facade OK".  The test compares the lines with the CPU model's answer.
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
    int32_t hdr[2];
    float K[4], Tcw[12];
    if (std::fread(hdr, 4, 2, f) != 2 || std::fread(K, 4, 4, f) != 4 || std::fread(Tcw, 4, 12, f) != 12) return 2;
    const int nk = hdr[0], nlev = hdr[1];
    std::vector<orb_keypoint_t> keys;
    std::vector<float> inv, pos;
    std::vector<uint8_t> has;
    if (!rd(f, keys, nk) || !rd(f, inv, nlev) || !rd(f, has, nk) || !rd(f, pos, (size_t)nk * 3)) return 2;
    std::fclose(f);
    try {
        ORB_SLAM::gpu::FrameView F{keys.data(), nullptr, nk, {0, 0, 0, 0}};
        std::vector<bool> mvbOutlier;
        orb_pose_opt_info_t info;
        const int n = ORB_SLAM::gpu::Optimizer::PoseOptimization(F, inv, K[0], K[1], K[2], K[3], has, pos, Tcw,
                                                                 mvbOutlier, 0, &info);
        unsigned h = 2166136261u;
        int set = 0;
        for (size_t i = 0; i < mvbOutlier.size(); ++i) {
            h = (h ^ (mvbOutlier[i] ? 1u : 0u)) * 16777619u;
            set += mvbOutlier[i] ? 1 : 0;
        }
        std::printf("POSEOPT inliers=%d flags=%d hash=%08x rounds=%d\n", n, set, h, info.rounds);
        std::printf("TCW");
        for (int k = 0; k < 12; ++k) {
            uint32_t u;
            std::memcpy(&u, &Tcw[k], 4);
            std::printf(" %08x", u);
        }
        std::printf("\n");
    } catch (const std::exception& e) {
        std::printf("FAIL exception: %s\n", e.what());
        return 2;
    }
    std::printf("optimizer facade OK\n");
    return 0;
}
