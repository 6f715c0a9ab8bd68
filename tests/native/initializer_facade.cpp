// initializer_facade.cpp — gpu::Initializer (include/orb_slam_gpu.hpp) driven through the C ABI the
// way Initializer::Initialize drives FindHomography / FindFundamental (reference
// src/Initializer.cc:98-110).  Input: a binary file written by tests/test_gpu_initializer.py:
//   int32 n1, n2, n_hyp | n1 x 28-byte keypoints | n2 x 28-byte keypoints | n1 int32 matches12 |
//   n_hyp x 9 floats H21 | H12 | F21
// Output, one line per model, floats as their bit patterns:
//   H best=<index> score=0x<hex> inliers=<count> N=<N>
//   F best=<index> score=0x<hex> inliers=<count> N=<N>
// and "initializer facade OK".  The test compares the lines with the CPU model's answer.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/orb_slam_gpu.hpp"

template <class T>
static bool rd(std::FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

static void report(const char* tag, int best, float score, const std::vector<bool>& in, const std::vector<float>& M,
                   const std::vector<float>& all) {
    uint32_t bits;
    std::memcpy(&bits, &score, 4);
    int cnt = 0;
    for (size_t i = 0; i < in.size(); ++i) cnt += in[i] ? 1 : 0;
    std::printf("%s best=%d score=0x%08x inliers=%d N=%d\n", tag, best, bits, cnt, (int)in.size());
    // the returned matrix is the winning iteration's
    if (best >= 0 && (M.size() != 9 || std::memcmp(M.data(), &all[(size_t)best * 9], 36) != 0))
        std::printf("FAIL %s matrix is not hypothesis %d\n", tag, best);
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hdr[3];
    if (std::fread(hdr, 4, 3, f) != 3) return 2;
    const int n1 = hdr[0], n2 = hdr[1], n_hyp = hdr[2];
    std::vector<orb_keypoint_t> k1, k2;
    std::vector<int32_t> m12;
    std::vector<float> H21, H12, F21;
    if (!rd(f, k1, n1) || !rd(f, k2, n2) || !rd(f, m12, n1) || !rd(f, H21, (size_t)n_hyp * 9) ||
        !rd(f, H12, (size_t)n_hyp * 9) || !rd(f, F21, (size_t)n_hyp * 9))
        return 2;
    std::fclose(f);
    try {
        ORB_SLAM::gpu::Initializer init(k1, 1.0f, n_hyp);
        const int N = init.SetMatches(k2, std::vector<int>(m12.begin(), m12.end()));
        std::vector<bool> vbMatchesInliersH, vbMatchesInliersF;
        float SH, SF;
        std::vector<float> H, F;
        const int bh = init.FindHomography(H21, H12, vbMatchesInliersH, SH, H);
        const int bf = init.FindFundamental(F21, vbMatchesInliersF, SF, F);
        if ((int)vbMatchesInliersH.size() != N || (int)vbMatchesInliersF.size() != N) std::printf("FAIL N\n");
        report("H", bh, SH, vbMatchesInliersH, H, H21);
        report("F", bf, SF, vbMatchesInliersF, F, F21);
    } catch (const std::exception& e) {
        std::printf("FAIL exception: %s\n", e.what());
        return 2;
    }
    std::printf("initializer facade OK\n");
    return 0;
}
