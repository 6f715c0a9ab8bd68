// initializer_ransac_facade.cpp — gpu::Initializer::Initialize (include/orb_slam_gpu.hpp) driven
// through the C ABI the way Tracking drives Initializer::Initialize, with the values rand() would
// have returned.  Input: a binary file written by tests/test_gpu_initializer_ransac.py:
//   int32 n1, n2, n_hyp | n1 x 28-byte keypoints | n2 x 28-byte keypoints | n1 int32 matches12 |
//   n_hyp x 8 int32 draws
// Output, floats as their bit patterns:
//   N=<N> useH=<0|1> RH=0x<hex>
//   H score=0x<hex> inliers=<count> m=<nine hex words or "empty">
//   F score=0x<hex> inliers=<count> m=<nine hex words or "empty">
//   sets=<sum over iterations it and positions j of (it * 8 + j + 1) * index, modulo 2^32>
// and "initializer ransac facade OK".  The test compares the lines with the CPU model's answer.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/orb_slam_gpu.hpp"

template <class T>
static bool rd(std::FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

static uint32_t bits(float x) {
    uint32_t b;
    std::memcpy(&b, &x, 4);
    return b;
}

static void report(const char* tag, float score, const std::vector<bool>& in, const std::vector<float>& M) {
    int cnt = 0;
    for (size_t i = 0; i < in.size(); ++i) cnt += in[i] ? 1 : 0;
    std::printf("%s score=0x%08x inliers=%d m=", tag, bits(score), cnt);
    if (M.empty()) std::printf("empty");
    for (size_t k = 0; k < M.size(); ++k) std::printf("%s%08x", k ? " " : "", bits(M[k]));
    std::printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hdr[3];
    if (std::fread(hdr, 4, 3, f) != 3) return 2;
    const int n1 = hdr[0], n2 = hdr[1], n_hyp = hdr[2];
    std::vector<orb_keypoint_t> k1, k2;
    std::vector<int32_t> m12, draws;
    if (!rd(f, k1, n1) || !rd(f, k2, n2) || !rd(f, m12, n1) || !rd(f, draws, (size_t)n_hyp * 8)) return 2;
    std::fclose(f);
    try {
        ORB_SLAM::gpu::Initializer init(k1, 1.0f, n_hyp);
        const ORB_SLAM::gpu::Initializer::TwoViewModels r =
            init.Initialize(k2, std::vector<int>(m12.begin(), m12.end()), std::vector<int>(draws.begin(), draws.end()));
        if ((int)r.vbMatchesInliersH.size() != r.N || (int)r.vbMatchesInliersF.size() != r.N) std::printf("FAIL N\n");
        std::printf("N=%d useH=%d RH=0x%08x\n", r.N, r.bUseH ? 1 : 0, bits(r.RH));
        report("H", r.SH, r.vbMatchesInliersH, r.H);
        report("F", r.SF, r.vbMatchesInliersF, r.F);
        uint32_t sum = 0;
        for (size_t it = 0; it < r.mvSets.size(); ++it)
            for (size_t j = 0; j < 8; ++j) sum += (uint32_t)(it * 8 + j + 1) * (uint32_t)r.mvSets[it][j];
        std::printf("sets=%u\n", sum);
    } catch (const std::exception& e) {
        std::printf("FAIL exception: %s\n", e.what());
        return 2;
    }
    std::printf("initializer ransac facade OK\n");
    return 0;
}
