// initializer_reconstruct_facade.cpp — gpu::Initializer::Initialize (the whole of it), ReconstructH
// and ReconstructF (include/orb_slam_gpu.hpp) driven through the C ABI the way Tracking drives
// Initializer::Initialize.  Input: a binary file written by tests/test_gpu_initializer_reconstruct.py:
//   int32 n1, n2, n_hyp, use_h | 4 floats K4 | 9 floats model | n1 x 28-byte keypoints |
//   n2 x 28-byte keypoints | n1 int32 matches12 | n1 mask bytes (N used) | n_hyp x 8 int32 draws
// Output, floats as their bit patterns:
//   reconstruct ok=<0|1> R=<nine hex words or "empty"> t=<three or "empty"> tri=<count> p3d=<checksum>
//   initialize  ok=... (the same)
// where the checksum is the sum over keys i and axes c of (3 i + c + 1) * bits(vP3D[i][c]) modulo
// 2^32, and "initializer reconstruct facade OK".  The test compares the lines with the CPU model's.
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

static void report(const char* tag, bool ok, const std::vector<float>& R, const std::vector<float>& t,
                   const std::vector<float>& P, const std::vector<bool>& tri) {
    std::printf("%s ok=%d R=", tag, ok ? 1 : 0);
    if (R.empty()) std::printf("empty");
    for (size_t k = 0; k < R.size(); ++k) std::printf("%s%08x", k ? " " : "", bits(R[k]));
    std::printf(" t=");
    if (t.empty()) std::printf("empty");
    for (size_t k = 0; k < t.size(); ++k) std::printf("%s%08x", k ? " " : "", bits(t[k]));
    int cnt = 0;
    for (size_t i = 0; i < tri.size(); ++i) cnt += tri[i] ? 1 : 0;
    uint32_t sum = 0;
    for (size_t k = 0; k < P.size(); ++k) sum += (uint32_t)(k + 1) * bits(P[k]);
    std::printf(" tri=%d p3d=%u\n", cnt, sum);
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hdr[4];
    float K4[4];
    std::vector<float> M;
    if (std::fread(hdr, 4, 4, f) != 4 || std::fread(K4, 4, 4, f) != 4 || !rd(f, M, 9)) return 2;
    const int n1 = hdr[0], n2 = hdr[1], n_hyp = hdr[2], use_h = hdr[3];
    std::vector<orb_keypoint_t> k1, k2;
    std::vector<int32_t> m12, draws;
    std::vector<uint8_t> mask;
    if (!rd(f, k1, n1) || !rd(f, k2, n2) || !rd(f, m12, n1) || !rd(f, mask, n1) || !rd(f, draws, (size_t)n_hyp * 8)) return 2;
    std::fclose(f);
    try {
        ORB_SLAM::gpu::Initializer init(k1, 1.0f, n_hyp);
        const std::vector<int> vm(m12.begin(), m12.end());
        const int N = init.SetMatches(k2, vm);
        std::vector<bool> in((size_t)N);
        for (int i = 0; i < N; ++i) in[(size_t)i] = mask[(size_t)i] != 0;
        std::vector<float> R, t, P;
        std::vector<bool> tri;
        const bool ok = use_h ? init.ReconstructH(in, M, K4, R, t, P, tri) : init.ReconstructF(in, M, K4, R, t, P, tri);
        report("reconstruct", ok, R, t, P, tri);
        std::vector<float> R2, t2, P2;
        std::vector<bool> tri2;
        const bool ok2 = init.Initialize(k2, vm, std::vector<int>(draws.begin(), draws.end()), K4, R2, t2, P2, tri2);
        report("initialize", ok2, R2, t2, P2, tri2);
    } catch (const std::exception& e) {
        std::printf("FAIL exception: %s\n", e.what());
        return 2;
    }
    std::printf("initializer reconstruct facade OK\n");
    return 0;
}
