// local_mapping_facade.cpp — gpu::LocalMapping (include/orb_slam_gpu.hpp) driven through the C ABI the
// way LocalMapping::CreateNewMapPoints drives ComputeF12, the triangulation and UpdateNormalAndDepth.
// Input: a binary file written by tests/test_gpu_local_mapping.py:
//   int32 n1, n2, nlevels, M, R | 2 x (4 floats K4, 9 Rcw, 3 tcw, 3 Ow) | nlevels scale factors |
//   nlevels level sigma2 | n1 x 28-byte keypoints | n2 x 28-byte keypoints | n1 int32 match12 |
//   M + 1 int32 offsets | R x 3 floats obs_Ow | M x 3 pos | M x 3 ref_Ow | M int32 ref_level |
//   n2 x 3 floats mp_pos2 | n2 bytes has_mp2 (KF2's MapPoints, for the baseline gate)
// Output, floats as their bit patterns:
//   f12 <nine hex words>
//   create go=<0|1> n=<accepted> pairs=<checksum> x3d=<checksum> status=<checksum>
//   gated  go=<0|1> n=<accepted> x3d=<checksum>      (the same call with the baseline gate's inputs)
//   update normal=<checksum> dmin=<checksum> dmax=<checksum>
// where a checksum is the sum over elements k of (k + 1) * value (bits of a float) modulo 2^32, and
// "local mapping facade OK".  The test compares the lines with the Python path's.
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

static uint32_t fsum(const std::vector<float>& v) {
    uint32_t s = 0;
    for (size_t k = 0; k < v.size(); ++k) s += (uint32_t)(k + 1) * bits(v[k]);
    return s;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hdr[5];
    if (std::fread(hdr, 4, 5, f) != 5) return 2;
    const int n1 = hdr[0], n2 = hdr[1], nl = hdr[2], M = hdr[3], R = hdr[4];
    if (nl < 1 || nl > ORB_MAX_VIEW_LEVELS) return 2;
    float cam[2][19];
    std::vector<float> sf, s2, obs, pos, ref;
    std::vector<orb_keypoint_t> k1, k2;
    std::vector<int32_t> m12, off, lev;
    std::vector<uint8_t> has2;
    std::vector<float> pos2;
    if (std::fread(cam, 4, 38, f) != 38 || !rd(f, sf, nl) || !rd(f, s2, nl) || !rd(f, k1, n1) || !rd(f, k2, n2) ||
        !rd(f, m12, n1) || !rd(f, off, (size_t)M + 1) || !rd(f, obs, (size_t)R * 3) || !rd(f, pos, (size_t)M * 3) ||
        !rd(f, ref, (size_t)M * 3) || !rd(f, lev, M) || !rd(f, pos2, (size_t)n2 * 3) || !rd(f, has2, n2))
        return 2;
    std::fclose(f);
    orb_frame_view_t V[2];
    std::memset(V, 0, sizeof(V));
    for (int v = 0; v < 2; ++v) {
        V[v].kps = v ? k2.data() : k1.data();
        V[v].n = v ? n2 : n1;
        V[v].nlevels = nl;
        for (int k = 0; k < nl; ++k) V[v].scale_factors[k] = sf[k], V[v].level_sigma2[k] = s2[k];
        V[v].fx = cam[v][0], V[v].fy = cam[v][1], V[v].cx = cam[v][2], V[v].cy = cam[v][3];
        std::memcpy(V[v].Rcw, cam[v] + 4, 36);
        std::memcpy(V[v].tcw, cam[v] + 13, 12);
        std::memcpy(V[v].Ow, cam[v] + 16, 12);
    }
    try {
        float F12[9];
        ORB_SLAM::gpu::LocalMapping::ComputeF12(V[0], V[1], F12);
        std::printf("f12");
        for (int k = 0; k < 9; ++k) std::printf(" %08x", bits(F12[k]));
        std::printf("\n");
        std::vector<std::pair<int, int> > pairs;
        std::vector<float> x3d;
        std::vector<uint8_t> st;
        const bool go = ORB_SLAM::gpu::LocalMapping::CreateNewMapPoints(V[0], V[1], std::vector<int>(m12.begin(), m12.end()),
                                                                        nullptr, nullptr, pairs, x3d, &st);
        uint32_t ps = 0, ss = 0;
        for (size_t k = 0; k < pairs.size(); ++k)
            ps += (uint32_t)(2 * k + 1) * (uint32_t)pairs[k].first + (uint32_t)(2 * k + 2) * (uint32_t)pairs[k].second;
        for (size_t k = 0; k < st.size(); ++k) ss += (uint32_t)(k + 1) * st[k];
        std::printf("create go=%d n=%d pairs=%u x3d=%u status=%u\n", go ? 1 : 0, (int)pairs.size(), ps, fsum(x3d), ss);
        std::vector<std::pair<int, int> > gpairs;
        std::vector<float> gx3d;
        const bool ggo = ORB_SLAM::gpu::LocalMapping::CreateNewMapPoints(V[0], V[1], std::vector<int>(m12.begin(), m12.end()),
                                                                         pos2.data(), has2.data(), gpairs, gx3d);
        std::printf("gated go=%d n=%d x3d=%u\n", ggo ? 1 : 0, (int)gpairs.size(), fsum(gx3d));
        std::vector<float> normal, dmin, dmax;
        ORB_SLAM::gpu::LocalMapping::UpdateNormalAndDepth(off, obs, pos, ref, lev, sf, normal, dmin, dmax);
        std::printf("update normal=%u dmin=%u dmax=%u\n", fsum(normal), fsum(dmin), fsum(dmax));
    } catch (const std::exception& e) {
        std::printf("FAIL exception: %s\n", e.what());
        return 2;
    }
    std::printf("local mapping facade OK\n");
    return 0;
}
