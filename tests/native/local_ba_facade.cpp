// local_ba_facade.cpp — gpu::Optimizer::LocalBundleAdjustment (include/orb_slam_gpu.hpp) driven through
// the C ABI the way LocalMapping::Run drives Optimizer::LocalBundleAdjustment and then mutates the map
// (reference src/Optimizer.cc:453-535).  Input: a binary file written by tests/test_gpu_local_ba.py:
//   int32 nk, np, ne | nk x 12 floats pose | nk x 4 floats K | nk u8 fixed | np x 3 floats pos |
//   np int32 nobs | ne int32 edge_pt | ne int32 edge_kf | ne x 2 floats obs | ne floats invSigma2
// Output:
//   LOCALBA erased1=<edges erased after round 1> erased2=<after round 2> bad=<points gone bad>
//           hash=<fnv of edge_erased then pt_bad> iterations=<round 1>,<round 2>
//   WALK bad=<points that SetBadFlag reaches when edge_erased is walked in edge order with
//           EraseObservation's count> (must equal bad: the flags carry the reference's map mutation)
//   POSES <fnv of the float bit patterns of every pose>   POINTS <likewise>
// and "local BA facade OK".  The test compares the lines with the CPU model's answer.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/orb_slam_gpu.hpp"

template <class T>
static bool rd(std::FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

static unsigned fnv(unsigned h, const void* p, size_t n) {
    const unsigned char* b = (const unsigned char*)p;
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 16777619u;
    return h;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hdr[3];
    if (std::fread(hdr, 4, 3, f) != 3) return 2;
    const size_t nk = hdr[0], np = hdr[1], ne = hdr[2];
    ORB_SLAM::gpu::Optimizer::LocalBAGraph G;
    if (!rd(f, G.kfPose, nk * 12) || !rd(f, G.kfK, nk * 4) || !rd(f, G.kfFixed, nk) || !rd(f, G.ptPos, np * 3) ||
        !rd(f, G.ptNObs, np) || !rd(f, G.edgePt, ne) || !rd(f, G.edgeKf, ne) || !rd(f, G.edgeObs, ne * 2) ||
        !rd(f, G.edgeInvSigma2, ne))
        return 2;
    std::fclose(f);
    try {
        ORB_SLAM::gpu::Optimizer::LocalBAResult R;
        ORB_SLAM::gpu::Optimizer::LocalBundleAdjustment(G, R, 0);
        int er[3] = {0, 0, 0}, bad = 0;
        for (size_t e = 0; e < ne; ++e) ++er[R.edgeErased[e] < 3 ? R.edgeErased[e] : 0];
        for (size_t p = 0; p < np; ++p) bad += R.ptBad[p] ? 1 : 0;
        unsigned h = fnv(2166136261u, R.edgeErased.data(), ne);
        h = fnv(h, R.ptBad.data(), np);
        std::printf("LOCALBA erased1=%d erased2=%d bad=%d hash=%08x iterations=%d,%d\n", er[1], er[2], bad, h,
                    R.info.round[0].iterations, R.info.round[1].iterations);
        // the caller's walk: pKFi->EraseMapPointMatch(pMP); pMP->EraseObservation(pKFi) per flagged edge
        std::vector<int32_t> nobs = G.ptNObs;
        std::vector<uint8_t> isBad(np, 0);
        int walkBad = 0;
        for (size_t e = 0; e < ne; ++e)
            if (R.edgeErased[e] && !isBad[G.edgePt[e]] && --nobs[G.edgePt[e]] <= 2) isBad[G.edgePt[e]] = 1, ++walkBad;
        std::printf("WALK bad=%d\n", walkBad);
        std::printf("POSES %08x POINTS %08x\n", fnv(2166136261u, R.kfPose.data(), R.kfPose.size() * 4),
                    fnv(2166136261u, R.ptPos.data(), R.ptPos.size() * 4));
    } catch (const std::exception& e) {
        std::printf("FAIL exception: %s\n", e.what());
        return 2;
    }
    std::printf("local BA facade OK\n");
    return 0;
}
