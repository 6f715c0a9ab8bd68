// essential_graph_facade.cpp — gpu::Optimizer::OptimizeEssentialGraph (include/orb_slam_gpu.hpp) driven
// through the C ABI the way LoopClosing::CorrectLoop drives Optimizer::OptimizeEssentialGraph.  Input: a
// binary file written by tests/test_gpu_essential_graph.py:
//   int32 nk, ne, np, n_iterations | nk x 12 floats pose | nk u8 fixed | nk x 8 doubles corrected |
//   nk u8 has_corrected | nk x 8 doubles noncorrected | nk u8 has_noncorrected | ne int32 edge_i |
//   ne int32 edge_j | ne u8 kind | np x 3 floats pos | np int32 ref | np u8 skip
// Output:
//   ESSGRAPH free=<free vertices> iterations=<n> trials=<n> refused=<n> accepted=<the accept flags as 0 / 1>
//   SIM3 <fnv of the doubles of every estimate>  POSES <fnv of the float poses>  POINTS <likewise>
//   FROMPOSE <fnv of Sim3FromPose of every keyframe>  TOPOSE <fnv of PoseFromSim3 of every estimate>
// and "essential graph facade OK".  The test compares the lines with what the Python interface returns.
#include <cstdio>
#include <cstring>
#include <string>
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
    int32_t hdr[4];
    if (std::fread(hdr, 4, 4, f) != 4) return 2;
    const size_t nk = hdr[0], ne = hdr[1], np = hdr[2];
    ORB_SLAM::gpu::Optimizer::EssentialGraph G;
    if (!rd(f, G.kfPose, nk * 12) || !rd(f, G.kfFixed, nk) || !rd(f, G.kfCorrected, nk * 8) || !rd(f, G.kfHasCorrected, nk) ||
        !rd(f, G.kfNonCorrected, nk * 8) || !rd(f, G.kfHasNonCorrected, nk) || !rd(f, G.edgeI, ne) || !rd(f, G.edgeJ, ne) ||
        !rd(f, G.edgeKind, ne) || !rd(f, G.ptPos, np * 3) || !rd(f, G.ptRef, np) || !rd(f, G.ptSkip, np))
        return 2;
    std::fclose(f);
    try {
        ORB_SLAM::gpu::Optimizer::EssentialGraphResult R;
        ORB_SLAM::gpu::Optimizer::OptimizeEssentialGraph(G, R, hdr[3], 0);
        std::string acc;
        for (int k = 0; k < R.info.trials && k < ORB_EG_MAX_TRIALS; ++k) acc += R.info.trial_accepted[k] ? '1' : '0';
        std::printf("ESSGRAPH free=%d iterations=%d trials=%d refused=%d accepted=%s\n", R.info.n_free, R.info.iterations,
                    R.info.trials, R.info.refused, acc.c_str());
        std::printf("SIM3 %08x POSES %08x POINTS %08x\n", fnv(2166136261u, R.kfSim3.data(), R.kfSim3.size() * 8),
                    fnv(2166136261u, R.kfPose.data(), R.kfPose.size() * 4),
                    fnv(2166136261u, R.ptPos.data(), R.ptPos.size() * 4));
        unsigned hf = 2166136261u, ht = 2166136261u;
        for (size_t i = 0; i < nk; ++i) {
            const auto S = ORB_SLAM::gpu::Sim3FromPose(G.kfPose.data() + 12 * i);
            hf = fnv(hf, S.data(), 64);
            const auto T = ORB_SLAM::gpu::PoseFromSim3(R.kfSim3.data() + 8 * i);
            ht = fnv(ht, T.data(), 48);
        }
        std::printf("FROMPOSE %08x TOPOSE %08x\n", hf, ht);
    } catch (const std::exception& e) {
        std::printf("FAIL exception: %s\n", e.what());
        return 2;
    }
    std::printf("essential graph facade OK\n");
    return 0;
}
