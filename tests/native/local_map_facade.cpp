// local_map_facade.cpp — gpu::LocalMap (include/orb_slam_gpu.hpp) driven through the C ABI the way
// Tracking::TrackLocalMap and LocalMapping drive UpdateReference and KeyFrame::UpdateConnections.  Input: a
// binary file written by tests/test_gpu_local_map_facade.py:
//   int32 nk, np, nkmp, nobs, nframe, K | nk u8 kf_bad | nk + 1 int32 kf_mp_off | nkmp int32 kf_mp |
//   nk x 10 int32 kf_cov | np u8 pt_bad | np + 1 int32 pt_obs_off | nobs int32 pt_obs_kf |
//   nframe int32 f_mp | K int32 keyframes
// Output:
//   REF ref=<kf> votes=<n> voted=<n> kfs=<n> pts=<n> cleared=<n>
//   LISTS <fnv of mvpMapPoints> <fnv of mvpLocalKeyFrames> <fnv of mvpLocalMapPoints> <fnv of seen>
//   CONN <keyframe> conn=<n> ord=<n> unchanged=<0 / 1> <fnv of connKF, connW, ordKF, ordW>   (one per keyframe)
// and "local map facade OK".  The test compares the lines with the model's results.
#include <cstdio>
#include <vector>

#include "../../include/orb_slam_gpu.hpp"

template <class T>
static bool rd(std::FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

template <class T>
static unsigned fnv(unsigned h, const std::vector<T>& v) {
    const unsigned char* b = (const unsigned char*)v.data();
    for (size_t i = 0; i < v.size() * sizeof(T); ++i) h = (h ^ b[i]) * 16777619u;
    return h;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hdr[6];
    if (std::fread(hdr, 4, 6, f) != 6) return 2;
    const size_t nk = hdr[0], np = hdr[1];
    ORB_SLAM::gpu::LocalMap::Tables T;
    std::vector<int32_t> frame, kfs;
    if (!rd(f, T.kfBad, nk) || !rd(f, T.kfMpOff, nk + 1) || !rd(f, T.kfMp, hdr[2]) || !rd(f, T.kfCov, nk * 10) ||
        !rd(f, T.ptBad, np) || !rd(f, T.ptObsOff, np + 1) || !rd(f, T.ptObsKf, hdr[3]) || !rd(f, frame, hdr[4]) ||
        !rd(f, kfs, hdr[5]))
        return 2;
    std::fclose(f);
    const unsigned H0 = 2166136261u;
    try {
        ORB_SLAM::gpu::LocalMap::Reference R;
        ORB_SLAM::gpu::LocalMap::UpdateReference(T, frame, R, 0);
        std::printf("REF ref=%d votes=%d voted=%d kfs=%d pts=%d cleared=%d\n", R.info.ref_kf, R.info.ref_votes, R.info.n_voted,
                    (int)R.vpLocalKeyFrames.size(), (int)R.vpLocalMapPoints.size(), R.info.n_cleared);
        std::printf("LISTS %08x %08x %08x %08x\n", fnv(H0, R.vpMapPoints), fnv(H0, R.vpLocalKeyFrames),
                    fnv(H0, R.vpLocalMapPoints), fnv(H0, R.vbSeen));
        std::vector<ORB_SLAM::gpu::LocalMap::Connections> C;
        ORB_SLAM::gpu::LocalMap::UpdateConnections(T, kfs, C, 0);
        for (size_t q = 0; q < C.size(); ++q)
            std::printf("CONN %d conn=%d ord=%d unchanged=%d %08x\n", kfs[q], (int)C[q].connKF.size(), (int)C[q].ordKF.size(),
                        C[q].unchanged ? 1 : 0, fnv(fnv(fnv(fnv(H0, C[q].connKF), C[q].connW), C[q].ordKF), C[q].ordW));
    } catch (const std::exception& e) {
        std::printf("FAIL exception: %s\n", e.what());
        return 2;
    }
    std::printf("local map facade OK\n");
    return 0;
}
