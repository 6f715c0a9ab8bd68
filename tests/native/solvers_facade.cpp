// solvers_facade.cpp — gpu::PnPsolver and gpu::Sim3Solver (include/orb_slam_gpu.hpp) driven through
// the C ABI the way Tracking::Relocalisation and LoopClosing::ComputeSim3 drive iterate(5, ...)
// (reference src/Tracking.cc:961, src/LoopClosing.cc:314).  Input: a binary file written by
// tests/test_gpu_solvers.py:
//   int32 nk, nlev, n_hyp, block, pnp_min, n, N1, sim3_min | 4 floats K |
//   nk x 28-byte keypoints | nlev floats levelSigma2 | nk u8 usable | nk x 3 floats worldPos |
//   n_hyp x 9 doubles R | n_hyp x 3 doubles t |
//   n x 3 floats x3Dc1 | x3Dc2 | n floats sigma2_1 | sigma2_2 | n int32 indices1 |
//   n_hyp x 12 floats T12 | T21
// The hypotheses are handed over `block` at a time.  Output, one line per call:
//   PNP first=<index in block or -1> its=<mnIterations> best=<mnBestInliers> flags=<set bits> hash=<fnv of flags>
//   SIM3 first=<..> its=<..> best=<..> n=<nInliers> flags=<set bits of vbInliers> hash=<..>
// and "solvers facade OK".  The test compares the lines with the CPU model's answer.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/orb_slam_gpu.hpp"

template <class T>
static bool rd(std::FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

static void digest(const std::vector<bool>& v, int* set, unsigned* hash) {
    unsigned h = 2166136261u;
    int c = 0;
    for (size_t i = 0; i < v.size(); ++i) {
        h = (h ^ (v[i] ? 1u : 0u)) * 16777619u;
        c += v[i] ? 1 : 0;
    }
    *set = c;
    *hash = h;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hdr[8];
    float K[4];
    if (std::fread(hdr, 4, 8, f) != 8 || std::fread(K, 4, 4, f) != 4) return 2;
    const int nk = hdr[0], nlev = hdr[1], n_hyp = hdr[2], block = hdr[3], pnp_min = hdr[4], n = hdr[5], N1 = hdr[6],
              sim3_min = hdr[7];
    std::vector<orb_keypoint_t> keys;
    std::vector<float> ls2, pos, x1, x2, s1, s2, T12, T21;
    std::vector<uint8_t> usable;
    std::vector<double> R, t;
    std::vector<int32_t> idx1;
    if (!rd(f, keys, nk) || !rd(f, ls2, nlev) || !rd(f, usable, nk) || !rd(f, pos, (size_t)nk * 3) ||
        !rd(f, R, (size_t)n_hyp * 9) || !rd(f, t, (size_t)n_hyp * 3) || !rd(f, x1, (size_t)n * 3) ||
        !rd(f, x2, (size_t)n * 3) || !rd(f, s1, n) || !rd(f, s2, n) || !rd(f, idx1, n) ||
        !rd(f, T12, (size_t)n_hyp * 12) || !rd(f, T21, (size_t)n_hyp * 12))
        return 2;
    std::fclose(f);
    try {
        ORB_SLAM::gpu::PnPsolver pnp(keys, ls2, usable, pos, K[0], K[1], K[2], K[3]);
        pnp.SetRansacParameters(0.99, pnp_min, 300, 4, 0.5f, 5.991f);
        std::printf("PNP N=%d min=%d maxits=%d\n", pnp.N, pnp.mRansacMinInliers, pnp.mRansacMaxIts);
        for (int h0 = 0; h0 < n_hyp; h0 += block) {
            const int k = std::min(block, n_hyp - h0);
            const std::vector<double> vR(R.begin() + (size_t)h0 * 9, R.begin() + (size_t)(h0 + k) * 9);
            const std::vector<double> vt(t.begin() + (size_t)h0 * 3, t.begin() + (size_t)(h0 + k) * 3);
            const int first = pnp.iterate(vR, vt);
            int set;
            unsigned hash;
            digest(pnp.InliersByKeyPoint(pnp.mvbBestInliers), &set, &hash);
            std::printf("PNP first=%d its=%d best=%d flags=%d hash=%08x\n", first, pnp.mnIterations, pnp.mnBestInliers,
                        set, hash);
        }
        std::vector<bool> one;
        const int c0 = pnp.CheckInliers(R.data(), t.data(), one);
        int set;
        unsigned hash;
        digest(one, &set, &hash);
        std::printf("PNP refine count=%d flags=%d hash=%08x\n", c0, set, hash);

        ORB_SLAM::gpu::Sim3Solver sim3(x1, x2, s1, s2, std::vector<size_t>(idx1.begin(), idx1.end()), N1, K, K);
        sim3.SetRansacParameters(0.99, sim3_min, 300);
        std::printf("SIM3 N=%d min=%d maxits=%d\n", sim3.N, sim3.mRansacMinInliers, sim3.mRansacMaxIts);
        for (int h0 = 0; h0 < n_hyp; h0 += block) {
            const int k = std::min(block, n_hyp - h0);
            const std::vector<float> a(T12.begin() + (size_t)h0 * 12, T12.begin() + (size_t)(h0 + k) * 12);
            const std::vector<float> b(T21.begin() + (size_t)h0 * 12, T21.begin() + (size_t)(h0 + k) * 12);
            std::vector<bool> vbInliers;
            int nInliers = 0;
            const int first = sim3.iterate(a, b, vbInliers, nInliers);
            digest(vbInliers, &set, &hash);
            std::printf("SIM3 first=%d its=%d best=%d n=%d flags=%d hash=%08x\n", first, sim3.mnIterations,
                        sim3.mnBestInliers, nInliers, set, hash);
        }
    } catch (const std::exception& e) {
        std::printf("FAIL exception: %s\n", e.what());
        return 2;
    }
    std::printf("solvers facade OK\n");
    return 0;
}
