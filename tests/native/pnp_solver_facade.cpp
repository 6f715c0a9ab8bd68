// pnp_solver_facade.cpp — gpu::PnPsolver::iterate / find with the caller's rand() values
// (include/orb_slam_gpu.hpp) driven through the C ABI the way Tracking::Relocalisation drives
// iterate(5, ...) (reference src/Tracking.cc:961).  Input: a binary file written by
// tests/test_gpu_pnp_solver.py:
//   int32 nk, nlev, min_inliers, max_its, block, n_rand | 4 floats K |
//   nk x 28-byte keypoints | nlev floats levelSigma2 | nk u8 usable | nk x 3 floats worldPos |
//   n_rand x 4 int32 rand31
// One solver is driven `block` iterations at a time until it returns a pose or has no more; a second
// one runs find() on the same stream of values.  Output, one line per call:
//   ITER ok=<0|1> nomore=<0|1> its=<mnIterations> best=<mnBestInliers> n=<nInliers> flags=<set bits> hash=<fnv> used=<values>
//   FIND ok=.. its=.. best=.. n=.. flags=.. hash=..
//   TCW <12 floats as hex>     (after a call that returned a pose)
// and "pnp solver facade OK".  The test compares the lines with the CPU model's answer.
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

static void tcw(const float* T) {
    std::printf("TCW");
    for (int k = 0; k < 12; ++k) {
        uint32_t u;
        std::memcpy(&u, &T[k], 4);
        std::printf(" %08x", u);
    }
    std::printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hdr[6];
    float K[4];
    if (std::fread(hdr, 4, 6, f) != 6 || std::fread(K, 4, 4, f) != 4) return 2;
    const int nk = hdr[0], nlev = hdr[1], min_inliers = hdr[2], max_its = hdr[3], block = hdr[4], n_rand = hdr[5];
    std::vector<orb_keypoint_t> keys;
    std::vector<float> ls2, pos;
    std::vector<uint8_t> usable;
    std::vector<int32_t> rand31;
    if (!rd(f, keys, nk) || !rd(f, ls2, nlev) || !rd(f, usable, nk) || !rd(f, pos, (size_t)nk * 3) ||
        !rd(f, rand31, (size_t)n_rand * 4))
        return 2;
    std::fclose(f);
    try {
        ORB_SLAM::gpu::PnPsolver a(keys, ls2, usable, pos, K[0], K[1], K[2], K[3]);
        a.SetRansacParameters(0.99, min_inliers, max_its, 4, 0.5f, 5.991f);  // Tracking.cc:939
        std::printf("PNP N=%d min=%d maxits=%d\n", a.N, a.mRansacMinInliers, a.mRansacMaxIts);
        size_t at = 0;
        bool ok = false, bNoMore = false;
        int set;
        unsigned hash;
        float T[12];
        while (!ok && !bNoMore) {
            const std::vector<int32_t> r(rand31.begin() + at, rand31.end());
            std::vector<bool> vbInliers;
            int nInliers = 0;
            size_t used = 0;
            ok = a.iterate(block, bNoMore, vbInliers, nInliers, r, T, &used);
            at += used;
            digest(vbInliers, &set, &hash);
            std::printf("ITER ok=%d nomore=%d its=%d best=%d n=%d flags=%d hash=%08x used=%d\n", ok ? 1 : 0,
                        bNoMore ? 1 : 0, a.mnIterations, a.mnBestInliers, nInliers, set, hash, (int)used);
        }
        if (ok) tcw(T);
        ORB_SLAM::gpu::PnPsolver b(keys, ls2, usable, pos, K[0], K[1], K[2], K[3]);
        b.SetRansacParameters(0.99, min_inliers, max_its, 4, 0.5f, 5.991f);
        std::vector<bool> vbInliers;
        int nInliers = 0;
        ok = b.find(vbInliers, nInliers, rand31, T);
        digest(vbInliers, &set, &hash);
        std::printf("FIND ok=%d its=%d best=%d n=%d flags=%d hash=%08x\n", ok ? 1 : 0, b.mnIterations, b.mnBestInliers,
                    nInliers, set, hash);
        if (ok) tcw(T);
    } catch (const std::exception& e) {
        std::printf("FAIL exception: %s\n", e.what());
        return 2;
    }
    std::printf("pnp solver facade OK\n");
    return 0;
}
