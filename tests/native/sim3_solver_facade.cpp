// sim3_solver_facade.cpp — gpu::Sim3Solver::iterate / find with the caller's rand() values
// (include/orb_slam_gpu.hpp) driven through the C ABI the way LoopClosing::ComputeSim3 drives
// iterate(5, ...) (reference src/LoopClosing.cc:314).  Input: a binary file written by
// tests/test_gpu_sim3_solver.py:
//   int32 n, N1, min_inliers, max_its, block, n_rand | 4 floats K |
//   n x 3 floats x3Dc1 | x3Dc2 | n floats sigma2_1 | sigma2_2 | n int32 indices1 | n_rand x 3 int32 rand31
// One solver is driven `block` iterations at a time until it accepts or has no more; a second one
// runs find() on the same stream of values.  Output, one line per call:
//   ITER ok=<0|1> nomore=<0|1> its=<mnIterations> best=<mnBestInliers> n=<nInliers> flags=<set bits> hash=<fnv>
//   FIND ok=.. its=.. best=.. n=.. flags=.. hash=..
//   EST <13 floats as hex: R, t, s>     (after the loop and after find)
// and "sim3 solver facade OK".  The test compares the lines with the CPU model's answer.
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

static void estimate(const ORB_SLAM::gpu::Sim3Solver& s) {
    float e[13];
    std::memcpy(e, s.GetEstimatedRotation(), 36);
    std::memcpy(e + 9, s.GetEstimatedTranslation(), 12);
    e[12] = s.GetEstimatedScale();
    std::printf("EST");
    for (int k = 0; k < 13; ++k) {
        uint32_t u;
        std::memcpy(&u, &e[k], 4);
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
    const int n = hdr[0], N1 = hdr[1], min_inliers = hdr[2], max_its = hdr[3], block = hdr[4], n_rand = hdr[5];
    std::vector<float> x1, x2, s1, s2;
    std::vector<int32_t> idx1, rand31;
    if (!rd(f, x1, (size_t)n * 3) || !rd(f, x2, (size_t)n * 3) || !rd(f, s1, n) || !rd(f, s2, n) || !rd(f, idx1, n) ||
        !rd(f, rand31, (size_t)n_rand * 3))
        return 2;
    std::fclose(f);
    try {
        const std::vector<size_t> indices(idx1.begin(), idx1.end());
        ORB_SLAM::gpu::Sim3Solver a(x1, x2, s1, s2, indices, N1, K, K);
        a.SetRansacParameters(0.99, min_inliers, max_its);
        std::printf("SIM3 N=%d min=%d maxits=%d\n", a.N, a.mRansacMinInliers, a.mRansacMaxIts);
        size_t at = 0;
        bool ok = false, bNoMore = false;
        int set;
        unsigned hash;
        while (!ok && !bNoMore) {
            const std::vector<int32_t> r(rand31.begin() + at, rand31.end());
            std::vector<bool> vbInliers;
            int nInliers = 0;
            size_t used = 0;
            ok = a.iterate(block, bNoMore, vbInliers, nInliers, r, &used);
            at += used;
            digest(vbInliers, &set, &hash);
            std::printf("ITER ok=%d nomore=%d its=%d best=%d n=%d flags=%d hash=%08x\n", ok ? 1 : 0, bNoMore ? 1 : 0,
                        a.mnIterations, a.mnBestInliers, nInliers, set, hash);
        }
        estimate(a);
        ORB_SLAM::gpu::Sim3Solver b(x1, x2, s1, s2, indices, N1, K, K);
        b.SetRansacParameters(0.99, min_inliers, max_its);
        std::vector<bool> vbInliers;
        int nInliers = 0;
        ok = b.find(vbInliers, nInliers, rand31);
        digest(vbInliers, &set, &hash);
        std::printf("FIND ok=%d its=%d best=%d n=%d flags=%d hash=%08x\n", ok ? 1 : 0, b.mnIterations, b.mnBestInliers,
                    nInliers, set, hash);
        estimate(b);
    } catch (const std::exception& e) {
        std::printf("FAIL exception: %s\n", e.what());
        return 2;
    }
    std::printf("sim3 solver facade OK\n");
    return 0;
}
