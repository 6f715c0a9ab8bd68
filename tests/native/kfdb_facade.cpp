// kfdb_facade.cpp — gpu::KeyFrameDatabase (include/orb_slam_gpu.hpp) driven through the C ABI the
// way LoopClosing / Tracking drive the reference's KeyFrameDatabase, on scenarios whose answer
// is known by construction (tests/kfdb_cases.py states the same ones): the order of the sharing
// list, the stale reloc score of a covisible keyframe, the connected filter, and mpVoc->score.
// Exit status 0 and "kfdb facade OK" when every answer is the expected one.
#include <cstdio>
#include <map>
#include <vector>

#include "../../include/orb_slam_gpu.hpp"

using ORB_SLAM::gpu::BowVector;
typedef ORB_SLAM::gpu::KeyFrameDatabase DB;
typedef std::map<unsigned, double> Bow;  // DBoW2::BowVector
typedef std::vector<DB::Id> Ids;

static const double U = 1.0 / 1024.0;
static int failures = 0;

static void expect(const char* what, const Ids& got, const Ids& want) {
    if (got == want) return;
    ++failures;
    std::printf("FAIL %s: got", what);
    for (size_t i = 0; i < got.size(); ++i) std::printf(" %lu", got[i]);
    std::printf(", want");
    for (size_t i = 0; i < want.size(); ++i) std::printf(" %lu", want[i]);
    std::printf("\n");
}

static Bow words(int first, int last, double v) {
    Bow b;
    for (int w = first; w <= last; ++w) b[(unsigned)w] = v;
    return b;
}

int main() {
    const int nWords = 1000;
    std::vector<int32_t> parent(nWords, 0);
    std::vector<uint8_t> leaf(nWords, 1), desc((size_t)nWords * 32, 0);
    std::vector<double> weight(nWords, 1.0);
    orb_vocabulary_t* voc = nullptr;
    try {
        ORB_SLAM::gpu::orb_check(orb_vocabulary_create(10, 1, 0, 0, nWords, parent.data(), leaf.data(), desc.data(),
                                                      weight.data(), 0, &voc));
        {   // mpVoc->score
            Bow a, b;
            a[1] = 0.5, a[7] = 0.5, b[7] = 0.25, b[9] = 0.75;
            if (ORB_SLAM::gpu::score(voc, BowVector(a), BowVector(b)) != 0.25) {
                ++failures;
                std::printf("FAIL score\n");
            }
        }
        {   // list order: first shared word, then add order; a re-added keyframe goes last among its ties
            DB db(voc, 64, 4096);
            Bow q;
            q[10] = q[20] = q[30] = 1.0;
            db.add(7, BowVector(words(20, 20, 100 * U)));
            db.add(3, BowVector(words(30, 30, 100 * U)));
            db.add(5, BowVector(words(10, 10, 100 * U)));
            expect("order", db.DetectRelocalisationCandidates(BowVector(q)), Ids{5, 7, 3});
            db.add(9, BowVector(words(10, 10, 100 * U)));
            db.add(2, BowVector(words(10, 10, 100 * U)));
            expect("ties", db.DetectLoopCandidates(BowVector(q), Ids(), 0.0f), Ids{5, 9, 2, 7, 3});
            db.erase(5);
            db.add(5, BowVector(words(10, 10, 100 * U)));
            expect("re-add", db.DetectRelocalisationCandidates(BowVector(q)), Ids{9, 2, 5, 7, 3});
            if (db.size() != 5) ++failures, std::printf("FAIL size\n");
            db.clear();
            expect("clear", db.DetectRelocalisationCandidates(BowVector(q)), Ids());
        }
        {   // the stale score of a covisible keyframe, and the connected filter
            DB db(voc, 64, 4096);
            const DB::Id A = 1000000, B = 2000000, N = 3000000;
            db.add(A, BowVector(words(0, 4, 60 * U)));
            db.add(B, BowVector(words(0, 4, 80 * U)));
            Bow n;
            n[0] = U, n[100] = 1.0;
            db.add(N, BowVector(n));
            db.SetBestCovisibilityKeyFrames(A, Ids{N});
            const BowVector q2(words(0, 4, 1.0));
            expect("never scored", db.DetectRelocalisationCandidates(q2), Ids{B});
            expect("query 1", db.DetectRelocalisationCandidates(BowVector(words(100, 100, 900 * U))), Ids{N});
            expect("stale", db.DetectRelocalisationCandidates(q2), Ids{N});
            expect("loop", db.DetectLoopCandidates(q2, Ids(), 0.0f), Ids{B});
            expect("connected", db.DetectLoopCandidates(q2, Ids{B, 42}, 0.0f), Ids{A});
        }
        orb_vocabulary_destroy(voc);
    } catch (const std::exception& e) {
        std::printf("FAIL exception: %s\n", e.what());
        return 2;
    }
    if (failures) return 1;
    std::printf("kfdb facade OK\n");
    return 0;
}
