// staging_host.cpp — csrc/orb_staging.h and csrc/orb_initializer_scratch.h as plain C++
// (build/libstaging_host.so, tests/test_staging_host.py; with -DSTAGING_HOST_MAIN a program that runs
// every check, which is what the sanitizer run executes).
//
// Each staging_check_*() returns 0, or the line of the first expectation that did not hold.
// "Before" below means the hand-written offset chains these headers replaced: they are restated here
// as they stood, with an alignment function of this file's own, and the plans next to them repeat the
// declarations of the entry points.
//
// A pointer cannot be asked for before the arena is reserved: that does not compile.  A plan has no
// accessor that gives one and a stage cannot be made without its memory (the static_asserts below).
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/orb_abi.h"
#include "../../orbslam_jpminipc_amd/csrc/orb_initializer_scratch.h"
#include "../../orbslam_jpminipc_amd/csrc/orb_staging.h"

namespace {

#define EXPECT(c)                  \
    do {                           \
        if (!(c)) return __LINE__; \
    } while (0)

size_t al(size_t x) { return (x + 255) / 256 * 256; }  // (not the header's expression)

template <class P, class = void>
struct gives_dev : std::false_type {};
template <class P>
struct gives_dev<P, std::void_t<decltype(std::declval<const P&>().dev(OrbRegion<float>{}))>> : std::true_type {};
template <class P, class = void>
struct gives_host : std::false_type {};
template <class P>
struct gives_host<P, std::void_t<decltype(std::declval<const P&>().host(OrbRegion<float>{}))>> : std::true_type {};
static_assert(gives_dev<OrbStage>::value && gives_host<OrbStage>::value, "the detector sees an accessor that exists");
static_assert(!gives_dev<OrbStagePlan>::value && !gives_host<OrbStagePlan>::value, "a plan gives no pointer");
static_assert(!std::is_default_constructible<OrbStage>::value, "no stage without the memory reserved for its plan");

const size_t SIZES[5] = {0, 1, 255, 256, 257};

struct Spans {
    size_t in_end, out_end, total;
};
Spans spans(const OrbStagePlan& P) { return {P.in_end(), P.out_end(), P.total()}; }
bool same(const Spans& a, size_t in_end, size_t out_end, size_t total) {
    return a.in_end == in_end && a.out_end == out_end && a.total == total;
}

// the kernels' argument structs, reduced to what the region functions fill
struct TestHyp {
    int32_t *ord_i, *nmatch;
    float *norm, *H21, *H12, *F21;
};
struct TestInit {
    float* scores[2];
    int32_t* best[2];
    float* best_score[2];
};
struct TestRec {
    int32_t *ord_i, *nwalk;
    uint8_t* flags;
    float* cosv;
    int32_t *n_motion, *n_inliers, *best;
    float *motion_R, *motion_t;
    int32_t* n_good;
    float *cos_sel, *parallax;
};

struct Piece {  // one array a chain uses: where it is, how long, and the caller's array if it gave one
    const void* p;
    size_t bytes;
    const void* given;
    bool needed;
};

// Every needed piece is the caller's array, or lies inside [base, base + size) and meets no other.
int pieces_ok(std::vector<Piece> v, const uint8_t* base, size_t size) {
    std::vector<std::pair<const uint8_t*, size_t>> carved;
    for (const Piece& x : v) {
        if (x.given) {
            EXPECT(x.p == x.given);
        } else if (!x.needed) {
            EXPECT(x.p == nullptr);
        } else {
            const uint8_t* q = (const uint8_t*)x.p;
            EXPECT(q >= base && q + x.bytes <= base + size && (size_t)(q - base) % 256 == 0);
            carved.push_back({q, x.bytes});
        }
    }
    std::sort(carved.begin(), carved.end());
    for (size_t k = 1; k < carved.size(); ++k) EXPECT(carved[k - 1].first + carved[k - 1].second <= carved[k].first);
    return 0;
}

}  // namespace

extern "C" {

// off[0..3]: the offsets of four regions of bytes[0..3] taken in order; off[4]: the block's size.
void staging_offsets4(const size_t* bytes, size_t* off) {
    OrbLayout L;
    for (int k = 0; k < 4; ++k) off[k] = L.add(bytes[k]);
    off[4] = L.end;
}

int staging_check_chain4() {
    std::vector<uint8_t> block(4 * 512);
    for (size_t a : SIZES)
        for (size_t b : SIZES)
            for (size_t c : SIZES)
                for (size_t d : SIZES) {
                    const size_t o0 = 0, o1 = al(o0 + a), o2 = al(o1 + b), o3 = al(o2 + c), end = al(o3 + d);
                    const size_t bytes[4] = {a, b, c, d};
                    size_t off[5];
                    staging_offsets4(bytes, off);
                    EXPECT(off[0] == o0 && off[1] == o1 && off[2] == o2 && off[3] == o3 && off[4] == end);
                    EXPECT(a || o1 == o0);  // a region of no bytes occupies nothing
                    // the pointer pass gives the same offsets, the sizing pass no pointer
                    OrbLayout L(block.data()), S;
                    EXPECT(end <= block.size());
                    EXPECT(L.take<uint8_t>(a) == block.data() + o0 && L.take<uint8_t>(b) == block.data() + o1);
                    EXPECT(L.take<uint8_t>(c) == block.data() + o2 && L.take<uint8_t>(d) == block.data() + o3);
                    EXPECT(S.take<uint8_t>(a) == nullptr && L.end == end);
                    EXPECT(orb_layout_size([&](OrbLayout& Z) { Z.add(a), Z.add(b), Z.add(c), Z.add(d); }) == end);
                    // a plan: in, in, out, scratch
                    OrbStagePlan P;
                    const auto r0 = P.in<uint8_t>(a), r1 = P.in<uint8_t>(b), r2 = P.out<uint8_t>(c), r3 = P.scratch<uint8_t>(d);
                    EXPECT(r0.off == o0 && r1.off == o1 && r2.off == o2 && r3.off == o3);
                    EXPECT(same(spans(P), o2, o3, end));
                }
    // typed counts are bytes / sizeof
    OrbLayout S;
    S.take<double>(3), S.take<uint8_t>(0);
    EXPECT(S.end == 256 && S.take<int32_t>(65) == nullptr && S.end == 256 + 512);
    return 0;
}

// One case of every ported entry point: the plan as the entry point declares it against the chain it
// had before.
int staging_check_cases() {
    const int n = 130, n_hyp = 65, cap = n, W = (n + 63) / 64;
    const size_t N = n, nh = n_hyp;
    {  // orb_pose_optimization
        const int NV = 7;
        const size_t oP = 0, oO = al(oP + N * 12), oS = al(oO + N * 8), oH = al(oS + N * 4), oT = al(oH + N),
                     in_end = al(oT + 48);
        const size_t o64 = in_end, oI = al(o64 + 96), o32 = al(oI + sizeof(orb_pose_opt_info_t)), oN = al(o32 + 48),
                     oF = al(oN + 4), out_end = al(oF + (size_t)cap);
        const size_t oSoa = out_end, oIdx = al(oSoa + (size_t)NV * cap * 8), oCnt = al(oIdx + (size_t)cap * 4),
                     total = al(oCnt + 4);
        OrbStagePlan P;
        P.in<float>(N * 3), P.in<float>(N * 2), P.in<float>(N), P.in<uint8_t>(N), P.in<float>(12);
        const auto r64 = P.out<double>(12);
        P.out<orb_pose_opt_info_t>(1), P.out<float>(12), P.out<int32_t>(1);
        const auto rF = P.out<uint8_t>(cap);
        P.scratch<double>((size_t)NV * cap), P.scratch<int32_t>(cap);
        const auto rCnt = P.scratch<int32_t>(1);
        EXPECT(same(spans(P), in_end, out_end, total) && r64.off == o64 && rF.off == oF && rCnt.off == oCnt);
    }
    {  // orb_optimize_sim3
        const int NV = 14;
        const size_t oX1 = 0, oX2 = al(oX1 + N * 12), oO1 = al(oX2 + N * 12), oO2 = al(oO1 + N * 8), oW1 = al(oO2 + N * 8),
                     oW2 = al(oW1 + N * 4), oU = al(oW2 + N * 4), oT = al(oU + N), in_end = al(oT + 52);
        const size_t o64 = in_end, oI = al(o64 + 64), o32 = al(oI + sizeof(orb_sim3_opt_info_t)), oN = al(o32 + 52),
                     oK = al(oN + 4), out_end = al(oK + (size_t)cap);
        const size_t oSoa = out_end, oIdx = al(oSoa + (size_t)NV * cap * 8), oCnt = al(oIdx + (size_t)cap * 4),
                     total = al(oCnt + 4);
        OrbStagePlan P;
        P.in<float>(N * 3), P.in<float>(N * 3), P.in<float>(N * 2), P.in<float>(N * 2), P.in<float>(N), P.in<float>(N);
        P.in<uint8_t>(N);
        const auto rT = P.in<float>(13);
        P.out<double>(8), P.out<orb_sim3_opt_info_t>(1), P.out<float>(13), P.out<int32_t>(1);
        const auto rK = P.out<uint8_t>(cap);
        P.scratch<double>((size_t)NV * cap), P.scratch<int32_t>(cap), P.scratch<int32_t>(1);
        EXPECT(same(spans(P), in_end, out_end, total) && rT.off == oT && rK.off == oK);
    }
    for (int model = 0; model < 2; ++model) {  // run_host<PNP, double>, run_host<SIM3, float>
        const int NV = model == 0 ? 6 : 12;  // NV_PNP, NV_SIM3
        const size_t in_bytes[2][6] = {{N * 12, N * 8, N * 4, 0, nh * 72, nh * 24}, {N * 12, N * 12, N * 4, N * 4, nh * 48, nh * 48}};
        size_t o_in[7], off = 0;
        for (int k = 0; k < 6; ++k) {
            o_in[k] = off;
            off = al(off + in_bytes[model][k]);
        }
        o_in[6] = off;
        const size_t in_end = al(off + 4);
        const size_t oC = in_end, oB = al(oC + nh * 4), oF = al(oB + nh * 4), oM = al(oF + 8),
                     out_end = al(oM + nh * W * 8), total = al(out_end + (size_t)NV * cap * 4);
        OrbStagePlan P;
        OrbRegion<uint8_t> rIn[6];
        for (int k = 0; k < 6; ++k) rIn[k] = P.in<uint8_t>(in_bytes[model][k]);
        const auto rBest = P.in<int32_t>(1);
        P.out<int32_t>(nh), P.out<int32_t>(nh), P.out<int32_t>(2);
        const auto rM = P.out<uint64_t>(nh * W);
        const auto rSoa = P.scratch<float>((size_t)NV * cap);
        for (int k = 0; k < 6; ++k) EXPECT(rIn[k].off == o_in[k]);
        EXPECT(same(spans(P), in_end, out_end, total) && rBest.off == o_in[6] && rM.off == oM && rSoa.off == out_end);
    }
    {  // run_host_sim3
        const int NV = 12;  // NV_SIM3
        const size_t o1 = 0, o2 = al(o1 + N * 12), o3 = al(o2 + N * 12), o4 = al(o3 + N * 4), oD = al(o4 + N * 4),
                     oI = al(oD + nh * 12), in_end = al(oI + 4);
        const size_t oC = in_end, oB = al(oC + nh * 4), oF = al(oB + nh * 4), oT12 = al(oF + 8), oT21 = al(oT12 + nh * 48),
                     oS = al(oT21 + nh * 48), oQ = al(oS + nh * 52), oSet = al(oQ + nh * 16), oA = al(oSet + nh * 12),
                     oM = al(oA + 52), out_end = al(oM + nh * W * 8), total = al(out_end + (size_t)NV * cap * 4);
        OrbStagePlan P;
        P.in<float>(N * 3), P.in<float>(N * 3), P.in<float>(N), P.in<float>(N), P.in<int32_t>(nh * 3), P.in<int32_t>(1);
        P.out<int32_t>(nh), P.out<int32_t>(nh), P.out<int32_t>(2);
        P.out<float>(nh * 12), P.out<float>(nh * 12), P.out<float>(nh * 13), P.out<float>(nh * 4), P.out<int32_t>(nh * 3);
        const auto rA = P.out<float>(13);
        const auto rM = P.out<uint64_t>(nh * W);
        P.scratch<float>((size_t)NV * cap);
        EXPECT(same(spans(P), in_end, out_end, total) && rA.off == oA && rM.off == oM);
    }
    for (int n_sel : {0, 7}) {  // run_host_pnp: the hypotheses / the iterate, and compute_pose_n
        const int NV = 6;
        const size_t h = n_sel ? 1 : nh;
        const size_t o1 = 0, o2 = al(o1 + N * 12), o3 = al(o2 + N * 8), oD = al(o3 + N * 4), oL = al(oD + h * 16),
                     oI = al(oL + (size_t)n_sel * 4), in_end = al(oI + 4);
        const size_t oC = in_end, oB = al(oC + h * 4), oF = al(oB + h * 4), oR = al(oF + 8), oT = al(oR + h * 72),
                     oE = al(oT + h * 24), oSet = al(oE + h * 8), oRC = al(oSet + h * 16), oFR = al(oRC + h * 4),
                     oP = al(oFR + 8), oPM = al(oP + 48), oM = al(oPM + (size_t)W * 8), out_end = al(oM + h * W * 8);
        const size_t oRR = out_end, oRT = al(oRR + h * 72), oRM = al(oRT + h * 24), oSoa = al(oRM + h * W * 8),
                     total = al(oSoa + (size_t)NV * cap * 4);
        OrbStagePlan P;
        P.in<float>(N * 3), P.in<float>(N * 2), P.in<float>(N), P.in<int32_t>(h * 4);
        const auto rL = P.in<int32_t>(n_sel);
        P.in<int32_t>(1);
        P.out<int32_t>(h), P.out<int32_t>(h), P.out<int32_t>(2);
        P.out<double>(h * 9), P.out<double>(h * 3), P.out<double>(h), P.out<int32_t>(h * 4), P.out<int32_t>(h);
        const auto rFR = P.out<int32_t>(2);
        P.out<float>(12);
        const auto rPM = P.out<uint64_t>(W), rM = P.out<uint64_t>(h * W);
        P.scratch<double>(h * 9), P.scratch<double>(h * 3);
        const auto rRM = P.scratch<uint64_t>(h * W);
        const auto rSoa = P.scratch<float>((size_t)NV * cap);
        EXPECT(same(spans(P), in_end, out_end, total));
        EXPECT(rL.off == oL && rFR.off == oFR && rPM.off == oPM && rM.off == oM && rRM.off == oRM && rSoa.off == oSoa);
    }
    const int n1 = 70, n2 = 130, icap = std::max(n1, n2);
    const size_t kp = sizeof(orb_keypoint_t);
    {  // orb_initializer_check
        const size_t hyp = nh * 9 * sizeof(float);
        const size_t oK = 0, oC = al(oK + 2 * (size_t)icap * kp), oM = al(oC + 16), oH21 = al(oM + (size_t)icap * 4),
                     oH12 = al(oH21 + hyp), oF = al(oH12 + hyp), in_end = al(oF + hyp);
        const size_t oS = in_end, oB = al(oS + 2 * nh * 4), oI = al(oB + 20), total = al(oI + 2 * (size_t)icap);
        OrbStagePlan P;
        P.in<orb_keypoint_t>(2 * (size_t)icap), P.in<int32_t>(4), P.in<int32_t>(icap);
        P.in<float>(nh * 9), P.in<float>(nh * 9);
        const auto rF = P.in<float>(nh * 9);
        P.out<float>(2 * nh), P.out<int32_t>(5);
        const auto rI = P.out<uint8_t>(2 * (size_t)icap);
        EXPECT(same(spans(P), in_end, total, total) && rF.off == oF && rI.off == oI);
    }
    {  // host_run (orb_initializer_ransac): the chain's scratch at its most
        const int P1 = 1;
        const size_t chyp = al((size_t)P1 * n_hyp * 9 * 4);
        const size_t chain_scratch_bytes = al((size_t)P1 * icap * 4) + al((size_t)P1 * 4) + al((size_t)P1 * 2 * 16 * 4) +
                                           3 * chyp + 2 * al((size_t)P1 * n_hyp * 4) + 4 * al((size_t)P1 * 4);
        const size_t hyp = al(nh * 9 * 4);
        const size_t oK = 0, oC = al(oK + 2 * (size_t)icap * kp), oM = al(oC + 16), oD = al(oM + (size_t)icap * 4),
                     in_end = al(oD + nh * 32);
        const size_t oH = in_end, oSet = oH + 5 * hyp, oN = al(oSet + nh * 32), oS = al(oN + 2 * 16 * 4),
                     oB = al(oS + 2 * nh * 4), oBH = al(oB + 28), oI = al(oBH + 72), out_end = al(oI + 2 * (size_t)icap);
        OrbLayout most;
        TestHyp h{};
        TestInit a{};
        chain_regions(most, ChainOut{}, true, icap, 1, n_hyp, h, a);
        OrbStagePlan P;
        P.in<orb_keypoint_t>(2 * (size_t)icap), P.in<int32_t>(4), P.in<int32_t>(icap), P.in<int32_t>(nh * 8);
        for (int k = 0; k < 5; ++k) P.out<float>(nh * 9);
        const auto rSet = P.out<int32_t>(nh * 8);
        P.out<float>(2 * HY_NORM), P.out<float>(2 * nh);
        const auto rB = P.out<int32_t>(7);
        P.out<float>(18);
        const auto rI = P.out<uint8_t>(2 * (size_t)icap);
        P.scratch<uint8_t>(most.end);
        EXPECT(same(spans(P), in_end, out_end, out_end + chain_scratch_bytes));
        EXPECT(rSet.off == oSet && rB.off == oB && rI.off == oI);
    }
    {  // orb_initializer_reconstruct
        const size_t pc = icap;
        const size_t rec_scratch_bytes = al(pc * 4) + al(4) + al(pc * 8) + al(pc * 8 * 4) + 3 * al(4) + al(72 * 4) +
                                         al(24 * 4) + 3 * al(8 * 4);
        const size_t oK = 0, oC = al(oK + 2 * (size_t)icap * kp), oM = al(oC + 20), oMod = al(oM + (size_t)icap * 4),
                     oI = al(oMod + 36), in_end = al(oI + (size_t)icap);
        const size_t oS = in_end, oR = al(oS + 16), oMR = al(oR + 48), oMT = al(oMR + 288), oG = al(oMT + 96),
                     oCs = al(oG + 32), oPa = al(oCs + 32), oP = al(oPa + 32), oT = al(oP + (size_t)icap * 12),
                     out_end = al(oT + (size_t)icap);
        OrbLayout most;
        TestRec a{};
        rec_regions(most, RecOut{}, icap, 1, a);
        OrbStagePlan P;
        P.in<orb_keypoint_t>(2 * (size_t)icap), P.in<int32_t>(5), P.in<int32_t>(icap), P.in<float>(9);
        const auto rI = P.in<uint8_t>(icap);
        P.out<int32_t>(4), P.out<float>(12), P.out<float>(72), P.out<float>(24), P.out<int32_t>(8), P.out<float>(8);
        P.out<float>(8);
        const auto rP = P.out<float>((size_t)icap * 3);
        const auto rT = P.out<uint8_t>(icap);
        P.scratch<uint8_t>(most.end);
        EXPECT(same(spans(P), in_end, out_end, out_end + rec_scratch_bytes));
        EXPECT(rI.off == oI && rP.off == oP && rT.off == oT && oS == in_end);
    }
    return 0;
}

// run_chain: for every subset of the outputs the caller may give, with and without the scoring, the
// sizing pass ends where the pointer pass ends, inside what no subset exceeds, and the arrays carved
// meet neither each other nor the end.
int staging_check_chain_subsets() {
    const int cap = 130, P = 3, n_hyp = 65;
    const size_t p = P, hyp = p * n_hyp * 9 * 4;
    static float gf[8];
    static int32_t gi[4];
    for (int score = 0; score < 2; ++score) {
        OrbLayout most;
        TestHyp h0{};
        TestInit a0{};
        chain_regions(most, ChainOut{}, score, cap, P, n_hyp, h0, a0);
        std::vector<uint8_t> block(most.end);
        for (unsigned m = 0; m < (1u << 11); ++m) {
            ChainOut o{};
            if (m & 1) o.n_matches = gi;
            if (m & 2) o.norm = gf;
            if (m & 4) o.H21 = gf + 1;
            if (m & 8) o.H12 = gf + 2;
            if (m & 16) o.F21 = gf + 3;
            if (m & 32) o.scores_h = gf + 4;
            if (m & 64) o.scores_f = gf + 5;
            if (m & 128) o.best_h = gi + 1;
            if (m & 256) o.best_f = gi + 2;
            if (m & 512) o.best_score_h = gf + 6;
            if (m & 1024) o.best_score_f = gf + 7;
            OrbLayout size, L(block.data());
            TestHyp hs{}, h{};
            TestInit as{}, a{};
            chain_regions(size, o, score, cap, P, n_hyp, hs, as);
            chain_regions(L, o, score, cap, P, n_hyp, h, a);
            EXPECT(size.end == L.end && L.end <= most.end);
            const bool s = score;
            if (int line = pieces_ok({{h.ord_i, p * cap * 4, nullptr, true},
                                      {h.nmatch, p * 4, o.n_matches, true},
                                      {h.norm, p * 2 * HY_NORM * 4, o.norm, true},
                                      {h.H21, hyp, o.H21, s},
                                      {h.H12, hyp, o.H12, s},
                                      {h.F21, hyp, o.F21, s},
                                      {a.scores[0], p * n_hyp * 4, s ? o.scores_h : nullptr, s},
                                      {a.scores[1], p * n_hyp * 4, s ? o.scores_f : nullptr, s},
                                      {a.best[0], p * 4, s ? o.best_h : nullptr, s},
                                      {a.best[1], p * 4, s ? o.best_f : nullptr, s},
                                      {a.best_score[0], p * 4, s ? o.best_score_h : nullptr, s},
                                      {a.best_score[1], p * 4, s ? o.best_score_f : nullptr, s}},
                                     block.data(), L.end))
                return line;
        }
    }
    return 0;
}

int staging_check_rec_subsets() {
    const int cap = 130, P = 3;
    const size_t p = P, pc = p * cap;
    static float gf[5];
    static int32_t gi[4];
    OrbLayout most;
    TestRec a0{};
    rec_regions(most, RecOut{}, cap, P, a0);
    std::vector<uint8_t> block(most.end);
    for (unsigned m = 0; m < (1u << 8); ++m) {
        RecOut o{};
        if (m & 1) o.n_motion = gi;
        if (m & 2) o.n_inliers = gi + 1;
        if (m & 4) o.best = gi + 2;
        if (m & 8) o.motion_R = gf;
        if (m & 16) o.motion_t = gf + 1;
        if (m & 32) o.n_good = gi + 3;
        if (m & 64) o.cos_parallax = gf + 2;
        if (m & 128) o.parallax_deg = gf + 3;
        OrbLayout size, L(block.data());
        TestRec as{}, a{};
        rec_regions(size, o, cap, P, as);
        rec_regions(L, o, cap, P, a);
        EXPECT(size.end == L.end && L.end <= most.end);
        if (int line = pieces_ok({{a.ord_i, pc * 4, nullptr, true},
                                  {a.nwalk, p * 4, nullptr, true},
                                  {a.flags, pc * 8, nullptr, true},
                                  {a.cosv, pc * 8 * 4, nullptr, true},
                                  {a.n_motion, p * 4, o.n_motion, true},
                                  {a.n_inliers, p * 4, o.n_inliers, true},
                                  {a.best, p * 4, o.best, true},
                                  {a.motion_R, p * 72 * 4, o.motion_R, true},
                                  {a.motion_t, p * 24 * 4, o.motion_t, true},
                                  {a.n_good, p * 8 * 4, o.n_good, true},
                                  {a.cos_sel, p * 8 * 4, o.cos_parallax, true},
                                  {a.parallax, p * 8 * 4, o.parallax_deg, true}},
                                 block.data(), L.end))
            return line;
    }
    return 0;
}

// A stage on memory of exactly the planned sizes (so that the sanitizer sees a step outside): put,
// zero-fill, send, get with a NULL destination, a count and a first element.
int staging_check_stage() {
    OrbStagePlan P;
    const auto rA = P.in<float>(65);
    const auto rB = P.in<uint8_t>(0);
    const auto rC = P.in<int32_t>(3), rX = P.out<int32_t>(7);
    const auto rY = P.out<uint8_t>(130);
    const auto rS = P.scratch<double>(9);
    EXPECT(rB.off == rC.off && P.in_end() == 512 + 256 && P.out_end() == P.in_end() + 512 && P.total() == P.out_end() + 256);
    std::vector<uint8_t> dev(P.total(), 0xAB), host(P.out_end(), 0xCD);
    const OrbStage S(P, dev.data(), host.data());
    EXPECT((uint8_t*)S.dev(rS) == dev.data() + P.out_end() && (uint8_t*)S.dev(rA) == dev.data());
    float src[65];
    for (int k = 0; k < 65; ++k) src[k] = (float)k;
    EXPECT(S.send(rA, src) == S.dev(rA) && S.host(rA)[64] == 64.0f);
    S.put(rB, (const uint8_t*)nullptr);  // nothing to write, nothing written
    S.put(rC, (const int32_t*)nullptr);  // no source: zeros
    EXPECT(S.host(rC)[0] == 0 && S.host(rC)[2] == 0 && host[rC.off + 12] == 0xCD);
    const int32_t two[2] = {5, 6};
    S.put(rC, two, 2);
    EXPECT(S.host(rC)[0] == 5 && S.host(rC)[1] == 6 && S.host(rC)[2] == 0);
    S.zero_in();
    EXPECT(S.host(rA)[64] == 0.0f && S.host(rC)[1] == 0 && host[P.in_end()] == 0xCD);
    for (int k = 0; k < 7; ++k) S.host(rX)[k] = 100 + k;
    for (int k = 0; k < 130; ++k) S.host(rY)[k] = (uint8_t)k;
    int32_t x[7] = {0}, one = 0;
    S.get(rX, x);
    S.get(rX, &one, 1, 6);
    S.get(rX, (int32_t*)nullptr);
    EXPECT(x[0] == 100 && x[6] == 106 && one == 106);
    uint8_t y[66] = {0};
    S.get(rY, y, 65, 65);
    EXPECT(y[0] == 65 && y[64] == 129 && y[65] == 0);
    S.get(rY, y, 0, 130);
    return 0;
}

}  // extern "C"

#ifdef STAGING_HOST_MAIN
int main() {
    int (*const checks[])() = {staging_check_chain4, staging_check_cases, staging_check_chain_subsets,
                               staging_check_rec_subsets, staging_check_stage};
    int bad = 0;
    for (auto f : checks) {
        const int line = f();
        if (line) printf("expectation at line %d failed\n", line), ++bad;
    }
    printf("status %d\n", bad);
    return bad ? 1 : 0;
}
#endif
