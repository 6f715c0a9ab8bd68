// orb_extract_plan.h — the extractor's host arithmetic, HIP-free: what the ORBextractor constructor
// computes (ExtractParams) and everything a frame size decides (ExtractPlan: level and cell
// geometry, OpenCV's resize tables, k_fast's tiles, LDS sizes, k_pyr_stream's round schedule).
// plan_extract fills a plan or refuses the geometry; it allocates nothing on a device.  The
// handle (orb_hip.hip) uploads the tables and passes Geom / StreamGeom to the kernels by value;
// tests/native/extract_plan_host.cpp compiles this header with a plain C++ compiler.  DESIGN.md
// ("the extractor's plan") lists who reads which table and the order of the refusals.
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/orb_abi.h"
#include "orb_extract_geom.h"

// ---- sizes the kernels and the planner agree on ---------------------------------------------
// k_pyr_resize: one workgroup per RZ_TW x RZ_TH tile of the padded level
#define RZ_TW 256  // 64 lanes x 4 columns
#ifndef RZ_TH
#define RZ_TH 32
#endif
#ifndef RZ_THS
#define RZ_THS 4  // tile rows for batches below KR_SHORT_BATCH (B=1 640x480: 0.074 -> 0.035 ms for levels 1-7)
#endif
#define RT_LDS_MAX (150 * 1024)  // k_pyr_resize_tail: ping-pong ROIs + staged tables at most
#ifndef PS_LDS_TARGET
#define PS_LDS_TARGET (76 * 1024)  // k_pyr_stream: two workgroups per CU
#endif
#define RR_Q 320  // k_rerun: per-wave queue of compass survivors (< 64 carried + 4 x 64 new), + a trash slot
#ifndef OD_WAVES
#define OD_WAVES 4  // keypoint slots (waves) per workgroup (8 / 2 measured slower: 0.521 / 0.474 vs 0.468 ms c3;
                    // two slots per wave, lanes 0-31 / 32-63, 2 or 4 waves per workgroup: 0.531 / 0.567 vs
                    // 0.428 ms c3, 1.018 / 1.093 vs 0.818 c4 -- half the waves per CU, longer chains)
#endif

namespace orbplan {

inline int cvRoundH(double v) { return (int)lrint(v); }
inline short satS16(int v) { return (short)std::min(std::max(v, -32768), 32767); }

// OpenCV 2.4 getGaussianKernel(7, 2, CV_32F) -> convertTo(CV_32S, 256).
inline void gaussian_taps7(int* k7) {
    double scale2X = -0.5 / (2.0 * 2.0), sum = 0;
    float cf[7];
    for (int i = 0; i < 7; ++i) {
        double x = i - 3.0;
        cf[i] = (float)std::exp(scale2X * x * x);
        sum += cf[i];
    }
    sum = 1. / sum;
    for (int i = 0; i < 7; ++i) cf[i] = (float)(cf[i] * sum);
    for (int i = 0; i < 7; ++i) k7[i] = cvRoundH(cf[i] * 256.0f);
}

// LDS of one FAST(7) cell re-run over a dw x dh detection area (k_rerun, cell_fast_rerun):
// Sp | Bm | rowc | In | the per-wave queues
inline size_t rerun_lds(int dw, int dh) {
    const size_t dwp = (size_t)((dw + 3) & ~3);
    const size_t inW = (size_t)((15 + dw + 6 + 15) & ~15), spBytes = (dwp * dh + 15) & ~(size_t)15;
    const size_t bmBytes = 4 * (size_t)((dh * ((dw + 31) >> 5) + 3) & ~3);
    return spBytes + bmBytes + 4 * (size_t)((dh + 3) & ~3) + inW * (dh + 6) + 16 + 4 * (4 + 4 * (RR_Q + 8));
}

// k_select: survivors per level held in LDS (beyond: the global-scratch path, same result), per frame
// size: (W*H / 200) rounded down to 512 in [1024, 3072] -- 1536 at 640x480 (6 -> 10 work-groups
// per CU: 0.177 -> 0.146 ms with 3072), 2048 at 1241x376 (0.499 -> 0.474), 3072 at 1280x720
// (2048 there: 0.84 -> 1.14, most levels past LDS)
inline int select_cap(int w, int h) {
    return std::min(3072, std::max(1024, (int)(((long long)w * h / 200) & ~511ll)));
}

// ORBextractor ctor arithmetic (ORBextractor.cc:462-510)
struct ExtractParams {
    int nfeatures = 0, nlevels = 0, scoreType = 1, fastTh = 20;
    double scaleFactor = 1.2;  // double member, as in the reference (ORBextractor.h:62)
    std::vector<float> mvScaleFactor, mvInvScaleFactor;
    std::vector<int> nDesired;
    int kpCap = 0;  // sum of nDesired
    int umax[16] = {};
};

inline ExtractParams extract_params(int nfeatures, double scaleFactor, int nlevels, int scoreType, int fastTh) {
    ExtractParams p;
    p.nfeatures = nfeatures;
    p.scaleFactor = scaleFactor;
    p.nlevels = nlevels;
    p.scoreType = scoreType;
    p.fastTh = fastTh;
    p.mvScaleFactor.assign(nlevels, 1.f);
    for (int i = 1; i < nlevels; ++i) p.mvScaleFactor[i] = (float)(p.mvScaleFactor[i - 1] * scaleFactor);
    float invScaleFactor = (float)(1.0f / scaleFactor);
    p.mvInvScaleFactor.assign(nlevels, 1.f);
    for (int i = 1; i < nlevels; ++i) p.mvInvScaleFactor[i] = p.mvInvScaleFactor[i - 1] * invScaleFactor;
    p.nDesired.assign(nlevels, 0);
    float factor = (float)(1.0 / scaleFactor);
    float nd = nfeatures * (1 - factor) / (1 - (float)std::pow((double)factor, (double)nlevels));
    int sum = 0;
    for (int l = 0; l < nlevels - 1; ++l) {
        p.nDesired[l] = cvRoundH(nd);
        sum += p.nDesired[l];
        nd *= factor;
    }
    p.nDesired[nlevels - 1] = std::max(nfeatures - sum, 0);
    for (int n : p.nDesired) p.kpCap += n;
    int vmax = (int)std::floor(15 * std::sqrt(2.f) / 2 + 1), vmin = (int)std::ceil(15 * std::sqrt(2.f) / 2);
    for (int v = 0; v <= vmax; ++v) p.umax[v] = cvRoundH(std::sqrt(225.0 - v * v));
    for (int v = 15, v0 = 0; v >= vmin; --v) {
        while (p.umax[v0] == p.umax[v0 + 1]) ++v0;
        p.umax[v] = v0;
        ++v0;
    }
    return p;
}

// Everything one frame size decides.  Value-initialised: no geometry (W = H = 0).
struct ExtractPlan {
    int W = 0, H = 0;
    Geom g{};
    std::vector<CellGeom> cells;   // k_rerun, k_select
    std::vector<int> rtab;         // per level >= 1: xofs | alpha | yofs | beta | tiles<RZ_TH> | tiles<RZ_THS>
    std::vector<FastTile> tiles;   // k_fast
    std::vector<uint8_t> slotLvl;  // keypoint slot -> level (kpCap bytes, padded to a dword): k_orient_desc
    long long pyrBytes = 0;        // the pyramid of max_batch frames (the levels' base + fstride)
    size_t listLds = 0;            // k_select: the survivor lists
    size_t cellLds = 0;            // k_rerun: a FAST(7) re-run's LDS (largest cell)
    size_t resizeLds[ORB_MAX_LEVELS] = {}, resizeLdsS[ORB_MAX_LEVELS] = {};
    int resizeTail = 0;            // first level of k_pyr_resize_tail (nlevels: none)
    int tailBufA = 0, tailBufB = 0;
    size_t tailLds = 0;
    // k_pyr_stream (plan_stream); streamOk false: per-level launches only, noStream says why
    bool streamOk = false;
    const char* noStream = "";
    StreamGeom sgeom{};
    size_t streamLds = 0;
    int streamK0 = 0;                    // level-0 rows per round
    std::vector<StreamLevel> streamLv;
    std::vector<int> streamCap;          // ring rows of levels 0 .. L-2
    std::vector<uint32_t> streamCol;     // column words
    std::vector<uint32_t> streamRows;    // row entries, 8 words each, in round order
    std::vector<uint32_t> streamRounds;  // per round: L level words, first entry, entries
};

// k_pyr_stream's plan: the round schedule (greedy: level l computes every row whose source
// rows of level l-1 are in its ring), the ring capacity of each level (max over rounds of
// newest row written - oldest row read + 1), ring slots, per-row and per-quad tables.  K0
// (level-0 rows per round) is the largest whose rings fit PS_LDS_TARGET.  Frames with a
// level under 17 px (multiple reflections) or rings that never fit keep the per-level path:
// P.streamOk stays false and P.noStream names the reason.
inline void plan_stream(ExtractPlan& P) {
    const Geom& G = P.g;
    const std::vector<int>& rt = P.rtab;
    const int L = G.L;
    auto give_up = [&](const char* why) { P.noStream = why; };
    if (L < 2) return give_up("one level: nothing to stream");
    for (int l = 0; l < L; ++l)
        if (G.lv[l].w < 17 || G.lv[l].h < 17) return give_up("a level under 17 px (multiple reflections)");
    const int u0 = (G.lv[0].w + 15) / 16;
    std::vector<std::vector<int>> s0(L), s1(L);
    for (int l = 1; l < L; ++l) {
        const LevelGeom& lg = G.lv[l];
        const int hs = G.lv[l - 1].h;
        const int* yofs = rt.data() + lg.rtab + 2 * lg.w;
        s0[l].resize(lg.h);
        s1[l].resize(lg.h);
        for (int dy = 0; dy < lg.h; ++dy) {
            s0[l][dy] = std::min(std::max(yofs[dy], 0), hs - 1);
            s1[l][dy] = std::min(std::max(yofs[dy] + 1, 0), hs - 1);
        }
    }
    auto ringPitch = [&](int l) { return (G.lv[l].w + 15) & ~15; };
    auto nqOf = [&](int l) { return l == 0 ? G.lv[0].pitch / 16 : G.lv[l].pitch / 4; };
    // column words (LDS-resident): one u32 per padded column of levels >= 1
    // sx | a1 << 12 | (a0 - 2047 + a1) << 24 | simd << 26 | live << 27
    std::vector<uint32_t> cw;
    std::vector<int> colQuad(L, 0);
    for (int l = 1; l < L; ++l) {
        const LevelGeom& lg = G.lv[l];
        const int* xofs = rt.data() + lg.rtab;
        const int* alpha = xofs + lg.w;
        colQuad[l] = (int)(cw.size() / 4);
        for (int px = 0; px < 4 * nqOf(l); ++px) {
            const int lx = orbdev::reflect101(std::min(px, lg.w + 2 * orbdev::EDGE - 1) - orbdev::EDGE, lg.w);
            const int sx = xofs[lx];
            const int a0 = lx < lg.xmax ? (alpha[lx] & 0xFFFF) : 2048;
            const int a1 = lx < lg.xmax ? ((alpha[lx] >> 16) & 0xFFFF) : 0;
            const int d = a0 - 2047 + a1;
            if (sx < 0 || sx > 0xFFF || a1 > 0xFFF || d < 0 || d > 3)
                return give_up("a column word is not encodable (source column, tap or tap sum out of its field)");
            uint32_t c = (uint32_t)sx | ((uint32_t)a1 << 12) | ((uint32_t)d << 24);
            if (lx < lg.xs_resize) c |= 1u << 26;
            if (px < lg.w + 2 * orbdev::EDGE) c |= 1u << 27;
            cw.push_back(c);
        }
    }
    const size_t colBytes = (cw.size() * 4 + 15) & ~(size_t)15;
    std::vector<uint32_t> rounds;
    std::vector<int> cap;
    std::vector<std::vector<int>> plan;  // per round: lo, cnt per level
    int K0 = 0, maxEnt = 0;
    size_t lds = 0;
    for (int k0 : {32, 24, 16, 12, 8, 6, 4, 2}) {
        if (k0 * u0 > PS_NPF * 64 * PS_LOADERS) continue;
        std::vector<int> next(L, 0), cp(L, 0);
        std::vector<std::vector<int>> pl;
        int me = 0;
        bool ok = true;
        for (int n = 0;; ++n) {
            bool done = true;
            for (int l = 0; l < L; ++l) done = done && next[l] >= G.lv[l].h;
            if (done) break;
            if (n > 65536) {
                ok = false;
                break;
            }
            std::vector<int> lo(L), cnt(L);
            lo[0] = next[0];
            cnt[0] = std::min(k0, G.lv[0].h - next[0]);
            const int avail0 = next[0] + cnt[0];
            for (int l = 1; l < L; ++l) {
                const int srcAvail = l == 1 ? avail0 : next[l - 1];
                int d = next[l];
                while (d < G.lv[l].h && s1[l][d] < srcAvail) ++d;
                lo[l] = next[l];
                cnt[l] = d - next[l];
            }
            for (int l = 0; l + 1 < L; ++l) {
                // level 0: the loaders store round n+1's rows during round n
                const int newest = (l == 0 ? std::min(avail0 + k0, G.lv[0].h) : next[l] + cnt[l]) - 1;
                int oldest = INT32_MAX;
                if (l == 0 && cnt[0]) oldest = lo[0];
                if (cnt[l + 1]) oldest = std::min(oldest, s0[l + 1][lo[l + 1]]);
                if (oldest != INT32_MAX) cp[l] = std::max(cp[l], newest - oldest + 1);
            }
            std::vector<int> rec(2 * L);
            int ent = 0;
            for (int l = 0; l < L; ++l) {
                rec[2 * l] = lo[l];
                rec[2 * l + 1] = cnt[l];
                ent += cnt[l];
                next[l] += cnt[l];
            }
            me = std::max(me, ent);
            pl.push_back(std::move(rec));
        }
        if (!ok || me > PS_NPF * 64 * PS_LOADERS) continue;
        size_t bytes = 0;
        bool capOk = true;
        for (int l = 0; l + 1 < L; ++l) {
            cp[l] = std::min(std::max(cp[l], 1), G.lv[l].h);
            capOk = capOk && cp[l] <= 255;
            bytes += (size_t)cp[l] * ringPitch(l);
        }
        const int stride8 = (me + 1) & ~1;
        bytes += colBytes;
        if (capOk && bytes <= PS_LDS_TARGET) {
            K0 = k0;
            plan = std::move(pl);
            cap = std::move(cp);
            maxEnt = stride8;
            lds = bytes;
            break;
        }
    }
    if (!K0) return give_up("no K0 of the ladder whose rings and column words fit PS_LDS_TARGET");
    std::vector<StreamLevel> lv(L);
    int ringOff = 0;
    for (int l = 0; l < L; ++l) {
        const LevelGeom& lg = G.lv[l];
        StreamLevel& s = lv[l];
        s.nq = nqOf(l);
        s.nqm = (uint32_t)((0x100000000ull + s.nq - 1) / (uint64_t)s.nq);
        s.ringPitch = ringPitch(l);
        s.ringOff = l + 1 < L ? ringOff : 0;
        if (l + 1 < L) ringOff += cap[l] * s.ringPitch;
        s.w = lg.w;
        s.h = lg.h;
        s.pitch = lg.pitch;
        s.base = lg.base;
        s.fstride = lg.fstride;
    }
    // waves per level: one each, then greedily to the level with the most work per wave
    // (level-0 units are copies: weighted 1/4), up to one wave per 64 column units
    if (L > PS_THREADS / 64 - PS_LOADERS)
        return give_up("more levels than builder waves (L > PS_THREADS / 64 - PS_LOADERS = 14)");
    {
        std::vector<int> nw(L, 1);
        for (int left = PS_THREADS / 64 - PS_LOADERS - L; left > 0; --left) {
            int best = -1;
            double bw = 0;
            for (int l = 0; l < L; ++l) {
                if (nw[l] * 64 >= lv[l].nq) continue;
                const double wk = (double)lv[l].nq * G.lv[l].h * (l == 0 ? 0.25 : 1.0) / nw[l];
                if (wk > bw) {
                    bw = wk;
                    best = l;
                }
            }
            if (best < 0) break;
            ++nw[best];
        }
        int ws = PS_LOADERS;
        for (int l = 0; l < L; ++l) {
            lv[l].waveStart = ws;
            lv[l].nWaves = nw[l];
            ws += nw[l];
        }
    }
    const int colOff = ringOff;  // multiple of 16
    for (int l = 1; l < L; ++l) lv[l].colOff = colOff + 16 * colQuad[l];
    lv[0].colOff = 0;
    // rounds (L level words + the first entry) and the row entries in round order: per row
    // {source row 0, source row 1 (LDS addresses), b0 << 12, b1 << 12, own ring row (LDS
    //  address or ~0u), padded-row offset, top mirror offset, bottom mirror offset (~0u: none)}
    std::vector<uint32_t> ent;
    for (const auto& rec : plan) {
        int ne = 0;
        for (int l = 0; l < L; ++l) {
            if (rec[2 * l] > 0xFFF || rec[2 * l + 1] > 0x3F || ne > 0x3FFF)
                return give_up("a round word is not encodable (first row, row count or entry offset out of its field)");
            rounds.push_back((uint32_t)rec[2 * l] | ((uint32_t)rec[2 * l + 1] << 12) | ((uint32_t)ne << 18));
            ne += rec[2 * l + 1];
        }
        rounds.push_back((uint32_t)(ent.size() / 8));
        rounds.push_back((uint32_t)ne);
        for (int l = 0; l < L; ++l)
            for (int dy = rec[2 * l]; dy < rec[2 * l] + rec[2 * l + 1]; ++dy) {
                const LevelGeom& lg = G.lv[l];
                const uint32_t own =
                    l + 1 < L ? (uint32_t)(lv[l].ringOff + (dy % cap[l]) * lv[l].ringPitch) : 0xFFFFFFFFu;
                const uint32_t main = (uint32_t)((dy + orbdev::EDGE) * lg.pitch);
                const uint32_t top = dy >= 1 && dy <= orbdev::EDGE ? (uint32_t)((orbdev::EDGE - dy) * lg.pitch) : 0xFFFFFFFFu;
                const uint32_t bot = dy >= lg.h - 17 && dy <= lg.h - 2 ? (uint32_t)((2 * lg.h + 14 - dy) * lg.pitch) : 0xFFFFFFFFu;
                if (l == 0) {
                    ent.insert(ent.end(), {own, 0u, 0u, 0u, 0xFFFFFFFFu, main, top, bot});
                } else {
                    const int cs = cap[l - 1];
                    const uint32_t beta = (uint32_t)rt[lg.rtab + 2 * lg.w + lg.h + dy];
                    const uint32_t a0 = (uint32_t)(lv[l - 1].ringOff + (s0[l][dy] % cs) * lv[l - 1].ringPitch);
                    const uint32_t a1 = (uint32_t)(lv[l - 1].ringOff + (s1[l][dy] % cs) * lv[l - 1].ringPitch);
                    ent.insert(ent.end(), {a0, a1, (beta & 0xFFFFu) << 12, (beta >> 16) << 12, own, main, top, bot});
                }
            }
    }
    // the magic divisions are exact over every task index of every round
    for (int l = 0; l < L; ++l) {
        int maxCnt = 0;
        for (const auto& rec : plan) maxCnt = std::max(maxCnt, rec[2 * l + 1]);
        for (uint32_t i = 0; i < (uint32_t)(maxCnt * lv[l].nq); ++i)
            if ((uint32_t)(((uint64_t)i * lv[l].nqm) >> 32) != i / (uint32_t)lv[l].nq)
                return give_up("a level's row reciprocal is not exact over its task indices");
    }
    StreamGeom sg{};
    sg.L = L;
    sg.nRounds = (int)plan.size();
    sg.u0 = u0;
    sg.u0m = (uint32_t)((0x100000000ull + u0 - 1) / (uint64_t)u0);
    for (uint32_t i = 0; i < (uint32_t)(K0 * u0); ++i)
        if ((uint32_t)(((uint64_t)i * sg.u0m) >> 32) != i / (uint32_t)u0)
            return give_up("level 0's unit reciprocal is not exact over a round's units");
    sg.colWords = (int)cw.size();
    sg.colOff = colOff;
    sg.rowOff = colOff + (int)colBytes;
    sg.rowStride = maxEnt;
    sg.cap0 = cap[0];
    P.sgeom = sg;
    P.streamLv = std::move(lv);
    P.streamCap = std::move(cap);
    P.streamCol = std::move(cw);
    P.streamRows = std::move(ent);
    P.streamRounds = std::move(rounds);
    P.streamLds = lds;
    P.streamK0 = K0;
    P.streamOk = true;
}

// The plan of frame size w0 x h0 for batches of up to maxBatch frames (fastCl: Geom::fastCl).
// ORB_OK and `out` filled, or the refusal's code with its text in `err` and `out` left empty.
// The checks run in this order; the first that fails names the refusal.
inline int plan_extract(const ExtractParams& prm, int w0, int h0, int maxBatch, int fastCl, ExtractPlan& out,
                        std::string& err) {
    out = ExtractPlan{};
    auto refuse = [&](int code, std::string msg) {
        err = std::move(msg);
        return code;
    };
    const int nlevels = prm.nlevels;
    ExtractPlan P;
    Geom& G = P.g;
    G.L = nlevels;
    G.fastTh = std::min(std::max(prm.fastTh, 0), 255);
    G.fastCl = fastCl;
    G.scoreType = prm.scoreType;
    int k7[7];
    gaussian_taps7(k7);
    for (int i = 0; i < 4; ++i) G.taps[i] = k7[3 + i];
    if (G.taps[0] != 55 || G.taps[1] != 49 || G.taps[2] != 34 || G.taps[3] != 18)
        return refuse(ORB_EINVAL, "Gaussian taps differ from the kernel's constants (c_rowB, GP_*)");
    for (int v = 0; v < 16; ++v) G.umax[v] = prm.umax[v];
    G.umaxNib = 0;
    for (int v = 0; v < 16; ++v) G.umaxNib |= (unsigned long long)prm.umax[v] << (4 * v);
    std::vector<CellGeom>& cl = P.cells;
    std::vector<int>& rt = P.rtab;
    int cand = 0, kpBase = 0;
    for (int l = 0; l < nlevels; ++l) {
        LevelGeom& lg = G.lv[l];
        float sc = prm.mvInvScaleFactor[l];
        lg.w = cvRoundH((float)w0 * sc);
        lg.h = cvRoundH((float)h0 * sc);
        if (lg.w < 1 || lg.h < 1 || lg.w >= 4096 || lg.h >= 4096)
            return refuse(ORB_ENOTSUP, "level size out of the supported range [1, 4095]");
        lg.pitch = (lg.w + 2 * orbdev::EDGE + 15) & ~15;
        lg.ph = lg.h + 2 * orbdev::EDGE;
        lg.fstride = (long long)lg.pitch * lg.ph;
        lg.base = P.pyrBytes;
        P.pyrBytes += lg.fstride * maxBatch;
        lg.scale = prm.mvScaleFactor[l];
        lg.size = (float)(int)(31 * prm.mvScaleFactor[l]);
        lg.xsimd_blur = (lg.w / 4) * 4;
        lg.nDesired = prm.nDesired[l];
        lg.kpBase = kpBase;
        kpBase += prm.nDesired[l];
    }
    // cell grid (ORBextractor.cc:527-597)
    const float imageRatio = (float)G.lv[0].w / G.lv[0].h;
    for (int l = 0; l < nlevels; ++l) {
        LevelGeom& lg = G.lv[l];
        const int nD = prm.nDesired[l];
        const int levelCols = (int)std::sqrt((float)nD / (5 * imageRatio));
        const int levelRows = (int)(imageRatio * levelCols);
        if (levelCols <= 0 || levelRows <= 0)
            return refuse(ORB_ENOTSUP, "level " + std::to_string(l) + " has an empty cell grid (the reference "
                                       "divides by zero here)");
        if (levelCols * levelRows > ORB_MAX_CELLS_PER_LEVEL)
            return refuse(ORB_ENOTSUP, "more than 256 cells per level");
        const int maxBX = lg.w - 16, maxBY = lg.h - 16;
        const int Wd = maxBX - 16, Hd = maxBY - 16;
        const int cellW = (int)std::ceil((float)Wd / levelCols);
        const int cellH = (int)std::ceil((float)Hd / levelRows);
        const int nCells = levelRows * levelCols;
        lg.rows = levelRows;
        lg.cols = levelCols;
        lg.nfc = (int)std::ceil((float)nD / nCells);
        lg.cellW = cellW;
        lg.cellH = cellH;
        // (a 1-px cell's reciprocal 2^32 does not fit: 2^32 - 1, which k_fast applies to n + 1)
        lg.cellWm = cellW == 1 ? -1 : (int)(uint32_t)((0x100000000ull + cellW - 1) / (uint64_t)cellW);
        lg.cellHm = cellH == 1 ? -1 : (int)(uint32_t)((0x100000000ull + cellH - 1) / (uint64_t)cellH);
        lg.detX1 = std::max(maxBX, levelCols > 1 ? 16 + (levelCols - 1) * cellW : 0);
        lg.detY1 = std::max(maxBY, levelRows > 1 ? 16 + (levelRows - 1) * cellH : 0);
        // keypoints of non-last cells can sit past maxBorder (ORBextractor.cc:560-597); the
        // descriptor image must hold every sample they reach (|offset| <= 18)
        lg.ringX1 = std::max(lg.w + 3, lg.detX1 + 18);
        lg.ringY1 = std::max(lg.h + 3, lg.detY1 + 18);
        if (lg.ringX1 > lg.w + 12 || lg.ringY1 > lg.h + 12)
            return refuse(ORB_ENOTSUP, "cell grid too dense: rBRIEF samples leave the 16-px padding");
        if (cellW <= 0 || cellH <= 0) return refuse(ORB_ENOTSUP, "empty cell size");
        lg.cell0 = (int)cl.size();
        std::vector<int> iniXCol(levelCols, 0);
        float hY = cellH + 6;
        for (int i = 0; i < levelRows; ++i) {
            const float iniY = 16 + i * cellH - 3;
            bool rowSkip = false;
            if (i == levelRows - 1) {
                hY = maxBY + 3 - iniY;
                if (hY <= 0) rowSkip = true;
            }
            float hX = cellW + 6;
            for (int j = 0; j < levelCols; ++j) {
                CellGeom c{};
                c.level = l;
                float iniX;
                if (rowSkip) {
                    c.skipped = 1;
                } else {
                    if (i == 0) {
                        iniX = 16 + j * cellW - 3;
                        iniXCol[j] = (int)iniX;
                    } else {
                        iniX = iniXCol[j];
                    }
                    if (j == levelCols - 1) {
                        hX = maxBX + 3 - iniX;
                        if (hX <= 0) c.skipped = 1;
                    }
                    if (!c.skipped) {
                        c.x0 = (int)iniX;
                        c.y0 = (int)iniY;
                        c.hx = (int)(iniX + hX) - c.x0;
                        c.hy = (int)(iniY + hY) - c.y0;
                        if (c.x0 < 0 || c.y0 < 0 || c.x0 + c.hx > lg.w || c.y0 + c.hy > lg.h)
                            return refuse(ORB_ENOTSUP, "cell ROI outside the level (the reference asserts)");
                        int dw = c.hx - 6, dh = c.hy - 6;
                        c.cap = (dw > 0 && dh > 0) ? ((dw + 1) / 2) * ((dh + 1) / 2) : 0;
                        if (dw > 0 && dh > 0) P.cellLds = std::max(P.cellLds, rerun_lds(dw, dh));
                    }
                }
                cl.push_back(c);
            }
        }
        // uniform slot stride per level (k_fast computes a cell's slots arithmetically)
        int capMax = 0;
        for (size_t i = lg.cell0; i < cl.size(); ++i) capMax = std::max(capMax, cl[i].cap);
        lg.candBase = cand;
        lg.capMax = capMax;
        for (size_t i = lg.cell0; i < cl.size(); ++i) cl[i].candOff = cand + (int)(i - lg.cell0) * capMax;
        cand += (int)(cl.size() - lg.cell0) * capMax;
    }
    G.selCap = select_cap(w0, h0);
    P.listLds = (size_t)(prm.scoreType == ORB_HARRIS_SCORE ? 4 : 2) * G.selCap * 4;
    if (std::max(P.cellLds, P.listLds) > 150 * 1024)
        return refuse(ORB_ENOTSUP, "FAST cell larger than the LDS budget");
    // resize tables, l >= 1
    for (int l = 1; l < nlevels; ++l) {
        LevelGeom& lg = G.lv[l];
        const LevelGeom& ls = G.lv[l - 1];
        const int sw = ls.w, sh = ls.h, dw = lg.w, dh = lg.h;
        double inv_sx = (double)dw / sw, inv_sy = (double)dh / sh;
        double scale_x = 1. / inv_sx, scale_y = 1. / inv_sy;
        int isx = cvRoundH(scale_x), isy = cvRoundH(scale_y);
        if (std::abs(scale_x - isx) < 2.220446049250313e-16 && std::abs(scale_y - isy) < 2.220446049250313e-16 &&
            isx == 2 && isy == 2)
            return refuse(ORB_ENOTSUP, "exact 2x level step (OpenCV switches to INTER_AREA)");
        lg.rtab = (int)rt.size();
        std::vector<int> xofs(dw), alpha(dw), yofs(dh), beta(dh);
        int xmax = dw;
        for (int dx = 0; dx < dw; ++dx) {
            float fx = (float)((dx + 0.5) * scale_x - 0.5);
            int sx = (int)std::floor(fx);
            fx -= sx;
            if (sx < 0) fx = 0, sx = 0;
            if (sx + 1 >= sw) {
                xmax = std::min(xmax, dx);
                if (sx >= sw - 1) fx = 0, sx = sw - 1;
            }
            xofs[dx] = sx;
            short a0 = satS16(cvRoundH((1.f - fx) * 2048)), a1 = satS16(cvRoundH(fx * 2048));
            alpha[dx] = (int)(uint16_t)a0 | ((int)(uint16_t)a1 << 16);
        }
        for (int dy = 0; dy < dh; ++dy) {
            float fy = (float)((dy + 0.5) * scale_y - 0.5);
            int sy = (int)std::floor(fy);
            fy -= sy;
            yofs[dy] = sy;
            short b0 = satS16(cvRoundH((1.f - fy) * 2048)), b1 = satS16(cvRoundH(fy * 2048));
            beta[dy] = (int)(uint16_t)b0 | ((int)(uint16_t)b1 << 16);
        }
        for (int dx = 0; dx < dw; ++dx) {  // k_pyr_resize's no-saturation premise
            const int c0 = alpha[dx] & 0xFFFF, c1 = (alpha[dx] >> 16) & 0xFFFF;
            if ((short)c0 < 0 || (short)c1 < 0 || c0 + c1 > 2050)
                return refuse(ORB_ENOTSUP, "resize coefficient outside [0, 2050]");
        }
        for (int dy = 0; dy < dh; ++dy) {
            const int c0 = beta[dy] & 0xFFFF, c1 = (beta[dy] >> 16) & 0xFFFF;
            if ((short)c0 < 0 || (short)c1 < 0 || c0 + c1 > 2050)
                return refuse(ORB_ENOTSUP, "resize coefficient outside [0, 2050]");
        }
        int xs = 0;
        while (xs <= dw - 16) xs += 16;
        while (xs < dw - 4) xs += 4;
        lg.xs_resize = xs;
        lg.xmax = xmax;
        rt.insert(rt.end(), xofs.begin(), xofs.end());
        rt.insert(rt.end(), alpha.begin(), alpha.end());
        rt.insert(rt.end(), yofs.begin(), yofs.end());
        rt.insert(rt.end(), beta.begin(), beta.end());
        // source rectangle of every RZ_TW x TH tile of the padded level (k_pyr_resize), for
        // the two tile heights
        auto tiles = [&](int TH, int& off, size_t& ldsOut) {
            const int tx = (lg.pitch + RZ_TW - 1) / RZ_TW, ty = (lg.ph + TH - 1) / TH;
            off = (int)rt.size();
            size_t lds = 0;
            for (int y = 0; y < ty; ++y)
                for (int x = 0; x < tx; ++x) {
                    int c0 = INT32_MAX, c1 = -1, r0 = INT32_MAX, r1 = -1;
                    for (int px = x * RZ_TW; px < std::min((x + 1) * RZ_TW, lg.pitch); ++px) {
                        const int lx = orbdev::reflect101(std::min(px, dw + 31) - 16, dw);
                        const int sx = xofs[lx];
                        const int sx1 = (lx < xmax && (alpha[lx] >> 16) != 0) ? sx + 1 : sx;
                        c0 = std::min(c0, sx);
                        c1 = std::max(c1, sx1);
                    }
                    for (int py = y * TH; py < std::min((y + 1) * TH, lg.ph); ++py) {
                        const int ly = orbdev::reflect101(py - 16, dh);
                        r0 = std::min(r0, std::min(std::max(yofs[ly], 0), sh - 1));
                        r1 = std::max(r1, std::min(std::max(yofs[ly] + 1, 0), sh - 1));
                    }
                    const int cs = c0 & ~15, units = ((c1 - cs) >> 4) + 1, nr = r1 - r0 + 1;
                    rt.push_back(cs);
                    rt.push_back(units);
                    rt.push_back(r0);
                    rt.push_back(nr);
                    lds = std::max(lds, (size_t)units * 16 * nr);
                }
            ldsOut = lds;
        };
        tiles(RZ_TH, lg.rtile, P.resizeLds[l]);
        tiles(RZ_THS, lg.rtileS, P.resizeLdsS[l]);
        if (P.resizeLds[l] > 96 * 1024) return refuse(ORB_ENOTSUP, "scale factor too large for the resize tile");
    }
    // the fused small-level tail: the first level from which every later level's source
    // ROI (ping-pong A / B) plus the staged tables fit the CU's LDS
    P.resizeTail = nlevels;
    for (int l = 1; l + 1 < nlevels; ++l) {
        auto roi = [&](int k) { return k + 1 < nlevels ? (size_t)G.lv[k].w * G.lv[k].h : (size_t)0; };
        const size_t a = (roi(l) + 15) & ~(size_t)15, bsz = (roi(l + 1) + 15) & ~(size_t)15;
        const size_t need = a + bsz + (size_t)8 * (G.lv[l].w + G.lv[l].h);
        if (need <= (size_t)RT_LDS_MAX) {
            P.resizeTail = l;
            P.tailBufA = (int)a;
            P.tailBufB = (int)bsz;
            P.tailLds = need;
            break;
        }
    }
    const int kpCap = prm.kpCap;
    G.nCells = (int)cl.size();
    G.candPerFrame = cand;
    G.kpCap = kpCap;
    {  // k_orient_desc's grid is ((kpCap + slots - 1) / slots, B): bid / gridDim.x by multiply-high
        const unsigned long long gx = (unsigned long long)(std::max(kpCap, 1) + OD_WAVES - 1) / OD_WAVES;
        // and its per-slot offsets are 32-bit: descriptor bytes of the whole batch < 2^32
        if ((unsigned long long)std::max(kpCap, 1) * (unsigned long long)maxBatch * 32ull >= (1ull << 32))
            return refuse(ORB_ENOTSUP, "max_batch x keypoint capacity too large (descriptor bytes >= 4 GiB)");
        G.odDivMagic = (uint32_t)(((1ull << 32) + gx - 1) / gx);
        if (gx * gx * (unsigned long long)maxBatch >= (1ull << 32))
            return refuse(ORB_ENOTSUP, "keypoint grid too large for k_orient_desc's block decode");
    }
    // k_fast tiles over each level's detection region: the width split evenly into
    // ceil(width / 256) tiles of a multiple of 4 columns, as many rows as the LDS budgets
    // (staged tile, strength plane) and the 16-bit queue codes allow
    std::vector<FastTile>& tl = P.tiles;
    auto rcp = [](int d) { return (uint32_t)((0x100000000ull + (uint64_t)d - 1) / (uint64_t)d); };
    for (int l = 0; l < nlevels; ++l) {
        const int detW = G.lv[l].detX1 - orbdev::EDGE;
        const int nx = (detW + FT_TW_MAX - 1) / FT_TW_MAX;
        int tw4 = std::max(2, ((detW + 3) / 4 + nx - 1) / nx);
        tw4 = (tw4 + 1) & ~1;  // tiles of a multiple of 8 columns: every x0 = 0 mod 8
        const int TW = 4 * tw4;
        for (int x0 = orbdev::EDGE; x0 < G.lv[l].detX1; x0 += TW) {
            // first staged byte at sx = 16 + (x0 mod 16) in {16, 24}: the compass groups' dword
            // pairs (sx - 8 + 8 kp) 8-B aligned, and 16 bytes left of the tile for the left pair
            const int sx = 16 + (x0 & 15);
            const int sp = (sx + TW + 8 + 15) & ~15, spw = TW + 8;
            const int thMax = std::min({FT_IN_BYTES / sp - 8, FT_S_BYTES / spw - 2, 126, 4095 / (tw4 + 2) - 2});
            if (thMax < 1 || sp > 288) return refuse(ORB_EINVAL, "k_fast tile geometry");
            for (int y0 = orbdev::EDGE; y0 < G.lv[l].detY1; y0 += thMax) {
                const int th = std::min(thMax, G.lv[l].detY1 - y0);
                tl.push_back(FastTile{l, x0, y0, tw4, th, sp, sx, rcp(tw4 + 2), rcp(tw4), rcp(sp >> 4)});
            }
        }
    }
    P.slotLvl.assign(((size_t)std::max(kpCap, 1) + 3) & ~(size_t)3, 0);
    for (int l = 0; l < nlevels; ++l)
        for (int k = 0; k < G.lv[l].nDesired; ++k) P.slotLvl[(size_t)G.lv[l].kpBase + k] = (uint8_t)l;
    plan_stream(P);
    P.W = w0;
    P.H = h0;
    out = std::move(P);
    return ORB_OK;
}

}  // namespace orbplan
