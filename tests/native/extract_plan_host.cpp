// extract_plan_host.cpp — csrc/orb_extract_plan.h, the extractor's frame-size planner, as plain C++
// (build/libextract_plan_host.so, tests/test_extract_plan_host.py; with -DEXTRACT_PLAN_HOST_MAIN a
// program that runs the checks over tests/golden/extract_plan_digests.json, which is what the
// sanitizer run executes).
//
// extract_plan_describe() writes one geometry's answer as a JSON object on one line: the parameters,
// the status, whether there is a stream plan and its K0, and an FNV-1a digest of every table and of
// the scalar fields, serialised field by field (no struct padding enters a digest).  The golden file
// holds those lines as recorded from the planner's statements before they left orb_hip.hip; the
// program compares them as text, the Python test as parsed objects.
// Each extract_plan_check_*() returns 0, or the line of the first expectation that did not hold.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/orb_abi.h"
#include "../../orbslam_jpminipc_amd/csrc/orb_extract_plan.h"

using orbplan::ExtractParams;
using orbplan::ExtractPlan;

extern "C" {
struct PlanCase {
    int w, h, nf;
    float sf;  // as orb_extractor_create takes it
    int nl, score, fast_th, max_batch, fast_cl;
};
}

namespace {

#define EXPECT(c)                  \
    do {                           \
        if (!(c)) return __LINE__; \
    } while (0)

struct Planned {
    ExtractParams prm;
    ExtractPlan plan;
    int code = 0;
    std::string err;
};
Planned make(const PlanCase& c) {
    Planned r;
    r.prm = orbplan::extract_params(c.nf, c.sf, c.nl, c.score, c.fast_th);
    r.code = orbplan::plan_extract(r.prm, c.w, c.h, c.max_batch, c.fast_cl, r.plan, r.err);
    return r;
}

// ---- digests ---------------------------------------------------------------------------------
struct Digest {
    uint64_t h = 1469598103934665603ull;
    void bytes(const void* p, size_t n) {
        for (size_t i = 0; i < n; ++i) h = (h ^ ((const uint8_t*)p)[i]) * 1099511628211ull;
    }
    template <class T>
    Digest& operator<<(const T& v) {
        static_assert(std::is_arithmetic<T>::value, "fields only: a struct would bring its padding");
        bytes(&v, sizeof v);
        return *this;
    }
    template <class T>
    Digest& operator<<(const std::vector<T>& v) {
        *this << (uint64_t)v.size();
        for (const T& x : v) *this << x;
        return *this;
    }
};
void put(Digest& d, const LevelGeom& g) {
    d << g.w << g.h << g.pitch << g.ph << g.base << g.fstride << g.rows << g.cols << g.cell0 << g.nDesired << g.nfc
      << g.kpBase << g.xsimd_blur << g.xs_resize << g.xmax << g.rtab << g.rtile << g.rtileS << g.scale << g.size
      << g.cellW << g.cellH << g.cellWm << g.cellHm << g.candBase << g.capMax << g.detX1 << g.detY1 << g.ringX1
      << g.ringY1;
}

struct Field {
    const char* name;
    uint64_t value;
};
std::vector<Field> digests(const ExtractParams& prm, const ExtractPlan& P) {
    std::vector<Field> out;
    const Geom& G = P.g;
    {
        Digest d;
        d << prm.mvScaleFactor << prm.mvInvScaleFactor << prm.nDesired << prm.kpCap;
        for (int v = 0; v < 16; ++v) d << prm.umax[v];
        out.push_back({"params", d.h});
    }
    {
        Digest d;
        d << G.L << G.nCells << G.candPerFrame << G.kpCap << G.selCap << G.fastTh << G.scoreType;
        for (int i = 0; i < 4; ++i) d << G.taps[i];
        for (int v = 0; v < 16; ++v) d << G.umax[v];
        d << G.umaxNib << G.odDivMagic << G.fastCl;
        for (int l = 0; l < ORB_MAX_LEVELS; ++l) put(d, G.lv[l]);
        out.push_back({"geom", d.h});
    }
    {
        Digest d;
        d << (uint64_t)P.cells.size();
        for (const CellGeom& c : P.cells)
            d << c.level << c.x0 << c.y0 << c.hx << c.hy << c.cap << c.candOff << c.skipped << c.cornerOff;
        out.push_back({"cells", d.h});
    }
    out.push_back({"rtab", (Digest() << P.rtab).h});
    {
        Digest d;
        d << (uint64_t)P.tiles.size();
        for (const FastTile& t : P.tiles)
            d << t.level << t.x0 << t.y0 << t.tw4 << t.th << t.sp << t.sx << t.rcpF << t.rcpI << t.rcpU;
        out.push_back({"tiles", d.h});
    }
    out.push_back({"slot_levels", (Digest() << P.slotLvl).h});
    {
        Digest d;
        d << P.W << P.H << (int64_t)P.pyrBytes << (uint64_t)P.listLds << (uint64_t)P.cellLds;
        for (int l = 0; l < ORB_MAX_LEVELS; ++l) d << (uint64_t)P.resizeLds[l] << (uint64_t)P.resizeLdsS[l];
        d << P.resizeTail << P.tailBufA << P.tailBufB << (uint64_t)P.tailLds;
        out.push_back({"scalars", d.h});
    }
    if (!P.streamOk) return out;
    {
        const StreamGeom& s = P.sgeom;
        Digest d;
        d << s.L << s.nRounds << s.u0 << s.u0m << s.align << s.colWords << s.colOff << s.rowOff << s.rowStride << s.cap0;
        d << P.streamK0 << (uint64_t)P.streamLds << P.streamCap;
        out.push_back({"stream_geom", d.h});
    }
    {
        Digest d;
        d << (uint64_t)P.streamLv.size();
        for (const StreamLevel& s : P.streamLv)
            d << s.nq << s.nqm << s.ringOff << s.ringPitch << s.colOff << s.waveStart << s.nWaves << s.w << s.h << s.pitch
              << s.base << s.fstride;
        out.push_back({"stream_levels", d.h});
    }
    out.push_back({"stream_col_words", (Digest() << P.streamCol).h});
    out.push_back({"stream_row_entries", (Digest() << P.streamRows).h});
    out.push_back({"stream_rounds", (Digest() << P.streamRounds).h});
    return out;
}

}  // namespace

// One line of the golden file (no newline) for a geometry whose planning gave `code`.
std::string extract_plan_line(const char* name, const PlanCase& c, int code, const ExtractParams& prm,
                              const ExtractPlan& P) {
    char b[512];
    snprintf(b, sizeof b,
             "{\"name\": \"%s\", \"w\": %d, \"h\": %d, \"nf\": %d, \"sf\": %.9g, \"nl\": %d, \"score\": %d, \"fast_th\": %d, "
             "\"max_batch\": %d, \"fast_cl\": %d, \"code\": %d, \"stream\": %d, \"k0\": %d, \"rounds\": %d, \"digests\": {",
             name, c.w, c.h, c.nf, (double)c.sf, c.nl, c.score, c.fast_th, c.max_batch, c.fast_cl, code,
             (int)P.streamOk, P.streamK0, P.sgeom.nRounds);
    std::string s = b;
    if (code == ORB_OK) {
        bool first = true;
        for (const Field& f : digests(prm, P)) {
            snprintf(b, sizeof b, "%s\"%s\": \"%016llx\"", first ? "" : ", ", f.name, (unsigned long long)f.value);
            s += b;
            first = false;
        }
    }
    return s + "}}";
}

namespace {

uint32_t umulhi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }
int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// What tests/test_gpu_pyramid_geometry.py::test_plans_match_the_table asserts of a case's plan.
int check_table_row(const PlanCase& c, int expectPlan, int k0) {
    const Planned r = make(c);
    const ExtractPlan& P = r.plan;
    EXPECT(r.code == ORB_OK);
    EXPECT((int)P.streamOk == expectPlan);
    if (!P.streamOk) {
        EXPECT(P.streamLv.empty() && P.noStream[0] != 0);
        return 0;
    }
    EXPECT(P.noStream[0] == 0);
    EXPECT(P.streamK0 == k0);
    EXPECT(P.sgeom.nRounds >= (c.h + k0 - 1) / k0 && P.streamLds > 0 && P.streamLds <= 76 * 1024);
    EXPECT((int)P.streamLv.size() == c.nl && (int)P.streamCap.size() == c.nl);  // (the last level has no ring: 0)
    int waves = 0;
    for (int l = 0; l < c.nl; ++l) {
        const StreamLevel& s = P.streamLv[l];
        EXPECT(s.nWaves >= 1);
        waves += s.nWaves;
        if (c.nl >= 13 && l >= 1) EXPECT(s.nWaves == 1);
        const int pitch = (P.g.lv[l].w + 32 + 15) & ~15;
        EXPECT(s.nq == (l == 0 ? pitch / 16 : pitch / 4));
        if (l + 1 < c.nl) EXPECT(P.streamCap[l] >= 1 && P.streamCap[l] <= std::min(255, P.g.lv[l].h));
    }
    EXPECT(waves <= 14);
    return 0;
}

struct Refusal {
    PlanCase c;
    const char* text;
};
const Refusal REFUSALS[] = {
    {{5000, 100, 1000, 1.2f, 3, 1, 20, 1, FT_CL}, "level size out of the supported range"},
    {{640, 480, 10, 1.2f, 8, 1, 20, 1, FT_CL}, "level 0 has an empty cell grid"},
    {{300, 200, 300, 2.0f, 2, 1, 20, 1, FT_CL}, "exact 2x level step"},
    {{640, 480, 20000, 1.2f, 1, 1, 20, 1, FT_CL}, "more than 256 cells per level"},
    {{2000, 1500, 1000, 6.0f, 2, 1, 20, 1, FT_CL}, "scale factor too large for the resize tile"},
    {{640, 480, 1000, 1.2f, 16, 1, 20, 1, FT_CL}, "empty cell size"},
    {{4095, 4095, 1000, 1.2f, 2, 1, 20, 1, FT_CL}, "FAST cell larger than the LDS budget"},
    {{64, 48, 5000, 1.2f, 8, 1, 20, 1, FT_CL}, "cell grid too dense"},
};

int check_invariants(const PlanCase& c) {
    const Planned r = make(c);
    EXPECT(r.code == ORB_OK);
    const ExtractPlan& P = r.plan;
    const Geom& G = P.g;
    const int L = c.nl;
    EXPECT(G.L == L && P.W == c.w && P.H == c.h);
    // cells lie inside their level; candidate slots of distinct cells are disjoint and end at candPerFrame
    EXPECT((int)P.cells.size() == G.nCells);
    long long slotEnd = 0;
    int cell = 0;
    for (int l = 0; l < L; ++l) {
        const LevelGeom& lg = G.lv[l];
        EXPECT(lg.cell0 == cell && lg.candBase == slotEnd && lg.rows * lg.cols >= 1);
        for (int i = 0; i < lg.rows * lg.cols; ++i, ++cell) {
            const CellGeom& k = P.cells[cell];
            EXPECT(k.level == l);
            if (!k.skipped) EXPECT(k.x0 >= 0 && k.y0 >= 0 && k.hx > 0 && k.hy > 0 && k.x0 + k.hx <= lg.w && k.y0 + k.hy <= lg.h);
            EXPECT(k.cap >= 0 && k.cap <= lg.capMax);
            EXPECT(k.candOff == slotEnd);  // the slots before it end where its own begin
            slotEnd += lg.capMax;
        }
    }
    EXPECT(cell == G.nCells && slotEnd == G.candPerFrame);
    // kpBase is the running sum of nDesired
    int kp = 0;
    for (int l = 0; l < L; ++l) {
        EXPECT(G.lv[l].kpBase == kp && G.lv[l].nDesired == r.prm.nDesired[l]);
        for (int k = 0; k < G.lv[l].nDesired; ++k) EXPECT(P.slotLvl[kp + k] == l);
        kp += G.lv[l].nDesired;
    }
    EXPECT(kp == G.kpCap && kp == r.prm.kpCap && P.slotLvl.size() >= (size_t)kp);
    // FAST tiles cover [16, detX1) x [16, detY1) of each level exactly once
    for (int l = 0; l < L; ++l) {
        const LevelGeom& lg = G.lv[l];
        const int dw = lg.detX1 - 16, dh = lg.detY1 - 16;
        EXPECT(dw > 0 && dh > 0);
        std::vector<uint8_t> seen((size_t)dw * dh, 0);
        for (const FastTile& t : P.tiles) {
            if (t.level != l) continue;
            EXPECT(t.x0 >= 16 && t.y0 >= 16 && t.th >= 1 && t.tw4 >= 2 && t.x0 < lg.detX1 && t.y0 + t.th <= lg.detY1);
            for (int y = t.y0; y < t.y0 + t.th; ++y)
                for (int x = t.x0; x < std::min(t.x0 + 4 * t.tw4, lg.detX1); ++x) EXPECT(seen[(size_t)(y - 16) * dw + x - 16]++ == 0);
            // the tile's reciprocals divide exactly over the index ranges the kernel uses
            for (uint32_t i = 0; i < (uint32_t)((t.tw4 + 2) * (t.th + 2)); ++i) EXPECT(umulhi(i, t.rcpF) == i / (t.tw4 + 2));
            for (uint32_t i = 0; i < (uint32_t)(t.tw4 * t.th); ++i) EXPECT(umulhi(i, t.rcpI) == i / t.tw4);
            for (uint32_t i = 0; i < (uint32_t)((t.sp >> 4) * (t.th + 8)); ++i) EXPECT(umulhi(i, t.rcpU) == i / (t.sp >> 4));
        }
        EXPECT(std::count(seen.begin(), seen.end(), 1) == (long)seen.size());
        // corner -> cell bucket: n / cell by multiply-high for n < 4096 (a 1-px cell: 2^32 - 1 applied to n + 1)
        for (uint32_t n = 0; n < 4096; ++n) {
            EXPECT((lg.cellW == 1 ? umulhi(n + 1, (uint32_t)lg.cellWm) : umulhi(n, (uint32_t)lg.cellWm)) == n / lg.cellW);
            EXPECT((lg.cellH == 1 ? umulhi(n + 1, (uint32_t)lg.cellHm) : umulhi(n, (uint32_t)lg.cellHm)) == n / lg.cellH);
        }
    }
    {  // k_orient_desc's block decode over its whole grid
        const uint32_t gx = (uint32_t)((std::max(G.kpCap, 1) + OD_WAVES - 1) / OD_WAVES);
        for (uint32_t i = 0; i < gx * (uint32_t)c.max_batch; ++i) EXPECT(umulhi(i, G.odDivMagic) == i / gx);
    }
    if (!P.streamOk) return 0;
    const StreamGeom& sg = P.sgeom;
    const int K0 = P.streamK0;
    EXPECT(sg.L == L && (int)P.streamRounds.size() == sg.nRounds * (L + 2) && P.streamRows.size() % 8 == 0);
    // sum(nWaves) <= 14, the planned LDS <= PS_LDS_TARGET
    int ws = PS_LOADERS;
    for (int l = 0; l < L; ++l) {
        EXPECT(P.streamLv[l].waveStart == ws && P.streamLv[l].nWaves >= 1);
        ws += P.streamLv[l].nWaves;
    }
    EXPECT(ws - PS_LOADERS <= 14 && ws <= PS_THREADS / 64);
    EXPECT(P.streamLds <= (size_t)PS_LDS_TARGET);
    size_t ring = 0;
    for (int l = 0; l + 1 < L; ++l) {
        EXPECT(P.streamLv[l].ringOff == (int)ring && P.streamLv[l].ringPitch >= G.lv[l].w);
        ring += (size_t)P.streamCap[l] * P.streamLv[l].ringPitch;
    }
    EXPECT(sg.colOff == (int)ring && ring + (((size_t)sg.colWords * 4 + 15) & ~(size_t)15) == P.streamLds);
    EXPECT(sg.cap0 == P.streamCap[0] && (int)P.streamCol.size() == sg.colWords);
    // every row of every level appears in exactly one round, and a row's two source rows lie within
    // the previous level's ring window of that round
    std::vector<std::vector<int>> rounds_of(L);
    for (int l = 0; l < L; ++l) rounds_of[l].assign(G.lv[l].h, 0);
    std::vector<int> next(L, 0);
    size_t entry = 0;
    for (int n = 0; n < sg.nRounds; ++n) {
        const uint32_t* rw = &P.streamRounds[(size_t)n * (L + 2)];
        std::vector<int> lo(L), cnt(L);
        int ne = 0;
        for (int l = 0; l < L; ++l) {
            lo[l] = rw[l] & 0xFFF;
            cnt[l] = (rw[l] >> 12) & 0x3F;
            EXPECT((int)(rw[l] >> 18) == ne && lo[l] == next[l]);
            ne += cnt[l];
            // the magic division of the level's tasks in this round
            for (uint32_t i = 0; i < (uint32_t)(cnt[l] * P.streamLv[l].nq); ++i)
                EXPECT(umulhi(i, P.streamLv[l].nqm) == i / (uint32_t)P.streamLv[l].nq);
        }
        EXPECT(rw[L] == entry / 8 && (int)rw[L + 1] == ne && ne <= sg.rowStride);
        EXPECT(cnt[0] <= K0 && cnt[0] * sg.u0 <= PS_NPF * 64 * PS_LOADERS);
        for (uint32_t i = 0; i < (uint32_t)(cnt[0] * sg.u0); ++i) EXPECT(umulhi(i, sg.u0m) == i / (uint32_t)sg.u0);
        for (int l = 0; l < L; ++l)
            for (int dy = lo[l]; dy < lo[l] + cnt[l]; ++dy, entry += 8) {
                EXPECT(dy < G.lv[l].h && entry + 8 <= P.streamRows.size());
                ++rounds_of[l][dy];
                const uint32_t* e = &P.streamRows[entry];
                const LevelGeom& lg = G.lv[l];
                EXPECT(e[5] == (uint32_t)((dy + 16) * lg.pitch));
                const uint32_t own = l + 1 < L ? (uint32_t)(P.streamLv[l].ringOff + dy % P.streamCap[l] * P.streamLv[l].ringPitch) : ~0u;
                EXPECT(e[l == 0 ? 0 : 4] == own);
                if (l == 0) continue;
                // the level's source rows, from OpenCV's yofs of the resize table
                const int hs = G.lv[l - 1].h, yo = P.rtab[lg.rtab + 2 * lg.w + dy];
                const int s0 = clampi(yo, 0, hs - 1), s1 = clampi(yo + 1, 0, hs - 1);
                // rows of level l-1 ready when this round starts (level 0: the loaders brought this round's too)
                const int avail = l == 1 ? lo[0] + cnt[0] : lo[l - 1];
                // newest row the ring of level l-1 receives during this round (level 0: the next round's rows)
                const int newest = (l == 1 ? std::min(lo[0] + cnt[0] + K0, G.lv[0].h) : lo[l - 1] + cnt[l - 1]) - 1;
                const int cap = P.streamCap[l - 1];
                EXPECT(s1 < avail && s0 <= s1 && s0 > newest - cap);
                const StreamLevel& ps = P.streamLv[l - 1];
                EXPECT(e[0] == (uint32_t)(ps.ringOff + s0 % cap * ps.ringPitch));
                EXPECT(e[1] == (uint32_t)(ps.ringOff + s1 % cap * ps.ringPitch));
            }
        for (int l = 0; l < L; ++l) next[l] += cnt[l];
    }
    EXPECT(entry == P.streamRows.size());
    for (int l = 0; l < L; ++l)
        EXPECT(std::count(rounds_of[l].begin(), rounds_of[l].end(), 1) == (long)rounds_of[l].size());
    return 0;
}

}  // namespace

extern "C" {

// The golden line of a case into buf; its length, or -1 when buf is too small.
int extract_plan_describe(const char* name, const PlanCase* c, char* buf, int cap) {
    const Planned r = make(*c);
    const std::string s = extract_plan_line(name, *c, r.code, r.prm, r.plan);
    if ((int)s.size() + 1 > cap) return -1;
    memcpy(buf, s.c_str(), s.size() + 1);
    return (int)s.size();
}

// What the handle's getters answer (orb_get_level_info, orb_get_max_keypoints, orb_debug_pyramid_plan,
// orb_debug_pyramid_plan_levels): returns the status; arrays of 16; msg / why of 256 bytes.
int extract_plan_query(const PlanCase* c, char* msg, int* features_per_level, float* scale, int* max_keypoints,
                       int* stream, int* k0, int* rounds, int* lds, int* nq, int* n_waves, int* ring_rows, char* why) {
    const Planned r = make(*c);
    snprintf(msg, 256, "%s", r.err.c_str());
    snprintf(why, 256, "%s", r.plan.noStream);
    for (int l = 0; l < c->nl; ++l) {
        features_per_level[l] = r.prm.nDesired[l];
        scale[l] = r.prm.mvScaleFactor[l];
    }
    *max_keypoints = r.prm.kpCap;
    const ExtractPlan& P = r.plan;
    *stream = P.streamOk;
    *k0 = P.streamK0;
    *rounds = P.sgeom.nRounds;
    *lds = (int)P.streamLds;
    for (size_t l = 0; l < P.streamLv.size(); ++l) {
        nq[l] = P.streamLv[l].nq;
        n_waves[l] = P.streamLv[l].nWaves;
        ring_rows[l] = l + 1 < P.streamLv.size() ? P.streamCap[l] : 0;
    }
    return r.code;
}

int extract_plan_check_table_row(const PlanCase* c, int expect_plan, int k0) { return check_table_row(*c, expect_plan, k0); }

int extract_plan_check_invariants(const PlanCase* c) { return check_invariants(*c); }

// The refusals (code and text) and the two accepted neighbours.
int extract_plan_check_refusals() {
    for (const Refusal& f : REFUSALS) {
        const Planned r = make(f.c);
        EXPECT(r.code == ORB_ENOTSUP && r.err.find(f.text) != std::string::npos);
        EXPECT(r.plan.W == 0 && r.plan.H == 0 && r.plan.cells.empty() && !r.plan.streamOk);  // a refusal leaves no plan
    }
    const Planned one = make({640, 480, 1000, 1.2f, 1, 1, 20, 1, FT_CL});
    EXPECT(one.code == ORB_OK && !one.plan.streamOk && strstr(one.plan.noStream, "one level"));
    const Planned small = make({320, 240, 500, 1.2f, 8, 1, 20, 1, FT_CL});
    EXPECT(small.code == ORB_OK && small.plan.streamOk && small.plan.streamK0 == 32 && small.plan.sgeom.nRounds == 14);
    for (const PlanCase& c : {PlanCase{140, 134, 700, 1.1f, 15, 1, 20, 1, FT_CL}, PlanCase{160, 150, 800, 1.1f, 16, 1, 20, 1, FT_CL}}) {
        const Planned r = make(c);
        EXPECT(r.code == ORB_OK && !r.plan.streamOk);
        EXPECT(strstr(r.plan.noStream, "more levels than builder waves (L > PS_THREADS / 64 - PS_LOADERS = 14)"));
    }
    return 0;
}

}  // extern "C"

#ifdef EXTRACT_PLAN_HOST_MAIN
// extract_plan_host GOLDEN.json: the refusals, then every line of the golden file reproduced as text,
// its stream plan and K0 put to the table row's assertions, and the invariants.
int main(int argc, char** argv) {
    if (argc < 2) return 2;
    int status = extract_plan_check_refusals();
    if (status) printf("refusals: line %d\n", status);
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    std::vector<char> line(1 << 16);
    int cases = 0;
    while (!status && fgets(line.data(), (int)line.size(), f)) {
        std::string s = line.data();
        while (!s.empty() && (s.back() == '\n' || s.back() == ',' || s.back() == ' ')) s.pop_back();
        if (s.rfind("{\"name\"", 0) != 0) continue;
        char name[128];
        PlanCase c{};
        int code = 0, stream = 0, k0 = 0;
        if (sscanf(s.c_str(),
                   "{\"name\": \"%127[^\"]\", \"w\": %d, \"h\": %d, \"nf\": %d, \"sf\": %f, \"nl\": %d, \"score\": %d, "
                   "\"fast_th\": %d, \"max_batch\": %d, \"fast_cl\": %d, \"code\": %d, \"stream\": %d, \"k0\": %d",
                   name, &c.w, &c.h, &c.nf, &c.sf, &c.nl, &c.score, &c.fast_th, &c.max_batch, &c.fast_cl, &code, &stream,
                   &k0) != 13) {
            printf("unreadable line: %s\n", s.c_str());
            status = __LINE__;
            break;
        }
        ++cases;
        const Planned r = make(c);
        if (extract_plan_line(name, c, r.code, r.prm, r.plan) != s) {
            printf("%s: the planner's answer differs from the recorded line\n", name);
            status = __LINE__;
        } else if (int e = check_table_row(c, stream, k0)) {
            printf("%s: table row, line %d\n", name, e);
            status = e;
        } else if (int e = check_invariants(c)) {
            printf("%s: invariants, line %d\n", name, e);
            status = e;
        }
    }
    fclose(f);
    if (!status && cases < 118) status = __LINE__;
    printf("%d geometries, status %d\n", cases, status);
    return status != 0;
}
#endif
