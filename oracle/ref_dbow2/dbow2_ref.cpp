// dbow2_ref.cpp — TEST INFRASTRUCTURE ONLY, our own text.
//
// Command-line driver around the reference's own DBoW2 (TemplatedVocabulary<FORB::TDescriptor,
// FORB>, BowVector, FeatureVector, ScoringObject, FORB), compiled unmodified from the reference
// tree against the opencv/cv.h stand-in beside this file.  scripts/gen_ref_dbow2_golden.py runs
// it to record the fixtures tests/golden/ref_dbow2_*.npz; tests/test_ref_dbow2.py reruns it to
// check that they have not drifted.  Every number crosses the process boundary as raw
// little-endian bytes (u32 / i32 / f64), never as decimal text.
//
//   dbow2_ref load+transform VOC DESC COUNTS LEVELSUPS OUT
//       VOC: vocabulary text file; DESC: raw 32-byte descriptors, the frames one after the
//       other; COUNTS / LEVELSUPS: comma-separated.  For every frame, for every levelsup, OUT
//       gets one record:
//         u32 nb, u32 word[nb], f64 value[nb]                    BowVector, map order
//         u32 nf, u32 node[nf], u32 count[nf], u32 feature[sum]  FeatureVector, map order
//         u32 n,  u32 word[n],  f64 weight[n], u32 nid[n]        single-feature overload
//       nid is set to 0xFFFFFFFF before each single-feature call, so a call that leaves it
//       unwritten shows.
//   dbow2_ref score VOC BOWS PAIRS OUT
//       BOWS: u32 B, then B x (u32 n, u32 word[n], f64 value[n]); PAIRS: u32 P, then
//       P x (u32 a, u32 b); OUT: f64 score[P] = voc.score(bow a, bow b).
//   dbow2_ref distance PAIRS OUT
//       PAIRS: rows of 64 bytes (descriptor a, descriptor b); OUT: i32 FORB::distance per row.
//   dbow2_ref resave VOC OUT
//       loadFromTextFile, then saveToTextFile.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "FORB.h"
#include "TemplatedVocabulary.h"

namespace {

typedef DBoW2::TemplatedVocabulary<DBoW2::FORB::TDescriptor, DBoW2::FORB> Base;

struct Voc : Base {
    // the single-feature overload is protected in the reference
    void one(const cv::Mat& f, DBoW2::WordId& id, DBoW2::WordValue& w, DBoW2::NodeId* nid, int levelsup) const {
        Base::transform(f, id, w, nid, levelsup);
    }
};

[[noreturn]] void die(const std::string& msg) {
    std::fprintf(stderr, "dbow2_ref: %s\n", msg.c_str());
    std::exit(2);
}

std::vector<unsigned char> slurp(const char* path) {
    std::ifstream f(path, std::ios::binary);
    if (!f.is_open()) die(std::string("cannot open ") + path);
    return std::vector<unsigned char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

struct Out {
    FILE* fp;
    explicit Out(const char* path) : fp(std::fopen(path, "wb")) {
        if (!fp) die(std::string("cannot write ") + path);
    }
    ~Out() {
        if (std::fclose(fp) != 0) die("write failed");
    }
    template <class T> void put(const T& x) {
        if (std::fwrite(&x, sizeof(T), 1, fp) != 1) die("write failed");
    }
};

struct In {
    std::vector<unsigned char> buf;
    size_t pos;
    explicit In(const char* path) : buf(slurp(path)), pos(0) {}
    template <class T> T get() {
        if (pos + sizeof(T) > buf.size()) die("input file is truncated");
        T x;
        std::memcpy(&x, buf.data() + pos, sizeof(T));
        pos += sizeof(T);
        return x;
    }
};

std::vector<int> ints(const char* s) {
    std::vector<int> v;
    std::stringstream ss(s);
    std::string tok;
    while (std::getline(ss, tok, ','))
        if (!tok.empty()) v.push_back(std::atoi(tok.c_str()));
    return v;
}

cv::Mat row(const unsigned char* p) {
    cv::Mat m;
    m.create(1, 32, CV_8U);
    std::memcpy(m.ptr<unsigned char>(), p, 32);
    return m;
}

void load(Voc& voc, const char* path) {
    std::ifstream probe(path);
    if (!probe.is_open()) die(std::string("cannot open ") + path);
    probe.close();
    if (!voc.loadFromTextFile(path)) die(std::string("loadFromTextFile refused ") + path);
}

int cmd_load_transform(char** a) {
    Voc voc;
    load(voc, a[0]);
    const std::vector<unsigned char> desc = slurp(a[1]);
    const std::vector<int> counts = ints(a[2]), levels = ints(a[3]);
    size_t total = 0;
    for (size_t i = 0; i < counts.size(); ++i) total += (size_t)counts[i];
    if (desc.size() != total * 32) die("DESC does not hold the rows that COUNTS names");
    Out out(a[4]);
    size_t first = 0;
    for (size_t fi = 0; fi < counts.size(); first += (size_t)counts[fi], ++fi) {
        std::vector<cv::Mat> feats;
        for (int i = 0; i < counts[fi]; ++i) feats.push_back(row(desc.data() + (first + (size_t)i) * 32));
        for (size_t li = 0; li < levels.size(); ++li) {
            DBoW2::BowVector bow;
            DBoW2::FeatureVector fv;
            voc.transform(feats, bow, fv, levels[li]);
            out.put((uint32_t)bow.size());
            for (DBoW2::BowVector::const_iterator it = bow.begin(); it != bow.end(); ++it) out.put((uint32_t)it->first);
            for (DBoW2::BowVector::const_iterator it = bow.begin(); it != bow.end(); ++it) out.put((double)it->second);
            out.put((uint32_t)fv.size());
            for (DBoW2::FeatureVector::const_iterator it = fv.begin(); it != fv.end(); ++it) out.put((uint32_t)it->first);
            for (DBoW2::FeatureVector::const_iterator it = fv.begin(); it != fv.end(); ++it)
                out.put((uint32_t)it->second.size());
            for (DBoW2::FeatureVector::const_iterator it = fv.begin(); it != fv.end(); ++it)
                for (size_t j = 0; j < it->second.size(); ++j) out.put((uint32_t)it->second[j]);
            std::vector<uint32_t> w(feats.size()), nid(feats.size());
            std::vector<double> wt(feats.size());
            for (size_t i = 0; i < feats.size(); ++i) {
                DBoW2::WordId id = 0xFFFFFFFFu;
                DBoW2::WordValue weight = -1.0;
                DBoW2::NodeId n = 0xFFFFFFFFu;
                voc.one(feats[i], id, weight, &n, levels[li]);
                w[i] = id;
                wt[i] = weight;
                nid[i] = n;
            }
            out.put((uint32_t)feats.size());
            for (size_t i = 0; i < feats.size(); ++i) out.put(w[i]);
            for (size_t i = 0; i < feats.size(); ++i) out.put(wt[i]);
            for (size_t i = 0; i < feats.size(); ++i) out.put(nid[i]);
        }
    }
    return 0;
}

int cmd_score(char** a) {
    Voc voc;
    load(voc, a[0]);
    In bows(a[1]), pairs(a[2]);
    const uint32_t B = bows.get<uint32_t>();
    std::vector<DBoW2::BowVector> v(B);
    for (uint32_t b = 0; b < B; ++b) {
        const uint32_t n = bows.get<uint32_t>();
        std::vector<uint32_t> words(n);
        for (uint32_t i = 0; i < n; ++i) words[i] = bows.get<uint32_t>();
        for (uint32_t i = 0; i < n; ++i) v[b].addWeight(words[i], bows.get<double>());
    }
    const uint32_t P = pairs.get<uint32_t>();
    Out out(a[3]);
    for (uint32_t p = 0; p < P; ++p) {
        const uint32_t x = pairs.get<uint32_t>(), y = pairs.get<uint32_t>();
        if (x >= B || y >= B) die("pair index out of range");
        out.put((double)voc.score(v[x], v[y]));
    }
    return 0;
}

int cmd_distance(char** a) {
    const std::vector<unsigned char> rows = slurp(a[0]);
    if (rows.size() % 64 != 0) die("PAIRS is not rows of 64 bytes");
    Out out(a[1]);
    for (size_t i = 0; i < rows.size(); i += 64)
        out.put((int32_t)DBoW2::FORB::distance(row(rows.data() + i), row(rows.data() + i + 32)));
    return 0;
}

int cmd_resave(char** a) {
    Voc voc;
    load(voc, a[0]);
    voc.saveToTextFile(a[1]);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "load+transform" && argc == 7) return cmd_load_transform(argv + 2);
    if (cmd == "score" && argc == 6) return cmd_score(argv + 2);
    if (cmd == "distance" && argc == 4) return cmd_distance(argv + 2);
    if (cmd == "resave" && argc == 4) return cmd_resave(argv + 2);
    std::fprintf(stderr,
                 "usage: dbow2_ref load+transform VOC DESC COUNTS LEVELSUPS OUT\n"
                 "       dbow2_ref score VOC BOWS PAIRS OUT\n"
                 "       dbow2_ref distance PAIRS OUT\n"
                 "       dbow2_ref resave VOC OUT\n");
    return 2;
}
