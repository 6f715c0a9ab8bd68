// kfdb_baseline.cpp — the CPU baseline of scripts/kfdb_timing.py: a single-threaded
// inverted-file keyframe database in the reference's shape (a std::list of keyframes per word,
// per-keyframe query / words / score fields, std::map BowVectors scored by the L1 walk), compiled
// -O3 into build/libkfdb_baseline.so.  Measurement infrastructure: the product never loads it.
// Its candidate lists must equal the kernels' (the timing script checks that before it times).
#include <cmath>
#include <cstdint>
#include <list>
#include <map>
#include <set>
#include <utility>
#include <vector>

namespace {

typedef std::map<unsigned, double> Bow;

struct KF {
    int id = 0;
    Bow bow;
    std::vector<KF*> neighbours;
    long query = -1;
    int words = 0;
    float score = 0.0f;
};

struct DB {
    std::vector<std::list<KF*> > inverted;
    std::map<int, KF*> kfs;
    long nquery = 0;
    ~DB() {
        for (std::map<int, KF*>::iterator it = kfs.begin(); it != kfs.end(); ++it) delete it->second;
    }
};

double l1(const Bow& v1, const Bow& v2) {
    Bow::const_iterator a = v1.begin(), b = v2.begin();
    double score = 0;
    while (a != v1.end() && b != v2.end()) {
        if (a->first == b->first) {
            const double vi = a->second, wi = b->second;
            score += std::fabs(vi - wi) - std::fabs(vi) - std::fabs(wi);
            ++a;
            ++b;
        } else if (a->first < b->first) {
            a = v1.lower_bound(b->first);
        } else {
            b = v2.lower_bound(a->first);
        }
    }
    return -score / 2.0;
}

}  // namespace

extern "C" {

void* kfb_create(int n_words) {
    DB* db = new DB();
    db->inverted.resize((size_t)n_words);
    return db;
}

void kfb_destroy(void* h) { delete (DB*)h; }

void kfb_add(void* h, int id, const uint32_t* w, const double* v, int n) {
    DB* db = (DB*)h;
    KF* kf = new KF();
    kf->id = id;
    for (int i = 0; i < n; ++i) kf->bow[w[i]] = v[i];
    db->kfs[id] = kf;
    for (Bow::const_iterator it = kf->bow.begin(); it != kf->bow.end(); ++it) db->inverted[it->first].push_back(kf);
}

void kfb_set_covisible(void* h, int id, const int32_t* nb, int n) {
    DB* db = (DB*)h;
    KF* kf = db->kfs.at(id);
    kf->neighbours.clear();
    for (int i = 0; i < n; ++i) {
        std::map<int, KF*>::iterator it = db->kfs.find(nb[i]);
        if (it != db->kfs.end()) kf->neighbours.push_back(it->second);
    }
}

// Relocalisation candidates of one query; returns their number (ids in out, at most cap written).
int kfb_reloc(void* h, const uint32_t* w, const double* v, int n, int32_t* out, int cap) {
    DB* db = (DB*)h;
    Bow q;
    for (int i = 0; i < n; ++i) q[w[i]] = v[i];
    const long fid = ++db->nquery;
    std::list<KF*> sharing;
    for (Bow::const_iterator it = q.begin(); it != q.end(); ++it) {
        std::list<KF*>& l = db->inverted[it->first];
        for (std::list<KF*>::iterator lit = l.begin(); lit != l.end(); ++lit) {
            KF* kf = *lit;
            if (kf->query != fid) {
                kf->words = 0;
                kf->query = fid;
                sharing.push_back(kf);
            }
            kf->words++;
        }
    }
    if (sharing.empty()) return 0;
    int maxCommon = 0;
    for (std::list<KF*>::iterator it = sharing.begin(); it != sharing.end(); ++it)
        if ((*it)->words > maxCommon) maxCommon = (*it)->words;
    const int minCommon = maxCommon * 0.8f;
    std::list<std::pair<float, KF*> > scored;
    for (std::list<KF*>::iterator it = sharing.begin(); it != sharing.end(); ++it) {
        KF* kf = *it;
        if (kf->words > minCommon) {
            const float si = l1(q, kf->bow);
            kf->score = si;
            scored.push_back(std::make_pair(si, kf));
        }
    }
    if (scored.empty()) return 0;
    std::list<std::pair<float, KF*> > acc;
    float bestAcc = 0;
    for (std::list<std::pair<float, KF*> >::iterator it = scored.begin(); it != scored.end(); ++it) {
        KF* kf = it->second;
        float best = it->first, sum = best;
        KF* bestKF = kf;
        for (size_t j = 0; j < kf->neighbours.size(); ++j) {
            KF* k2 = kf->neighbours[j];
            if (k2->query != fid) continue;
            sum += k2->score;
            if (k2->score > best) {
                bestKF = k2;
                best = k2->score;
            }
        }
        acc.push_back(std::make_pair(sum, bestKF));
        if (sum > bestAcc) bestAcc = sum;
    }
    const float retain = 0.75f * bestAcc;
    std::set<KF*> seen;
    int m = 0;
    for (std::list<std::pair<float, KF*> >::iterator it = acc.begin(); it != acc.end(); ++it)
        if (it->first > retain && !seen.count(it->second)) {
            if (m < cap) out[m] = it->second->id;
            ++m;
            seen.insert(it->second);
        }
    return m;
}

}  // extern "C"
