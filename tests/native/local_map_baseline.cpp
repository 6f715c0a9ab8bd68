// local_map_baseline.cpp — the single-threaded CPU baseline of scripts/local_map_timing.py:
// Tracking::UpdateReferenceKeyFrames, UpdateReferencePoints and the "already matched" pass of
// SearchReferencePointsInFrustum with the reference's own containers (std::map keyed by keyframe,
// std::vector, per-object stamps), over the flat tables of include/orb_abi.h.  Keyframe and point objects
// are built once (local_map_baseline_create), as the reference's map exists before a frame arrives; a
// call does what the reference does per frame.  A keyframe's address order is its index order.
#include <stddef.h>
#include <stdint.h>

#include <map>
#include <vector>

namespace {

struct KeyFrame;
struct MapPoint {
    int id;
    bool bad;
    std::map<KeyFrame*, size_t> observations;
    long trackReferenceForFrame = -1, lastFrameSeen = -1;
};
struct KeyFrame {
    int id;
    bool bad;
    std::vector<MapPoint*> mapPoints;
    std::vector<KeyFrame*> covisible;  // GetBestCovisibilityKeyFrames(10)
    long trackReferenceForFrame = -1;
};
struct World {
    std::vector<KeyFrame> kfs;  // contiguous: pointer order is index order
    std::vector<MapPoint> pts;
    long frameId = 0;
};

}  // namespace

extern "C" {

void* local_map_baseline_create(int n_kf, int n_pt, const uint8_t* kf_bad, const int32_t* kf_mp_off, const int32_t* kf_mp,
                                const int32_t* kf_cov, const uint8_t* pt_bad, const int32_t* pt_obs_off,
                                const int32_t* pt_obs_kf) {
    World* W = new World;
    W->kfs.resize(n_kf);
    W->pts.resize(n_pt);
    for (int p = 0; p < n_pt; ++p) {
        W->pts[p].id = p, W->pts[p].bad = pt_bad[p] != 0;
        for (int e = pt_obs_off[p]; e < pt_obs_off[p + 1]; ++e) W->pts[p].observations[&W->kfs[pt_obs_kf[e]]] = 0;
    }
    for (int k = 0; k < n_kf; ++k) {
        KeyFrame& K = W->kfs[k];
        K.id = k, K.bad = kf_bad[k] != 0;
        for (int e = kf_mp_off[k]; e < kf_mp_off[k + 1]; ++e) K.mapPoints.push_back(kf_mp[e] < 0 ? nullptr : &W->pts[kf_mp[e]]);
        for (int c = 0; c < 10 && kf_cov[k * 10 + c] >= 0; ++c) K.covisible.push_back(&W->kfs[kf_cov[k * 10 + c]]);
    }
    return W;
}

void local_map_baseline_destroy(void* w) { delete (World*)w; }

// One frame.  out[0 .. 5] = n_voted, n_local_kf, ref_kf, ref_votes, n_local_pt, n_cleared; the lists are
// written when they fit their capacities.
void local_map_baseline_reference(void* w, int n, const int32_t* f_mp, int32_t* f_mp_out, int cap_kf, int32_t* local_kf,
                                  int cap_pt, int32_t* local_pt, uint8_t* local_pt_seen, int32_t* out) {
    World& W = *(World*)w;
    const long mnId = ++W.frameId;
    std::vector<MapPoint*> frame(n);
    for (int i = 0; i < n; ++i) frame[i] = f_mp[i] < 0 ? nullptr : &W.pts[f_mp[i]];
    int cleared = 0;

    std::map<KeyFrame*, int> keyframeCounter;
    for (size_t i = 0, iend = frame.size(); i < iend; i++) {
        if (frame[i]) {
            MapPoint* pMP = frame[i];
            if (!pMP->bad) {
                std::map<KeyFrame*, size_t> observations = pMP->observations;
                for (std::map<KeyFrame*, size_t>::iterator it = observations.begin(), itend = observations.end(); it != itend; it++)
                    keyframeCounter[it->first]++;
            } else {
                frame[i] = nullptr;
                ++cleared;
            }
        }
    }
    int max = 0;
    KeyFrame* pKFmax = nullptr;
    std::vector<KeyFrame*> localKFs;
    localKFs.reserve(3 * keyframeCounter.size());
    for (std::map<KeyFrame*, int>::iterator it = keyframeCounter.begin(), itEnd = keyframeCounter.end(); it != itEnd; it++) {
        KeyFrame* pKF = it->first;
        if (pKF->bad) continue;
        if (it->second > max) {
            max = it->second;
            pKFmax = pKF;
        }
        localKFs.push_back(it->first);
        pKF->trackReferenceForFrame = mnId;
    }
    const int n_voted = (int)localKFs.size();
    for (std::vector<KeyFrame*>::iterator itKF = localKFs.begin(), itEndKF = localKFs.end(); itKF != itEndKF; itKF++) {
        if (localKFs.size() > 80) break;
        KeyFrame* pKF = *itKF;
        std::vector<KeyFrame*> vNeighs = pKF->covisible;
        for (std::vector<KeyFrame*>::iterator itN = vNeighs.begin(), itEndN = vNeighs.end(); itN != itEndN; itN++) {
            KeyFrame* pNeighKF = *itN;
            if (!pNeighKF->bad) {
                if (pNeighKF->trackReferenceForFrame != mnId) {
                    localKFs.push_back(pNeighKF);
                    pNeighKF->trackReferenceForFrame = mnId;
                    break;
                }
            }
        }
    }
    std::vector<MapPoint*> localPts;
    for (std::vector<KeyFrame*>::iterator itKF = localKFs.begin(), itEndKF = localKFs.end(); itKF != itEndKF; itKF++) {
        KeyFrame* pKF = *itKF;
        std::vector<MapPoint*> vpMPs = pKF->mapPoints;
        for (std::vector<MapPoint*>::iterator itMP = vpMPs.begin(), itEndMP = vpMPs.end(); itMP != itEndMP; itMP++) {
            MapPoint* pMP = *itMP;
            if (!pMP) continue;
            if (pMP->trackReferenceForFrame == mnId) continue;
            if (!pMP->bad) {
                localPts.push_back(pMP);
                pMP->trackReferenceForFrame = mnId;
            }
        }
    }
    for (std::vector<MapPoint*>::iterator vit = frame.begin(), vend = frame.end(); vit != vend; vit++) {
        MapPoint* pMP = *vit;
        if (pMP) {
            if (pMP->bad) *vit = nullptr;
            else pMP->lastFrameSeen = mnId;
        }
    }
    out[0] = n_voted, out[1] = (int)localKFs.size(), out[2] = pKFmax ? pKFmax->id : -1, out[3] = max;
    out[4] = (int)localPts.size(), out[5] = cleared;
    for (int i = 0; i < n; ++i) f_mp_out[i] = frame[i] ? frame[i]->id : -1;
    if ((int)localKFs.size() <= cap_kf)
        for (size_t j = 0; j < localKFs.size(); ++j) local_kf[j] = localKFs[j]->id;
    if ((int)localPts.size() <= cap_pt)
        for (size_t j = 0; j < localPts.size(); ++j) {
            local_pt[j] = localPts[j]->id;
            local_pt_seen[j] = localPts[j]->lastFrameSeen == mnId ? 1 : 0;
        }
}

}  // extern "C"
