// orb_slam_gpu.hpp — header-only C++ facade re-exposing the reference's class API
// (ORB_SLAM::ORBextractor, include/ORBextractor.h:30-80; ORB_SLAM::ORBmatcher,
// include/ORBmatcher.h:36-108) on top of the C ABI in orb_abi.h (liborb_hip.so).
//
// Tracking / LocalMapping keep calling
//     (*mpORBextractor)(im, cv::Mat(), mvKeys, mDescriptors);                 // Frame.cc:60
//     ORBmatcher(0.9, true).SearchForInitialization(F1, F2, prev, m12, 100);  // Tracking.cc:392-393
// unchanged once Frame.cc / Tracking.cc include this header instead of ORBextractor.h and
// ORBmatcher.h and alias the classes.  With ORB_WITH_OPENCV defined the
// cv::InputArray / cv::KeyPoint overloads are available; without OpenCV the POD overloads
// are (std::vector<orb_keypoint_t>, row-major N x 32 descriptor bytes).
//
// gpu::KeyFrameDatabase re-exposes KeyFrameDatabase (include/KeyFrameDatabase.h:44-71) over
// keyframe ids, and gpu::score is mpVoc->score(...) (L1 vocabularies).  gpu::Initializer is the
// scoring half of Initializer (include/Initializer.h:31-97): FindHomography / FindFundamental over
// hypotheses the caller has computed, and Initialize up to the Reconstruct* call with the hypotheses
// computed on the device from the caller's rand() values.  gpu::PnPsolver and gpu::Sim3Solver are the consensus halves
// of PnPsolver (include/PnPsolver.h) and Sim3Solver (include/Sim3Solver.h): CheckInliers and the
// keep-the-best rule of iterate over poses the caller has computed.  gpu::Optimizer::PoseOptimization
// is Optimizer::PoseOptimization (include/Optimizer.h), the motion-only optimisation, whole, and
// gpu::Optimizer::OptimizeSim3 is Optimizer::OptimizeSim3, the 7-DoF optimisation of a loop candidate.
// gpu::LocalMapping is the arithmetic of LocalMapping::CreateNewMapPoints (ComputeF12, the triangulation
// and its gates) and MapPoint::UpdateNormalAndDepth.
//
// Error behaviour: the reference asserts on bad input (ORBextractor.cc:725) and has no
// status codes; the facade throws std::runtime_error carrying orb_last_error() for any
// non-OK status, and keeps the reference's early return on an empty image
// (ORBextractor.cc:721-722: outputs untouched).
#ifndef ORB_SLAM_GPU_HPP
#define ORB_SLAM_GPU_HPP

#include <algorithm>
#include <array>
#include <climits>
#include <cmath>
#include <cstdint>
#include <map>
#include <stdexcept>
#include <utility>
#include <string>
#include <vector>

#include "orb_abi.h"

#ifdef ORB_WITH_OPENCV
#include <opencv2/core/core.hpp>
#endif

namespace ORB_SLAM {
namespace gpu {

inline void orb_check(int st) {
    if (st < 0) throw std::runtime_error(std::string("orb: ") + orb_last_error() + " (status " + std::to_string(st) + ")");
}

class ORBextractor {
public:
    enum { HARRIS_SCORE = ORB_HARRIS_SCORE, FAST_SCORE = ORB_FAST_SCORE };

    ORBextractor(int nfeatures = 1000, float scaleFactor = 1.2f, int nlevels = 8, int scoreType = FAST_SCORE,
                 int fastTh = 20, int device = 0, int maxBatch = 1)
        : nlevels_(nlevels), scaleFactor_(scaleFactor) {
        orb_check(orb_extractor_create(nfeatures, scaleFactor, nlevels, scoreType, fastTh, device, maxBatch, &h_));
        cap_ = orb_get_max_keypoints(h_);
    }
    ~ORBextractor() { orb_extractor_destroy(h_); }
    ORBextractor(const ORBextractor&) = delete;
    ORBextractor& operator=(const ORBextractor&) = delete;

    // ORBextractor::operator() on a POD image (u8, w x h, row pitch `stride`).
    void operator()(const uint8_t* img, int w, int h, int stride, std::vector<orb_keypoint_t>& keypoints,
                    std::vector<uint8_t>& descriptors) {
        if (w <= 0 || h <= 0) return;  // _image.empty(): outputs untouched
        keypoints.resize(cap_);
        descriptors.resize((size_t)cap_ * 32);
        int n = 0;
        orb_check(orb_extract(h_, img, w, h, stride, keypoints.data(), cap_, descriptors.data(), &n));
        keypoints.resize(n);
        descriptors.resize((size_t)n * 32);  // n == 0: the reference's _descriptors.release()
    }

#ifdef ORB_WITH_OPENCV
    // The reference signature (ORBextractor.h:43-45).  The mask is ignored, as by the
    // reference's FAST (ORBextractor.cc:601-607).
    void operator()(cv::InputArray _image, cv::InputArray /*mask*/, std::vector<cv::KeyPoint>& _keypoints,
                    cv::OutputArray _descriptors) {
        if (_image.empty()) return;
        cv::Mat image = _image.getMat();
        CV_Assert(image.type() == CV_8UC1);
        std::vector<orb_keypoint_t> k;
        std::vector<uint8_t> d;
        (*this)(image.data, image.cols, image.rows, (int)image.step, k, d);
        _keypoints.clear();
        _keypoints.reserve(k.size());
        for (const orb_keypoint_t& p : k)
            _keypoints.push_back(cv::KeyPoint(p.x, p.y, p.size, p.angle, p.response, p.octave, p.class_id));
        if (k.empty()) {
            _descriptors.release();
        } else {
            _descriptors.create((int)k.size(), 32, CV_8U);
            cv::Mat D = _descriptors.getMat();
            for (size_t i = 0; i < k.size(); ++i) std::copy(&d[i * 32], &d[i * 32] + 32, D.ptr<uint8_t>((int)i));
        }
    }
#endif

    int inline GetLevels() { return nlevels_; }
    float inline GetScaleFactor() { return scaleFactor_; }
    orb_extractor_t* handle() { return h_; }

private:
    orb_extractor_t* h_ = nullptr;
    int nlevels_;
    float scaleFactor_;
    int cap_ = 0;
};

// The matcher-facing part of ORB_SLAM::Frame (Frame.h:43-138) for the POD overloads.
struct FrameView {
    const orb_keypoint_t* keysUn;  // mvKeysUn
    const uint8_t* descriptors;    // mDescriptors, N x 32
    int N;
    orb_frame_bounds_t bounds;     // mnMinX, mnMaxX, mnMinY, mnMaxY (static, first frame)
};

class ORBmatcher {
public:
    static const int TH_LOW = 50, TH_HIGH = 100, HISTO_LENGTH = 30;  // ORBmatcher.cc:40-42

    ORBmatcher(float nnratio = 0.6f, bool checkOri = true) : mfNNratio(nnratio), mbCheckOrientation(checkOri) {}

    static int DescriptorDistance(const uint8_t* a, const uint8_t* b) { return orb_descriptor_distance(a, b); }

    // SearchForInitialization (ORBmatcher.cc:598-713): vbPrevMatched is N1 x {x, y}.
    int SearchForInitialization(const FrameView& F1, const FrameView& F2, std::vector<float>& vbPrevMatched,
                                std::vector<int>& vnMatches12, int windowSize = 10) {
        vnMatches12.assign(F1.N, -1);
        int n = 0;
        orb_check(orb_search_for_initialization(F1.keysUn, F1.descriptors, F1.N, F2.keysUn, F2.descriptors, F2.N,
                                                F1.bounds, mfNNratio, mbCheckOrientation ? 1 : 0, windowSize,
                                                vbPrevMatched.data(), vnMatches12.data(), &n));
        return n;
    }

    // ---- the rest of the family over POD views (orb_abi.h documents every flag array).
    // Outputs are indices: the caller maps them back to MapPoint* exactly where the
    // reference assigns (vpMapPointMatches[j] = pMP ...).

    // SearchByBoW(KeyFrame*, Frame&, vpMapPointMatches) (ORBmatcher.cc:155-284):
    // vpMapPointMatches[j] = KF keypoint index whose MapPoint matched F keypoint j, or -1.
    int SearchByBoW(const orb_frame_view_t& KF, const uint8_t* kfUsable, const orb_feature_vector_t& kfFV,
                    const orb_frame_view_t& F, const orb_feature_vector_t& fFV, std::vector<int>& vpMapPointMatches,
                    int device = 0) {
        vpMapPointMatches.assign(F.n, -1);
        int n = 0;
        orb_check(orb_search_by_bow_kf_f(&KF, kfUsable, kfFV, &F, fFV, mfNNratio, mbCheckOrientation, vpMapPointMatches.data(), &n, device));
        return n;
    }
    // SearchByBoW(KeyFrame*, KeyFrame*, vpMatches12) (ORBmatcher.cc:715-850).
    int SearchByBoW(const orb_frame_view_t& KF1, const uint8_t* usable1, const orb_feature_vector_t& fv1,
                    const orb_frame_view_t& KF2, const uint8_t* usable2, const orb_feature_vector_t& fv2,
                    std::vector<int>& vpMatches12, int device = 0) {
        vpMatches12.assign(KF1.n, -1);
        int n = 0;
        orb_check(orb_search_by_bow_kf_kf(&KF1, usable1, fv1, &KF2, usable2, fv2, mfNNratio, mbCheckOrientation, vpMatches12.data(), &n, device));
        return n;
    }
    // SearchForTriangulation (ORBmatcher.cc:852-1014): vMatchedPairs (i1, i2) ascending in i1.
    int SearchForTriangulation(const orb_frame_view_t& KF1, const uint8_t* hasMP1, const orb_feature_vector_t& fv1,
                               const orb_frame_view_t& KF2, const uint8_t* hasMP2, const orb_feature_vector_t& fv2,
                               const float F12[9], std::vector<std::pair<size_t, size_t> >& vMatchedPairs,
                               int device = 0) {
        std::vector<int> m12(KF1.n, -1);
        int n = 0;
        orb_check(orb_search_for_triangulation(&KF1, hasMP1, fv1, &KF2, hasMP2, fv2, F12, mfNNratio, mbCheckOrientation, m12.data(), &n, device));
        vMatchedPairs.clear();
        for (int i = 0; i < KF1.n; ++i)
            if (m12[i] >= 0) vMatchedPairs.push_back(std::make_pair((size_t)i, (size_t)m12[i]));
        return n;
    }
    // WindowSearch (ORBmatcher.cc:409-516): vpMapPointMatches2[i2] = F1 index or -1.
    int WindowSearch(const orb_frame_view_t& F1, const uint8_t* usable1, const orb_frame_view_t& F2, int windowSize,
                     std::vector<int>& vpMapPointMatches2, int minScaleLevel = 0, int maxScaleLevel = INT_MAX,
                     int device = 0) {
        vpMapPointMatches2.assign(F2.n, -1);
        int n = 0;
        orb_check(orb_window_search(&F1, usable1, &F2, windowSize, minScaleLevel, maxScaleLevel, mfNNratio, mbCheckOrientation, vpMapPointMatches2.data(), &n, device));
        return n;
    }
    // SearchByProjection(Frame& F, vector<MapPoint*>, th) (ORBmatcher.cc:49-125) over the
    // isInFrustum fields; newMatches[j] = MapPoint row assigned to F keypoint j, or -1.
    int SearchByProjection(const orb_frame_view_t& F, const uint8_t* fTaken, int nMP, const uint8_t* usable,
                           const float* projX, const float* projY, const int32_t* level, const float* viewCos,
                           const uint8_t* mpDesc, float th, std::vector<int>& newMatches, int device = 0) {
        newMatches.assign(F.n, -1);
        int n = 0;
        orb_check(orb_search_by_projection_local(&F, fTaken, nMP, usable, projX, projY, level, viewCos, mpDesc, th, mfNNratio, newMatches.data(), &n, device));
        return n;
    }
    // SearchByProjection(Frame& F1, Frame& F2, windowSize, vpMapPointMatches2) (519-594).
    int SearchByProjection(const orb_frame_view_t& F1, const orb_map_points_t& mp1, const uint8_t* usable1,
                           const orb_frame_view_t& F2, const uint8_t* f2Taken, int windowSize,
                           std::vector<int>& newMatches2, int device = 0) {
        newMatches2.assign(F2.n, -1);
        int n = 0;
        orb_check(orb_search_by_projection_f2f(&F1, mp1, usable1, &F2, f2Taken, windowSize, mfNNratio, newMatches2.data(), &n, device));
        return n;
    }
    // SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th) (1507-1620).
    int SearchByProjection(const orb_frame_view_t& Cur, const uint8_t* curTaken, const orb_frame_view_t& Last,
                           const orb_map_points_t& mp, const uint8_t* usable, float th, std::vector<int>& newMatches,
                           int device = 0) {
        newMatches.assign(Cur.n, -1);
        int n = 0;
        orb_check(orb_search_by_projection_motion(&Cur, curTaken, &Last, mp, usable, th, mbCheckOrientation, newMatches.data(), &n, device));
        return n;
    }
    // SearchByProjection(Frame& CurrentFrame, KeyFrame*, sAlreadyFound, th, ORBdist) (1622-1746).
    int SearchByProjection(const orb_frame_view_t& Cur, const uint8_t* curTaken, const orb_frame_view_t& KF,
                           const orb_map_points_t& mp, const uint8_t* usable, float th, int ORBdist,
                           std::vector<int>& newMatches, int device = 0) {
        newMatches.assign(Cur.n, -1);
        int n = 0;
        orb_check(orb_search_by_projection_reloc(&Cur, curTaken, &KF, mp, usable, th, ORBdist, mbCheckOrientation, newMatches.data(), &n, device));
        return n;
    }
    // SearchByProjection(KeyFrame*, Scw, vpPoints, vpMatched, th) (286-407); KF's pose = Scw's.
    int SearchByProjection(const orb_frame_view_t& KFscw, const uint8_t* kfTaken, const orb_map_points_t& pts,
                           const uint8_t* usable, int th, std::vector<int>& newMatches, int device = 0) {
        newMatches.assign(KFscw.n, -1);
        int n = 0;
        orb_check(orb_search_by_projection_sim3(&KFscw, kfTaken, pts, usable, th, newMatches.data(), &n, device));
        return n;
    }
    // SearchBySim3 (ORBmatcher.cc:1267-1505): vpMatches12[i1] = agreeing KF2 index or -1.
    int SearchBySim3(const orb_frame_view_t& KF1, const orb_map_points_t& mp1, const uint8_t* usable1,
                     const orb_frame_view_t& KF2, const orb_map_points_t& mp2, const uint8_t* usable2,
                     const float sR12[9], const float t12[3], const float sR21[9], const float t21[3], float th,
                     std::vector<int>& vpMatches12, int device = 0) {
        vpMatches12.assign(KF1.n, -1);
        int n = 0;
        orb_check(orb_search_by_sim3(&KF1, mp1, usable1, &KF2, mp2, usable2, sR12, t12, sR21, t21, th, vpMatches12.data(), &n, device));
        return n;
    }
    // Fuse(KeyFrame*, vector<MapPoint*>, th) / Fuse(KeyFrame*, Scw, ..., th) (1016-1265):
    // bestIdx[i] = KF keypoint point i fuses with, or -1; the caller applies Replace /
    // AddObservation in point order.
    int Fuse(const orb_frame_view_t& KF, const orb_map_points_t& pts, const uint8_t* usable, float th, bool scw,
             std::vector<int>& bestIdx, int device = 0) {
        bestIdx.assign(pts.n, -1);
        int n = 0;
        orb_check(orb_fuse(&KF, pts, usable, th, scw ? 1 : 0, bestIdx.data(), &n, device));
        return n;
    }

#ifdef ORB_WITH_OPENCV
    static int DescriptorDistance(const cv::Mat& a, const cv::Mat& b) {
        return orb_descriptor_distance(a.ptr<uint8_t>(), b.ptr<uint8_t>());
    }
#endif

private:
    float mfNNratio;
    bool mbCheckOrientation;
};

// A DBoW2::BowVector (std::map<WordId, WordValue>) as the C ABI takes it: words ascending.
struct BowVector {
    std::vector<uint32_t> words;
    std::vector<double> values;
    BowVector() {}
    template <class Map>  // any map<unsigned, double>-like container iterated in key order
    explicit BowVector(const Map& m) {
        words.reserve(m.size());
        values.reserve(m.size());
        for (typename Map::const_iterator it = m.begin(); it != m.end(); ++it) {
            words.push_back((uint32_t)it->first);
            values.push_back((double)it->second);
        }
    }
    int size() const { return (int)words.size(); }
};

// mpVoc->score(v1, v2) (TemplatedVocabulary::score, L1Scoring::score).
inline double score(const orb_vocabulary_t* voc, const BowVector& v1, const BowVector& v2) {
    double s = 0.0;
    orb_check(orb_vocabulary_score(voc, v1.words.data(), v1.values.data(), v1.size(), v2.words.data(),
                                   v2.values.data(), v2.size(), &s));
    return s;
}

// KeyFrameDatabase over keyframe ids (KeyFrame::mnId).  The caller passes what the reference
// reads through the KeyFrame*: mBowVec on add and on a query, GetBestCovisibilityKeyFrames(10)
// whenever the covisibility graph changes, GetConnectedKeyFrames() with a loop query.  Every id
// met gets the next slot of the native database and keeps it until clear(), so maxKeyFrames
// bounds the ids met between two clear() calls.
class KeyFrameDatabase {
public:
    typedef long unsigned int Id;

    KeyFrameDatabase(const orb_vocabulary_t* voc, int maxKeyFrames = 4096, int64_t maxEntries = 0, int device = 0)
        : max_(maxKeyFrames) {
        orb_check(orb_kfdb_create(voc, maxKeyFrames, maxEntries > 0 ? maxEntries : (int64_t)1024 * maxKeyFrames, device,
                                  &h_));
    }
    ~KeyFrameDatabase() { orb_kfdb_destroy(h_); }
    KeyFrameDatabase(const KeyFrameDatabase&) = delete;
    KeyFrameDatabase& operator=(const KeyFrameDatabase&) = delete;

    void add(Id mnId, const BowVector& bow) {
        orb_check(orb_kfdb_add(h_, slot(mnId), bow.words.data(), bow.values.data(), bow.size()));
    }
    void erase(Id mnId) {
        std::map<Id, int>::const_iterator it = slot_.find(mnId);
        if (it != slot_.end()) orb_check(orb_kfdb_erase(h_, it->second));
    }
    void clear() {
        orb_check(orb_kfdb_clear(h_));
        slot_.clear();
        id_.clear();
    }
    int size() const { return orb_kfdb_size(h_); }
    // pKF->GetBestCovisibilityKeyFrames(10) as ids, in its order.
    void SetBestCovisibilityKeyFrames(Id mnId, const std::vector<Id>& neighbours) {
        std::vector<int32_t> nb;
        for (size_t i = 0; i < neighbours.size(); ++i) nb.push_back(slot(neighbours[i]));
        orb_check(orb_kfdb_set_covisible(h_, slot(mnId), nb.data(), (int)nb.size()));
    }
    // DetectLoopCandidates(pKF, minScore): bow = pKF->mBowVec, connected = pKF->GetConnectedKeyFrames().
    std::vector<Id> DetectLoopCandidates(const BowVector& bow, const std::vector<Id>& connected, float minScore) {
        std::vector<int32_t> conn;
        for (size_t i = 0; i < connected.size(); ++i) {
            std::map<Id, int>::const_iterator it = slot_.find(connected[i]);
            if (it != slot_.end()) conn.push_back(it->second);
        }
        std::vector<int32_t> out(id_.size() + 1);
        int n = 0;
        orb_check(orb_kfdb_detect_loop_candidates(h_, bow.words.data(), bow.values.data(), bow.size(), conn.data(),
                                                  (int)conn.size(), minScore, out.data(), (int)out.size(), &n));
        return ids(out, n);
    }
    // DetectRelocalisationCandidates(F): bow = F->mBowVec.
    std::vector<Id> DetectRelocalisationCandidates(const BowVector& bow) {
        std::vector<int32_t> out(id_.size() + 1);
        int n = 0;
        orb_check(orb_kfdb_detect_relocalisation_candidates(h_, bow.words.data(), bow.values.data(), bow.size(),
                                                            out.data(), (int)out.size(), &n));
        return ids(out, n);
    }
    orb_keyframe_db_t* handle() { return h_; }
    // The native slot of an id (for the device entry points), assigned on first use.
    int slot(Id mnId) {
        std::map<Id, int>::const_iterator it = slot_.find(mnId);
        if (it != slot_.end()) return it->second;
        if ((int)id_.size() >= max_) throw std::runtime_error("orb: more keyframe ids than maxKeyFrames");
        const int s = (int)id_.size();
        slot_[mnId] = s;
        id_.push_back(mnId);
        return s;
    }
    Id id(int slot) const { return id_.at((size_t)slot); }

private:
    std::vector<Id> ids(const std::vector<int32_t>& out, int n) const {
        std::vector<Id> r;
        for (int i = 0; i < n; ++i) r.push_back(id_[(size_t)out[i]]);
        return r;
    }
    orb_keyframe_db_t* h_ = nullptr;
    int max_;
    std::map<Id, int> slot_;
    std::vector<Id> id_;
};

// The scoring half of ORB_SLAM::Initializer (Initializer.cc:122-221, 303-466).  The caller runs
// the front of each RANSAC iteration as the reference does (minimal set, ComputeH21 / ComputeF21,
// the T2inv*Hn*T1, H21i.inv() and T2t*Fn*T1 products) for ALL iterations first and hands the
// matrices over, 9 row-major floats per iteration; one call then scores them all and keeps the
// best as the reference's loop does.  Initialize(keys2, vMatches12, rand31) does
// all of it, the front of every iteration included, on the device in one call.
class Initializer {
public:
    // Initializer(ReferenceFrame, sigma, iterations) (Initializer.cc:33-42): keys1 = the
    // reference frame's mvKeysUn.
    Initializer(const std::vector<orb_keypoint_t>& keys1, float sigma = 1.0f, int iterations = 200, int device = 0)
        : mvKeys1(keys1), mSigma(sigma), mMaxIterations(iterations), device_(device) {}

    // The head of Initialize (Initializer.cc:49-65): keys2 = CurrentFrame.mvKeysUn, vMatches12 as
    // SearchForInitialization wrote it.  Returns N = mvMatches12.size().
    int SetMatches(const std::vector<orb_keypoint_t>& keys2, const std::vector<int>& vMatches12) {
        if (vMatches12.size() != mvKeys1.size()) throw std::runtime_error("orb: vMatches12 must have one entry per key of frame 1");
        mvKeys2 = keys2;
        matches12_.assign(vMatches12.begin(), vMatches12.end());
        mvMatches12.clear();
        for (size_t i = 0; i < matches12_.size(); ++i)
            if (matches12_[i] >= 0) mvMatches12.push_back(std::make_pair((int)i, (int)matches12_[i]));
        return (int)mvMatches12.size();
    }

    // FindHomography (Initializer.cc:122-170) over vH21 / vH12 (mMaxIterations x 9 floats each):
    // vbMatchesInliers (N flags), score and H21 (9 floats) of the winning iteration; when no
    // iteration scores above 0 the flags are all false, score is 0 and H21 is left as it was (the
    // reference leaves its cv::Mat empty).  Returns the winning iteration or -1.
    int FindHomography(const std::vector<float>& vH21, const std::vector<float>& vH12,
                       std::vector<bool>& vbMatchesInliers, float& score, std::vector<float>& H21) {
        need(vH21);
        need(vH12);
        return find(vH21.data(), vH12.data(), nullptr, vH21, vbMatchesInliers, score, H21);
    }
    // FindFundamental (Initializer.cc:173-221) over vF21 (mMaxIterations x 9 floats).
    int FindFundamental(const std::vector<float>& vF21, std::vector<bool>& vbMatchesInliers, float& score,
                        std::vector<float>& F21) {
        need(vF21);
        return find(nullptr, nullptr, vF21.data(), vF21, vbMatchesInliers, score, F21);
    }

    // What Initialize (Initializer.cc:44-116) knows when it calls ReconstructH / ReconstructF.
    struct TwoViewModels {
        std::vector<float> H, F;                                 // 9 floats each; empty without a winner, as the reference's cv::Mat
        float SH, SF, RH;                                        // RH = SH / (SH + SF)
        std::vector<bool> vbMatchesInliersH, vbMatchesInliersF;  // N flags each
        bool bUseH;                                              // RH > 0.40: ReconstructH would be tried, else ReconstructF
        int N;                                                   // mvMatches12.size(); below 8 nothing was generated
        std::vector<std::vector<size_t> > mvSets;                // mMaxIterations x 8
    };
    // Initialize (Initializer.cc:44-116) up to the Reconstruct* call, on the device in one call:
    // the matches, the minimal sets, Normalize, ComputeH21 / ComputeF21 and both checks for all
    // mMaxIterations iterations.  rand31: the mMaxIterations x 8 values rand() returned, in the
    // order DUtils::Random::RandomInt would consume them (the package owns no generator).
    // ReconstructH / ReconstructF below take it from there; the eight-argument Initialize does both.
    TwoViewModels Initialize(const std::vector<orb_keypoint_t>& keys2, const std::vector<int>& vMatches12,
                             const std::vector<int>& rand31) {
        if (rand31.size() != (size_t)mMaxIterations * 8) throw std::runtime_error("orb: rand31 must hold mMaxIterations x 8 values");
        TwoViewModels r;
        r.N = SetMatches(keys2, vMatches12);
        std::vector<uint8_t> inH(mvKeys1.size() + 1, 0), inF(mvKeys1.size() + 1, 0);
        std::vector<int32_t> draws(rand31.begin(), rand31.end()), sets((size_t)mMaxIterations * 8);
        int32_t bh = -1, bf = -1, use_h = 0;
        int n = 0;
        float H[9], F[9];
        orb_check(orb_initializer_ransac(mvKeys1.data(), (int)mvKeys1.size(), mvKeys2.data(), (int)mvKeys2.size(),
                                         matches12_.data(), mSigma, mMaxIterations, draws.data(), nullptr, nullptr,
                                         nullptr, sets.data(), nullptr, nullptr, &bh, &r.SH, inH.data(), &bf, &r.SF,
                                         inF.data(), H, F, &r.RH, &use_h, &n, device_));
        if (bh >= 0) r.H.assign(H, H + 9);
        if (bf >= 0) r.F.assign(F, F + 9);
        r.bUseH = use_h != 0;
        r.vbMatchesInliersH.assign((size_t)n, false);
        r.vbMatchesInliersF.assign((size_t)n, false);
        for (int i = 0; i < n; ++i) {
            r.vbMatchesInliersH[(size_t)i] = inH[(size_t)i] != 0;
            r.vbMatchesInliersF[(size_t)i] = inF[(size_t)i] != 0;
        }
        r.mvSets.assign((size_t)mMaxIterations, std::vector<size_t>(8, 0));
        for (size_t k = 0; k < sets.size(); ++k) r.mvSets[k / 8][k % 8] = (size_t)sets[k];
        return r;
    }

    // ReconstructH / ReconstructF (Initializer.cc:468-730) on a given model, after SetMatches or
    // Initialize: vbMatchesInliers (N flags) and H21 / F21 (9 floats) as FindHomography /
    // FindFundamental gave them, K4 = fx, fy, cx, cy of mK.  On true R21 (9 floats), t21 (3), vP3D
    // (3 floats per key of frame 1) and vbTriangulated are the reference's; on false R21 and t21
    // are empty, as the reference's cv::Mat, and the two vectors are left as they were.
    bool ReconstructH(const std::vector<bool>& vbMatchesInliers, const std::vector<float>& H21, const float* K4,
                      std::vector<float>& R21, std::vector<float>& t21, std::vector<float>& vP3D,
                      std::vector<bool>& vbTriangulated, float minParallax = 1.0f, int minTriangulated = 50) {
        return reconstruct(1, vbMatchesInliers, H21, K4, R21, t21, vP3D, vbTriangulated, minParallax, minTriangulated);
    }
    bool ReconstructF(const std::vector<bool>& vbMatchesInliers, const std::vector<float>& F21, const float* K4,
                      std::vector<float>& R21, std::vector<float>& t21, std::vector<float>& vP3D,
                      std::vector<bool>& vbTriangulated, float minParallax = 1.0f, int minTriangulated = 50) {
        return reconstruct(0, vbMatchesInliers, F21, K4, R21, t21, vP3D, vbTriangulated, minParallax, minTriangulated);
    }
    // Initialize (Initializer.cc:44-119) whole: the reference's signature plus the draws and K.
    bool Initialize(const std::vector<orb_keypoint_t>& keys2, const std::vector<int>& vMatches12,
                    const std::vector<int>& rand31, const float* K4, std::vector<float>& R21, std::vector<float>& t21,
                    std::vector<float>& vP3D, std::vector<bool>& vbTriangulated) {
        const TwoViewModels m = Initialize(keys2, vMatches12, rand31);
        R21.clear();
        t21.clear();
        // (a model without a winner is empty in the reference and would throw inside Reconstruct*)
        if (m.bUseH) return !m.H.empty() && ReconstructH(m.vbMatchesInliersH, m.H, K4, R21, t21, vP3D, vbTriangulated, 1.0f, 50);
        return !m.F.empty() && ReconstructF(m.vbMatchesInliersF, m.F, K4, R21, t21, vP3D, vbTriangulated, 1.0f, 50);
    }

    std::vector<std::pair<int, int> > mvMatches12;  // (index in frame 1, index in frame 2), as the reference's
    std::vector<orb_keypoint_t> mvKeys1, mvKeys2;
    float mSigma;
    int mMaxIterations;

private:
    void need(const std::vector<float>& v) const {
        if (v.size() != (size_t)mMaxIterations * 9) throw std::runtime_error("orb: hypothesis array must hold mMaxIterations x 9 floats");
    }
    int find(const float* h21, const float* h12, const float* f21, const std::vector<float>& src,
             std::vector<bool>& vbMatchesInliers, float& score, std::vector<float>& M) {
        std::vector<uint8_t> in(mvKeys1.size() + 1, 0);
        int32_t best = -1;
        int n = 0;
        float s = 0.0f;
        orb_check(orb_initializer_check(mvKeys1.data(), (int)mvKeys1.size(), mvKeys2.data(), (int)mvKeys2.size(),
                                        matches12_.data(), mSigma, mMaxIterations, h21, h12, f21, nullptr, nullptr,
                                        f21 ? nullptr : &best, f21 ? nullptr : &s, f21 ? nullptr : in.data(),
                                        f21 ? &best : nullptr, f21 ? &s : nullptr, f21 ? in.data() : nullptr, &n,
                                        device_));
        score = s;
        vbMatchesInliers.assign((size_t)n, false);
        for (int i = 0; i < n; ++i) vbMatchesInliers[(size_t)i] = in[(size_t)i] != 0;
        if (best >= 0) M.assign(src.begin() + (size_t)best * 9, src.begin() + (size_t)best * 9 + 9);
        return best;
    }
    bool reconstruct(int use_h, const std::vector<bool>& vbMatchesInliers, const std::vector<float>& M21, const float* K4,
                     std::vector<float>& R21, std::vector<float>& t21, std::vector<float>& vP3D,
                     std::vector<bool>& vbTriangulated, float minParallax, int minTriangulated) {
        if (M21.size() != 9) throw std::runtime_error("orb: the model must hold 9 floats");
        if (vbMatchesInliers.size() != mvMatches12.size()) throw std::runtime_error("orb: vbMatchesInliers must have one entry per match");
        const size_t n1 = mvKeys1.size();
        std::vector<uint8_t> in(vbMatchesInliers.size() + 1, 0), tri(n1 + 1, 0);
        for (size_t i = 0; i < vbMatchesInliers.size(); ++i) in[i] = vbMatchesInliers[i] ? 1 : 0;
        std::vector<float> P(3 * n1 + 3, 0.0f);
        float R[9], t[3];
        int32_t ok = 0;
        orb_check(orb_initializer_reconstruct(mvKeys1.data(), (int)n1, mvKeys2.data(), (int)mvKeys2.size(), matches12_.data(),
                                              M21.data(), use_h, in.data(), K4, mSigma, minParallax, minTriangulated, &ok,
                                              R, t, P.data(), tri.data(), nullptr, nullptr, nullptr, nullptr, nullptr,
                                              nullptr, nullptr, nullptr, device_));
        R21.clear();
        t21.clear();
        if (!ok) return false;
        R21.assign(R, R + 9);
        t21.assign(t, t + 3);
        vP3D.assign(P.begin(), P.begin() + 3 * n1);
        vbTriangulated.assign(n1, false);
        for (size_t i = 0; i < n1; ++i) vbTriangulated[i] = tri[i] != 0;
        return true;
    }
    std::vector<int32_t> matches12_;
    int device_;
};

// ORB_SLAM::PnPsolver (PnPsolver.cc:39-311 and EPnP under it).  iterate(nIterations, bNoMore,
// vbInliers, nInliers, rand31, Tcw) / find run whole iterations on the device, minimal sets, EPnP's
// compute_pose and Refine included, from the values of rand() that the caller hands over (four per
// iteration; the class owns no random generator).  The older iterate(vR, vt) scores poses the caller
// made: one call scores them all and applies lines 181-196.
class PnPsolver {
public:
    // PnPsolver(F, vpMapPointMatches) (PnPsolver.cc:39-82) over PODs: keysUn = F.mvKeysUn,
    // levelSigma2 = F.mvLevelSigma2; for every keypoint i, usable[i] = vpMapPointMatches[i] is set
    // and not bad, worldPos[3 i ..] = its GetWorldPos().
    PnPsolver(const std::vector<orb_keypoint_t>& keysUn, const std::vector<float>& levelSigma2,
              const std::vector<uint8_t>& usable, const std::vector<float>& worldPos, float fx, float fy, float cx,
              float cy, int device = 0)
        : fu(fx), fv(fy), uc(cx), vc(cy), mnIterations(0), mnBestInliers(0), mnBest(-1), N(0), nKeys_(keysUn.size()),
          device_(device) {
        if (usable.size() != keysUn.size() || worldPos.size() != keysUn.size() * 3)
            throw std::runtime_error("orb: usable / worldPos must have one entry per keypoint");
        for (size_t i = 0; i < keysUn.size(); ++i) {
            if (!usable[i]) continue;
            mvP2D.push_back(keysUn[i].x);
            mvP2D.push_back(keysUn[i].y);
            mvSigma2.push_back(levelSigma2.at((size_t)keysUn[i].octave));
            mvP3Dw.insert(mvP3Dw.end(), worldPos.begin() + 3 * i, worldPos.begin() + 3 * i + 3);
            mvKeyPointIndices.push_back(i);
        }
        SetRansacParameters();
    }

    // PnPsolver.cc:93-129 (mvMaxError = mvSigma2 * th2 is formed on the device)
    void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 4,
                             float epsilon = 0.4f, float th2 = 5.991f) {
        N = (int)mvSigma2.size();
        int nMinInliers = (int)(N * epsilon);
        if (nMinInliers < minInliers) nMinInliers = minInliers;
        if (nMinInliers < minSet) nMinInliers = minSet;
        mRansacMinInliers = nMinInliers;
        mRansacEpsilon = epsilon;
        if (mRansacEpsilon < (float)mRansacMinInliers / N) mRansacEpsilon = (float)mRansacMinInliers / N;
        mRansacMaxIts = ransac_iterations(probability, mRansacEpsilon, mRansacMinInliers == N, maxIterations);
        mRansacTh = th2;
    }

    // vR (k x 9) / vt (k x 3): mRi / mti of the next k iterations.  Returns the first of them whose
    // count reaches mRansacMinInliers (where the reference calls Refine; the later ones are not
    // taken as run), or -1 when none does.  mnIterations, mnBestInliers and mvbBestInliers advance
    // as iterate() advances them; mnBest is the index, within the call that set it, of the pose
    // holding mvbBestInliers.
    int iterate(const std::vector<double>& vR, const std::vector<double>& vt) {
        const int k = (int)(vt.size() / 3);
        if (k < 1 || vR.size() != (size_t)k * 9 || vt.size() != (size_t)k * 3)
            throw std::runtime_error("orb: poses must be k x 9 and k x 3 doubles");
        const int W = (N + 63) / 64;
        std::vector<int32_t> counts((size_t)k), best_at((size_t)k);
        std::vector<uint64_t> masks((size_t)k * W + 1);
        int32_t first = -1;
        orb_check(orb_pnp_check_inliers(N, mvP3Dw.data(), mvP2D.data(), mvSigma2.data(), mRansacTh, fu, fv, uc, vc, k,
                                        vR.data(), vt.data(), mRansacMinInliers, mnBestInliers, counts.data(),
                                        masks.data(), best_at.data(), &first, device_));
        const int last = first >= 0 ? first : k - 1;
        mnIterations += last + 1;
        const int holder = best_at[(size_t)last];
        if (holder >= 0) {
            mnBest = holder;
            mnBestInliers = counts[(size_t)holder];
            unpack(&masks[(size_t)holder * W], mvbBestInliers);
        }
        return first;
    }

    // iterate(nIterations, bNoMore, vbInliers, nInliers) (PnPsolver.cc:137-230).  rand31: the values
    // rand() would return, 0 <= r < 2^31, four per iteration.  The reference's loop goes on while
    // mnIterations < mRansacMaxIts || nCurrentIterations < nIterations, an OR: up to
    // max(mRansacMaxIts - mnIterations, nIterations) iterations are run and rand31 must hold that many
    // sets of four.  Returns true with the pose in Tcw (12 floats: Rcw row-major, then tcw) where the
    // reference returns mRefinedTcw or mBestTcw, false where it returns an empty Mat.  vbInliers: per
    // frame keypoint.  randUsed (may be NULL): the number of values consumed, 4 per iteration taken
    // as run.  mRansacMinInliers >= 4 (SetRansacParameters sees to it).
    bool iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers,
                 const std::vector<int32_t>& rand31, float* Tcw, size_t* randUsed = nullptr) {
        bNoMore = false;
        vbInliers.clear();
        nInliers = 0;
        if (randUsed) *randUsed = 0;
        if (N < mRansacMinInliers) {
            bNoMore = true;
            return false;
        }
        const int k = std::max(mRansacMaxIts - mnIterations, nIterations);
        if (k > 0) {
            if (rand31.size() < (size_t)k * 4) throw std::runtime_error("orb: rand31 must hold 4 values per iteration");
            const int W = (N + 63) / 64;
            std::vector<int32_t> counts((size_t)k), best_at((size_t)k);
            std::vector<uint64_t> masks((size_t)k * W + 1), pose_mask((size_t)W + 1);
            std::vector<double> vR((size_t)k * 9), vt((size_t)k * 3);
            int32_t first_refined = -1, pose_inliers = 0;
            float pose[12];
            orb_check(orb_pnp_ransac(N, mvP3Dw.data(), mvP2D.data(), mvSigma2.data(), mRansacTh, fu, fv, uc, vc, k,
                                     nullptr, rand31.data(), mRansacMinInliers, mnBestInliers, counts.data(),
                                     masks.data(), best_at.data(), nullptr, vR.data(), vt.data(), nullptr, nullptr,
                                     &first_refined, pose, pose_mask.data(), &pose_inliers, device_));
            const int last = first_refined >= 0 ? first_refined : k - 1;
            mnIterations += last + 1;
            if (randUsed) *randUsed = (size_t)(last + 1) * 4;
            const int holder = best_at[(size_t)last];
            if (holder >= 0) {
                mnBest = holder;
                mnBestInliers = counts[(size_t)holder];
                unpack(&masks[(size_t)holder * W], mvbBestInliers);
                for (int j = 0; j < 9; ++j) mBestTcw[j] = (float)vR[(size_t)holder * 9 + j];
                for (int j = 0; j < 3; ++j) mBestTcw[9 + j] = (float)vt[(size_t)holder * 3 + j];
            }
            if (first_refined >= 0) {
                nInliers = pose_inliers;
                std::vector<bool> refined;
                unpack(pose_mask.data(), refined);
                vbInliers = InliersByKeyPoint(refined);
                std::copy(pose, pose + 12, Tcw);
                return true;
            }
        }
        if (mnIterations >= mRansacMaxIts) {
            bNoMore = true;
            if (mnBestInliers >= mRansacMinInliers) {
                nInliers = mnBestInliers;
                vbInliers = InliersByKeyPoint(mvbBestInliers);
                std::copy(mBestTcw, mBestTcw + 12, Tcw);
                return true;
            }
        }
        return false;
    }

    // find (PnPsolver.cc:131-135): iterate(mRansacMaxIts, ...)
    bool find(std::vector<bool>& vbInliers, int& nInliers, const std::vector<int32_t>& rand31, float* Tcw,
              size_t* randUsed = nullptr) {
        bool bFlag;
        return iterate(mRansacMaxIts, bFlag, vbInliers, nInliers, rand31, Tcw, randUsed);
    }

    // CheckInliers for one pose (Refine's scoring, PnPsolver.cc:255-262): the count and the flags.
    int CheckInliers(const double* R, const double* t, std::vector<bool>& vbInliers) const {
        std::vector<uint64_t> mask((size_t)(N + 63) / 64 + 1);
        int32_t count = 0;
        orb_check(orb_pnp_check_inliers(N, mvP3Dw.data(), mvP2D.data(), mvSigma2.data(), mRansacTh, fu, fv, uc, vc, 1,
                                        R, t, mRansacMinInliers, 0, &count, mask.data(), nullptr, nullptr, device_));
        unpack(mask.data(), vbInliers);
        return count;
    }

    // vbInliers of iterate / find (PnPsolver.cc:201-206, 219-224): per frame keypoint.
    std::vector<bool> InliersByKeyPoint(const std::vector<bool>& vbInliers) const {
        std::vector<bool> v(nKeys_, false);
        for (int i = 0; i < N && i < (int)vbInliers.size(); ++i)
            if (vbInliers[(size_t)i]) v[mvKeyPointIndices[(size_t)i]] = true;
        return v;
    }

    static int ransac_iterations(double probability, float epsilon, bool all, int maxIterations) {
        int nIterations;
        if (all)
            nIterations = 1;
        else {
            const double v = std::ceil(std::log(1 - probability) / std::log(1 - std::pow((double)epsilon, 3)));
            nIterations = v >= -2147483648.0 && v < 2147483648.0 ? (int)v : INT_MIN;  // as x86-64 converts
        }
        return std::max(1, std::min(nIterations, maxIterations));
    }

    std::vector<float> mvP2D, mvSigma2, mvP3Dw;  // N x 2, N, N x 3
    std::vector<size_t> mvKeyPointIndices;
    std::vector<bool> mvbBestInliers;
    double fu, fv, uc, vc;
    int mnIterations, mnBestInliers, mnBest;
    int mRansacMinInliers, mRansacMaxIts;
    float mRansacEpsilon, mRansacTh;
    float mBestTcw[12] = {0};  // Rcw row-major, tcw
    int N;

private:
    void unpack(const uint64_t* w, std::vector<bool>& v) const {
        v.assign((size_t)N, false);
        for (int i = 0; i < N; ++i) v[(size_t)i] = (w[i >> 6] >> (i & 63)) & 1;
    }
    size_t nKeys_;
    int device_;
};

// ORB_SLAM::Sim3Solver (Sim3Solver.cc:37-213, 335-418).  iterate(nIterations, bNoMore, vbInliers,
// nInliers, rand31) / find run whole iterations on the device, minimal sets and computeT included,
// from the values of rand() that the caller hands over (three per iteration; the class owns no
// random generator).  The older iterate(vT12, vT21, ...) scores hypotheses the caller made.
class Sim3Solver {
public:
    // Sim3Solver(pKF1, pKF2, vpMatched12) (Sim3Solver.cc:37-112) over PODs, one entry per kept
    // correspondence: x3Dc1 / x3Dc2 (N x 3, mvX3Dc1 / mvX3Dc2), sigma2_1 / sigma2_2 (GetSigma2 of the
    // keypoints' octaves), indices1 (mvnIndices1); N1 = vpMatched12.size(); K1 / K2: fx, fy, cx, cy.
    Sim3Solver(const std::vector<float>& x3Dc1, const std::vector<float>& x3Dc2, const std::vector<float>& sigma2_1,
               const std::vector<float>& sigma2_2, const std::vector<size_t>& indices1, int N1, const float* K1,
               const float* K2, int device = 0)
        : mvX3Dc1(x3Dc1), mvX3Dc2(x3Dc2), mvSigma2_1(sigma2_1), mvSigma2_2(sigma2_2), mvnIndices1(indices1),
          mnIterations(0), mnBestInliers(0), mnBest(-1), mN1(N1), device_(device) {
        N = (int)sigma2_1.size();
        if (x3Dc1.size() != (size_t)N * 3 || x3Dc2.size() != (size_t)N * 3 || sigma2_2.size() != (size_t)N ||
            indices1.size() != (size_t)N)
            throw std::runtime_error("orb: the correspondence arrays must have one entry per correspondence");
        for (int k = 0; k < 4; ++k) mK1[k] = K1[k], mK2[k] = K2[k];
        SetRansacParameters();
    }

    // Sim3Solver.cc:114-138
    void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300) {
        mRansacMinInliers = minInliers;
        const float epsilon = (float)mRansacMinInliers / N;
        mRansacMaxIts = PnPsolver::ransac_iterations(probability, epsilon, mRansacMinInliers == N, maxIterations);
        mnIterations = 0;
    }

    // vT12 / vT21 (k x 12 floats): the next k iterations.  Returns the first of them the reference
    // returns at (count >= the running best and > mRansacMinInliers; the later ones are not taken
    // as run), or -1.  vbInliers (mN1 flags by keyframe-1 keypoint) and nInliers are set as
    // iterate() sets them: filled on acceptance, all false / 0 otherwise.
    int iterate(const std::vector<float>& vT12, const std::vector<float>& vT21, std::vector<bool>& vbInliers,
                int& nInliers) {
        const int k = (int)(vT12.size() / 12);
        if (k < 1 || vT12.size() != (size_t)k * 12 || vT21.size() != (size_t)k * 12)
            throw std::runtime_error("orb: transforms must be k x 12 floats each");
        const int W = (N + 63) / 64;
        std::vector<int32_t> counts((size_t)k), best_at((size_t)k);
        std::vector<uint64_t> masks((size_t)k * W + 1);
        int32_t first = -1;
        orb_check(orb_sim3_check_inliers(N, mvX3Dc1.data(), mvX3Dc2.data(), mvSigma2_1.data(), mvSigma2_2.data(), mK1,
                                         mK2, k, vT12.data(), vT21.data(), mRansacMinInliers, mnBestInliers,
                                         counts.data(), masks.data(), best_at.data(), &first, device_));
        const int last = first >= 0 ? first : k - 1;
        mnIterations += last + 1;
        const int holder = best_at[(size_t)last];
        if (holder >= 0) {
            mnBest = holder;
            mnBestInliers = counts[(size_t)holder];
            mvbBestInliers.assign((size_t)N, false);
            for (int i = 0; i < N; ++i) mvbBestInliers[(size_t)i] = (masks[(size_t)holder * W + (i >> 6)] >> (i & 63)) & 1;
        }
        vbInliers.assign((size_t)mN1, false);
        nInliers = 0;
        if (first >= 0) {
            nInliers = counts[(size_t)first];
            for (int i = 0; i < N; ++i)
                if (mvbBestInliers[(size_t)i]) vbInliers[mvnIndices1[(size_t)i]] = true;
        }
        return first;
    }

    // iterate(nIterations, bNoMore, vbInliers, nInliers) (Sim3Solver.cc:140-207).  rand31: the values
    // rand() would return, 0 <= r < 2^31, three per iteration; min(nIterations, mRansacMaxIts -
    // mnIterations) iterations are run and rand31 must hold that many triples.  Returns true with
    // the accepted transform in mBest* (GetEstimated*) where the reference returns mBestT12, false
    // where it returns an empty Mat.  randUsed (may be NULL): the number of values consumed, 3 per
    // iteration taken as run.  mRansacMinInliers >= 3.
    bool iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers,
                 const std::vector<int32_t>& rand31, size_t* randUsed = nullptr) {
        bNoMore = false;
        vbInliers.assign((size_t)mN1, false);
        nInliers = 0;
        if (randUsed) *randUsed = 0;
        if (N < mRansacMinInliers) {
            bNoMore = true;
            return false;
        }
        const int k = std::min(nIterations, mRansacMaxIts - mnIterations);
        if (k > 0) {
            if (rand31.size() < (size_t)k * 3) throw std::runtime_error("orb: rand31 must hold 3 values per iteration");
            const int W = (N + 63) / 64;
            std::vector<int32_t> counts((size_t)k), best_at((size_t)k);
            std::vector<uint64_t> masks((size_t)k * W + 1);
            std::vector<float> sim3((size_t)k * 13);
            int32_t first = -1;
            orb_check(orb_sim3_ransac(N, mvX3Dc1.data(), mvX3Dc2.data(), mvSigma2_1.data(), mvSigma2_2.data(), mK1, mK2, k,
                                      nullptr, rand31.data(), mRansacMinInliers, mnBestInliers, counts.data(),
                                      masks.data(), best_at.data(), &first, nullptr, nullptr, sim3.data(), nullptr,
                                      nullptr, device_));
            const int last = first >= 0 ? first : k - 1;
            mnIterations += last + 1;
            if (randUsed) *randUsed = (size_t)(last + 1) * 3;
            const int holder = best_at[(size_t)last];
            if (holder >= 0) {
                mnBest = holder;
                mnBestInliers = counts[(size_t)holder];
                mvbBestInliers.assign((size_t)N, false);
                for (int i = 0; i < N; ++i)
                    mvbBestInliers[(size_t)i] = (masks[(size_t)holder * W + (i >> 6)] >> (i & 63)) & 1;
                std::copy(sim3.begin() + (size_t)holder * 13, sim3.begin() + (size_t)holder * 13 + 9, mBestRotation);
                std::copy(sim3.begin() + (size_t)holder * 13 + 9, sim3.begin() + (size_t)holder * 13 + 12, mBestTranslation);
                mBestScale = sim3[(size_t)holder * 13 + 12];
            }
            if (first >= 0) {
                nInliers = counts[(size_t)first];
                for (int i = 0; i < N; ++i)
                    if (mvbBestInliers[(size_t)i]) vbInliers[mvnIndices1[(size_t)i]] = true;
                return true;
            }
        }
        if (mnIterations >= mRansacMaxIts) bNoMore = true;
        return false;
    }

    // find (Sim3Solver.cc:209-213): iterate(mRansacMaxIts, ...)
    bool find(std::vector<bool>& vbInliers12, int& nInliers, const std::vector<int32_t>& rand31,
              size_t* randUsed = nullptr) {
        bool bFlag;
        return iterate(mRansacMaxIts, bFlag, vbInliers12, nInliers, rand31, randUsed);
    }

    // mBestRotation (row-major 3 x 3), mBestTranslation, mBestScale of the iterations so far
    const float* GetEstimatedRotation() const { return mBestRotation; }
    const float* GetEstimatedTranslation() const { return mBestTranslation; }
    float GetEstimatedScale() const { return mBestScale; }

    std::vector<float> mvX3Dc1, mvX3Dc2, mvSigma2_1, mvSigma2_2;
    std::vector<size_t> mvnIndices1;
    std::vector<bool> mvbBestInliers;
    float mK1[4], mK2[4];
    float mBestRotation[9] = {0}, mBestTranslation[3] = {0}, mBestScale = 0;
    int mnIterations, mnBestInliers, mnBest;
    int mRansacMinInliers, mRansacMaxIts;
    int N, mN1;

private:
    int device_;
};

// ORB_SLAM::Optimizer::PoseOptimization(Frame*) (Optimizer.cc:154-285) and Optimizer::OptimizeSim3
// (Optimizer.cc:1721-1917), Optimizer::LocalBundleAdjustment (Optimizer.cc:287-536) and
// Optimizer::OptimizeEssentialGraph (Optimizer.cc:1470-1719) over PODs; global bundle adjustment stays with
// the reference's g2o.

// g2o::Sim3(Converter::toMatrix3d(R), Converter::toVector3d(t), 1.0) of a keyframe's Tcw (Rcw row-major,
// tcw) as eight doubles (q x y z w, t, s): host arithmetic with the bits of the device's conversion.
inline std::array<double, 8> Sim3FromPose(const float Tcw[12]) {
    std::array<double, 8> S;
    orb_sim3_from_pose(Tcw, S.data());
    return S;
}
// [R | t (1 / s)] narrowed, what KeyFrame::SetPose receives (Optimizer.cc:1676-1684, LoopClosing.cc:498-506)
inline std::array<float, 12> PoseFromSim3(const double S[8]) {
    std::array<float, 12> T;
    orb_sim3_to_pose(S, T.data(), nullptr);
    return T;
}

class Optimizer {
public:
    // F.keysUn = pFrame->mvKeysUn (N of them), invLevelSigma2 = mvInvLevelSigma2, fx..cy the
    // frame's calibration; for every keypoint i, hasMP[i] = mvpMapPoints[i] is set and
    // worldPos[3 i ..] = its GetWorldPos().  Tcw: Rcw row-major then tcw (12 floats), read as
    // pFrame->mTcw and overwritten with the optimised pose.  mvbOutlier is resized to N and
    // written as the reference writes it (false where there is no MapPoint).  Returns
    // nInitialCorrespondences - nBad.
    static int PoseOptimization(const FrameView& F, const std::vector<float>& invLevelSigma2, float fx, float fy,
                                float cx, float cy, const std::vector<uint8_t>& hasMP,
                                const std::vector<float>& worldPos, float* Tcw, std::vector<bool>& mvbOutlier,
                                int device = 0, orb_pose_opt_info_t* info = nullptr) {
        const size_t N = (size_t)std::max(F.N, 0);
        if (hasMP.size() != N || worldPos.size() != N * 3)
            throw std::runtime_error("orb: hasMP / worldPos must have one entry per keypoint");
        std::vector<float> obs(N * 2), inv(N);
        for (size_t i = 0; i < N; ++i) {
            obs[2 * i] = F.keysUn[i].x, obs[2 * i + 1] = F.keysUn[i].y;
            inv[i] = hasMP[i] ? invLevelSigma2.at((size_t)F.keysUn[i].octave) : 0.0f;
        }
        std::vector<uint8_t> flags(std::max<size_t>(N, 1));
        float out[12];
        int32_t nInliers = 0;
        orb_check(orb_pose_optimization((int)N, worldPos.data(), obs.data(), inv.data(), hasMP.data(), fx, fy, cx, cy,
                                        Tcw, out, nullptr, flags.data(), &nInliers, info, device));
        std::copy(out, out + 12, Tcw);
        mvbOutlier.assign(N, false);
        for (size_t i = 0; i < N; ++i) mvbOutlier[i] = flags[i] != 0;
        return nInliers;
    }

    // ORB_SLAM::Optimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2) (Optimizer.cc:1721-1917)
    // over PODs.  KF1.keysUn / KF2.keysUn: the two keyframes' undistorted keypoints;
    // invLevelSigma2_1 = pKF1's mvInvLevelSigma2, levelSigma2_2 = pKF2's mvLevelSigma2 (the reference
    // weights e21 with GetSigma2).  Slot i of vpMatches1 (one per keypoint of KF1) holds i2 =
    // vpMatches1[i]->GetIndexInKeyFrame(pKF2), or -1 where there is no usable pair (no match, a
    // MapPoint missing or bad, i2 < 0); p3d1c[3 i ..] = R1w * P3D1w + t1w and p3d2c[3 i ..] = R2w *
    // P3D2w + t2w of the pair, as the caller's cv::Mat arithmetic gives them.  S12: 13 floats (R
    // row-major, t, s), read as g2oS12 and overwritten with the optimised Sim3; when the routine
    // returns 0 because fewer than 10 pairs are left it keeps the input, as the reference's does.
    // Slots the routine clears are set to -1.  Returns nIn.
    static int OptimizeSim3(const FrameView& KF1, const FrameView& KF2, const std::vector<float>& invLevelSigma2_1,
                            const std::vector<float>& levelSigma2_2, const float* K1, const float* K2,
                            std::vector<int>& vpMatches1, const std::vector<float>& p3d1c,
                            const std::vector<float>& p3d2c, float* S12, float th2, int device = 0,
                            orb_sim3_opt_info_t* info = nullptr) {
        const size_t N = vpMatches1.size();
        if (N > (size_t)std::max(KF1.N, 0) || p3d1c.size() != N * 3 || p3d2c.size() != N * 3)
            throw std::runtime_error("orb: vpMatches1 / p3d1c / p3d2c must have one entry per keypoint of KF1");
        std::vector<float> obs1(N * 2), obs2(N * 2), w1(N), w2(N);
        std::vector<uint8_t> usable(std::max<size_t>(N, 1)), kept(std::max<size_t>(N, 1));
        for (size_t i = 0; i < N; ++i) {
            const int i2 = vpMatches1[i];
            usable[i] = i2 >= 0 && i2 < KF2.N;
            if (!usable[i]) continue;
            obs1[2 * i] = KF1.keysUn[i].x, obs1[2 * i + 1] = KF1.keysUn[i].y;
            obs2[2 * i] = KF2.keysUn[i2].x, obs2[2 * i + 1] = KF2.keysUn[i2].y;
            w1[i] = invLevelSigma2_1.at((size_t)KF1.keysUn[i].octave);
            w2[i] = levelSigma2_2.at((size_t)KF2.keysUn[i2].octave);
        }
        float out[13];
        int32_t nIn = 0;
        orb_sim3_opt_info_t inf;
        orb_check(orb_optimize_sim3((int)N, p3d1c.data(), p3d2c.data(), obs1.data(), obs2.data(), w1.data(), w2.data(),
                                    usable.data(), K1, K2, th2, S12, kept.data(), nullptr, out, &nIn, &inf, device));
        if (info) *info = inf;
        for (size_t i = 0; i < N; ++i)
            if (usable[i] && !kept[i]) vpMatches1[i] = -1;
        // the reference copies the estimate out only past its early return (Optimizer.cc:1887-1888, 1914)
        if (inf.more_iterations != 0) std::copy(out, out + 13, S12);
        return nIn;
    }

    // The graph of ORB_SLAM::Optimizer::LocalBundleAdjustment (Optimizer.cc:356-447) as the caller's
    // flattening loop fills it, and what lines 453-535 read back.
    struct LocalBAGraph {
        std::vector<float> kfPose;        // 12 per keyframe (Rcw row-major, tcw): lLocalKeyFrames, then lFixedCameras
        std::vector<float> kfK;           // fx fy cx cy per keyframe
        std::vector<uint8_t> kfFixed;     // mnId == 0, or a fixed camera
        std::vector<float> ptPos;         // GetWorldPos() of lLocalMapPoints, in list order
        std::vector<int32_t> ptNObs;      // GetObservations().size(), bad keyframes included
        std::vector<int32_t> edgePt, edgeKf;  // one edge per observation in a keyframe that is not bad
        std::vector<float> edgeObs;       // kpUn.pt
        std::vector<float> edgeInvSigma2; // GetInvSigma2(kpUn.octave)
    };
    struct LocalBAResult {
        std::vector<float> kfPose, ptPos;      // what SetPose / SetWorldPos receive (lines 520-535)
        std::vector<uint8_t> edgeErased;       // 0, or the round after which the edge was erased: walk in edge order
        std::vector<uint8_t> ptBad;
        orb_local_ba_info_t info;
    };
    // pbStopFlag is not served: the call runs both rounds.
    static void LocalBundleAdjustment(const LocalBAGraph& G, LocalBAResult& R, int device = 0) {
        const size_t nk = G.kfFixed.size(), np = G.ptNObs.size(), ne = G.edgePt.size();
        if (G.kfPose.size() != nk * 12 || G.kfK.size() != nk * 4 || G.ptPos.size() != np * 3 || G.edgeKf.size() != ne ||
            G.edgeObs.size() != ne * 2 || G.edgeInvSigma2.size() != ne)
            throw std::invalid_argument("LocalBundleAdjustment: array sizes disagree");
        R.kfPose.assign(nk * 12, 0.0f), R.ptPos.assign(np * 3, 0.0f);
        R.edgeErased.assign(ne, 0), R.ptBad.assign(np, 0);
        orb_check(orb_local_bundle_adjustment((int)nk, G.kfPose.data(), G.kfK.data(), G.kfFixed.data(), (int)np,
                                              G.ptPos.data(), G.ptNObs.data(), (int)ne, G.edgePt.data(), G.edgeKf.data(),
                                              G.edgeObs.data(), G.edgeInvSigma2.data(), R.kfPose.data(), nullptr,
                                              R.ptPos.data(), nullptr, R.edgeErased.data(), R.ptBad.data(), &R.info,
                                              device));
    }

    // The graph of ORB_SLAM::Optimizer::OptimizeEssentialGraph (Optimizer.cc:1498-1659) as the caller's
    // flattening loop fills it, and what lines 1666-1718 read back.
    struct EssentialGraph {
        std::vector<float> kfPose;            // 12 per keyframe of vpKFs that is not bad (Rcw row-major, tcw)
        std::vector<uint8_t> kfFixed;         // pKF == pLoopKF
        std::vector<double> kfCorrected;      // 8 per keyframe (q x y z w, t, s): CorrectedSim3[pKF] where ...
        std::vector<uint8_t> kfHasCorrected;  // ... CorrectedSim3.count(pKF); both empty: no entry at all
        std::vector<double> kfNonCorrected;   // NonCorrectedSim3 likewise
        std::vector<uint8_t> kfHasNonCorrected;
        std::vector<int32_t> edgeI, edgeJ;    // vertex 0 and vertex 1, indices into the keyframe arrays
        std::vector<uint8_t> edgeKind;        // 0: lines 1539-1567, 1: lines 1570-1659
        std::vector<float> ptPos;             // GetWorldPos() of vpMPs
        std::vector<int32_t> ptRef;           // the index of nIDr's keyframe, -1 where it has no vertex
        std::vector<uint8_t> ptSkip;          // pMP->isBad(); empty: none
    };
    struct EssentialGraphResult {
        std::vector<double> kfSim3;           // the optimised estimates
        std::vector<float> kfPose, ptPos;     // what SetPose / SetWorldPos receive (a skipped point: its input)
        orb_essential_graph_info_t info;
    };
    static void OptimizeEssentialGraph(const EssentialGraph& G, EssentialGraphResult& R, int nIterations = 20,
                                       int device = 0) {
        const size_t nk = G.kfFixed.size(), ne = G.edgeI.size(), np = G.ptRef.size();
        auto table_ok = [nk](const std::vector<double>& t, const std::vector<uint8_t>& f) {
            return (t.empty() && f.empty()) || (t.size() == nk * 8 && f.size() == nk);
        };
        if (G.kfPose.size() != nk * 12 || G.edgeJ.size() != ne || G.edgeKind.size() != ne || G.ptPos.size() != np * 3 ||
            !table_ok(G.kfCorrected, G.kfHasCorrected) || !table_ok(G.kfNonCorrected, G.kfHasNonCorrected) ||
            (!G.ptSkip.empty() && G.ptSkip.size() != np))
            throw std::invalid_argument("OptimizeEssentialGraph: array sizes disagree");
        R.kfSim3.assign(nk * 8, 0.0), R.kfPose.assign(nk * 12, 0.0f), R.ptPos = G.ptPos;
        orb_check(orb_optimize_essential_graph(
            (int)nk, G.kfPose.data(), G.kfHasCorrected.empty() ? nullptr : G.kfCorrected.data(),
            G.kfHasCorrected.empty() ? nullptr : G.kfHasCorrected.data(),
            G.kfHasNonCorrected.empty() ? nullptr : G.kfNonCorrected.data(),
            G.kfHasNonCorrected.empty() ? nullptr : G.kfHasNonCorrected.data(), G.kfFixed.data(), (int)ne, G.edgeI.data(),
            G.edgeJ.data(), G.edgeKind.data(), (int)np, G.ptPos.data(), G.ptRef.data(),
            G.ptSkip.empty() ? nullptr : G.ptSkip.data(), nIterations, R.kfSim3.data(), R.kfPose.data(), nullptr,
            R.ptPos.data(), nullptr, &R.info, device));
    }
};

// LocalMapping::CreateNewMapPoints' arithmetic over POD views (LocalMapping.cc:227-393, 474-491) and
// MapPoint::UpdateNormalAndDepth (MapPoint.cc:273-312).  The thread, the map mutation and the culling
// stay with the caller (local BA is gpu::Optimizer::LocalBundleAdjustment): outputs are indices and points,
// where the reference calls `new MapPoint(x3D, ...)`, AddObservation and AddMapPoint.
class LocalMapping {
public:
    // ComputeF12(pKF1, pKF2): row-major 3 x 3, the matrix ORBmatcher::SearchForTriangulation takes.
    static void ComputeF12(const orb_frame_view_t& KF1, const orb_frame_view_t& KF2, float F12[9]) {
        orb_check(orb_compute_f12(&KF1, &KF2, F12));
    }

    // The neighbour-loop body for one pair past the matcher (lines 276-391): vMatches12[i1] = idx2 or -1.
    // vMatchedIndices: the accepted (idx1, idx2), in the order the reference creates its MapPoints;
    // vX3D: their points, 3 floats each.  mpPos2 / hasMp2 (KF2's MapPoints, or NULL) feed the baseline gate
    // of lines 258-265.  Returns false when that gate skips the pair.
    static bool CreateNewMapPoints(const orb_frame_view_t& KF1, const orb_frame_view_t& KF2,
                                   const std::vector<int>& vMatches12, const float* mpPos2, const uint8_t* hasMp2,
                                   std::vector<std::pair<int, int> >& vMatchedIndices, std::vector<float>& vX3D,
                                   std::vector<uint8_t>* vStatus = nullptr, int device = 0) {
        const size_t n1 = (size_t)KF1.n;
        if (vMatches12.size() != n1) throw std::invalid_argument("vMatches12 must have one entry per KF1 keypoint");
        std::vector<int32_t> m(vMatches12.begin(), vMatches12.end()), i1(n1), i2(n1);
        std::vector<float> x(3 * n1);
        std::vector<uint8_t> st(n1);
        int32_t nNew = 0, skipped = 0;
        orb_check(orb_create_new_map_points(&KF1, &KF2, m.data(), mpPos2, hasMp2, x.data(), st.data(), nullptr, &nNew,
                                            i1.data(), i2.data(), &skipped, nullptr, device));
        vMatchedIndices.clear();
        vX3D.clear();
        for (int k = 0; k < nNew; ++k) {
            vMatchedIndices.push_back(std::make_pair((int)i1[k], (int)i2[k]));
            vX3D.insert(vX3D.end(), x.begin() + 3 * i1[k], x.begin() + 3 * i1[k] + 3);
        }
        if (vStatus) *vStatus = st;
        return skipped == 0;
    }

    // MapPoint::UpdateNormalAndDepth for M points with their observations as CSR (orb_abi.h states the
    // order): normal M x 3, dmin / dmax M.
    static void UpdateNormalAndDepth(const std::vector<int32_t>& offsets, const std::vector<float>& obsOw,
                                     const std::vector<float>& pos, const std::vector<float>& refOw,
                                     const std::vector<int32_t>& refLevel, const std::vector<float>& scaleFactors,
                                     std::vector<float>& normal, std::vector<float>& dmin, std::vector<float>& dmax,
                                     int device = 0) {
        const size_t M = refLevel.size();
        if (offsets.size() != M + 1 || pos.size() != 3 * M || refOw.size() != 3 * M ||
            (M && obsOw.size() != 3 * (size_t)offsets[M]))
            throw std::invalid_argument("UpdateNormalAndDepth: array sizes disagree");
        normal.assign(3 * M, 0.0f);
        dmin.assign(M, 0.0f);
        dmax.assign(M, 0.0f);
        orb_check(orb_update_normal_and_depth((int)M, offsets.data(), obsOw.data(), pos.data(), refOw.data(),
                                              refLevel.data(), scaleFactors.data(), (int)scaleFactors.size(),
                                              normal.data(), dmin.data(), dmax.data(), device));
    }
};

// The counting of Tracking::UpdateReference (Tracking.cc:768-879, with lines 718-734) and
// KeyFrame::UpdateConnections (KeyFrame.cc:332-411) over the map as flat tables (orb_abi.h states them;
// INTEGRATION.md shows the flattening).  std::map's pointer order is ascending keyframe index.  The map
// and its mutation stay with the caller.
class LocalMap {
public:
    struct Tables {
        std::vector<uint8_t> kfBad;                  // isBad() per keyframe
        std::vector<int32_t> kfMpOff, kfMp;          // GetMapPointMatches() per keypoint: a point index or -1
        std::vector<int32_t> kfCov;                  // 10 per keyframe: GetBestCovisibilityKeyFrames(10), then -1
        std::vector<uint8_t> ptBad;                  // isBad() per point
        std::vector<int32_t> ptObsOff, ptObsKf;      // the keys of mObservations, ascending per point
        orb_local_map_tables_t abi() const {
            if (kfMpOff.size() != kfBad.size() + 1 || ptObsOff.size() != ptBad.size() + 1 || kfCov.size() != kfBad.size() * 10)
                throw std::invalid_argument("LocalMap::Tables: array sizes disagree");
            orb_local_map_tables_t t;
            t.kf_bad = kfBad.data(), t.kf_mp_off = kfMpOff.data(), t.kf_mp = kfMp.data(), t.kf_cov = kfCov.data();
            t.pt_bad = ptBad.data(), t.pt_obs_off = ptObsOff.data(), t.pt_obs_kf = ptObsKf.data();
            t.n_kf = (int32_t)kfBad.size(), t.n_pt = (int32_t)ptBad.size();
            t.n_kf_mp = (int32_t)kfMp.size(), t.n_obs = (int32_t)ptObsKf.size();
            return t;
        }
    };
    struct Reference {
        std::vector<int32_t> vpMapPoints;      // mCurrentFrame.mvpMapPoints after line 821
        std::vector<int32_t> vpLocalKeyFrames; // mvpLocalKeyFrames
        std::vector<int32_t> vpLocalMapPoints; // mvpLocalMapPoints
        std::vector<uint8_t> vbSeen;           // 1: mnLastFrameSeen == mnId at line 744 (pass !seen as usable)
        orb_local_map_info_t info;             // ref_kf is mpReferenceKF
    };
    // UpdateReference for the frame whose mvpMapPoints is vpMapPoints (point indices or -1).
    static void UpdateReference(const Tables& T, const std::vector<int32_t>& vpMapPoints, Reference& R, int device = 0) {
        const orb_local_map_tables_t t = T.abi();
        const size_t n = vpMapPoints.size();
        R.vpMapPoints.assign(n, -1);
        R.vpLocalKeyFrames.assign(T.kfBad.size(), -1);
        R.vpLocalMapPoints.assign(T.ptBad.size(), -1);
        R.vbSeen.assign(T.ptBad.size(), 0);
        orb_check(orb_local_map_reference(&t, (int)n, vpMapPoints.data(), t.n_kf, t.n_pt, R.vpMapPoints.data(),
                                          R.vpLocalKeyFrames.data(), R.vpLocalMapPoints.data(), R.vbSeen.data(), nullptr,
                                          &R.info, device));
        R.vpLocalKeyFrames.resize((size_t)R.info.n_local_kf);
        R.vpLocalMapPoints.resize((size_t)R.info.n_local_pt);
        R.vbSeen.resize((size_t)R.info.n_local_pt);
    }

    struct Connections {
        std::vector<int32_t> connKF, connW;  // mConnectedKeyFrameWeights, ascending index
        std::vector<int32_t> ordKF, ordW;    // mvpOrderedConnectedKeyFrames / mvOrderedWeights
        bool unchanged;                      // the early return of line 365: write nothing back
    };
    // UpdateConnections of the keyframes vKF, each on its own.
    static void UpdateConnections(const Tables& T, const std::vector<int32_t>& vKF, std::vector<Connections>& R,
                                  int device = 0) {
        const orb_local_map_tables_t t = T.abi();
        const size_t K = vKF.size(), cap = T.kfBad.size();
        std::vector<int32_t> ck(K * cap), cw(K * cap), ok(K * cap), ow(K * cap);
        std::vector<orb_update_connections_info_t> info(K);
        orb_check(orb_keyframe_update_connections(&t, (int)K, vKF.data(), (int)cap, (int)cap, ck.data(), cw.data(), ok.data(),
                                                  ow.data(), info.data(), device));
        R.assign(K, Connections());
        for (size_t q = 0; q < K; ++q) {
            const size_t nc = (size_t)info[q].n_conn, no = (size_t)info[q].n_ord;
            R[q].connKF.assign(ck.begin() + q * cap, ck.begin() + q * cap + nc);
            R[q].connW.assign(cw.begin() + q * cap, cw.begin() + q * cap + nc);
            R[q].ordKF.assign(ok.begin() + q * cap, ok.begin() + q * cap + no);
            R[q].ordW.assign(ow.begin() + q * cap, ow.begin() + q * cap + no);
            R[q].unchanged = info[q].unchanged != 0;
        }
    }
};

}  // namespace gpu
}  // namespace ORB_SLAM

#endif
