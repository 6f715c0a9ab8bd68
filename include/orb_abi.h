/*
 * orb_abi.h — C ABI of the MI355X-native ORB front end (liborb_hip.so).
 *
 * Drop-in boundary for the reference's per-frame feature front end:
 *   ORB_SLAM::ORBextractor (reference include/ORBextractor.h:30-80, src/ORBextractor.cc:457-822)
 *   ORB_SLAM::ORBmatcher   (reference include/ORBmatcher.h:36-108, src/ORBmatcher.cc)
 * Plain pointers and sizes only; no C++ types, no exceptions across the boundary.
 * Every entry point returns an int status: ORB_OK (0) or a negative errno-style code.
 *
 * Threading mirrors the reference: an extractor handle owns one HIP stream plus its
 * device workspace and is used by one host thread at a time (the reference extractor is
 * stateful, ORBextractor.h:74-75).  Distinct handles may run concurrently, on the same
 * or on different devices.
 */
#ifndef ORB_ABI_H
#define ORB_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ------------------------------------------------------------------ */
#define ORB_OK 0
#define ORB_EINVAL (-22)   /* bad argument / unsupported configuration                  */
#define ORB_ENOMEM (-12)   /* device or host allocation failed                          */
#define ORB_ERANGE (-34)   /* output capacity too small                                 */
#define ORB_EDEVICE (-5)   /* HIP runtime error (message via orb_last_error)           */
#define ORB_ENOTSUP (-95)  /* configuration the reference itself cannot run            */

/* ---- score types (reference ORBextractor.h:36) ------------------------------------- */
#define ORB_HARRIS_SCORE 0
#define ORB_FAST_SCORE 1

/* Keypoint record, layout-identical to cv::KeyPoint (OpenCV 2.4, 28 bytes) and to the
 * on-disk record of reference include/SaveLoadWorld.h:1406-1425. */
typedef struct orb_keypoint {
    float x, y;        /* pt, image (level-0) pixel coordinates                       */
    float size;        /* (int)(31 * scaleFactor^octave)                              */
    float angle;       /* degrees in [0, 360], IC_Angle via fastAtan2                 */
    float response;    /* FAST score (or Harris response)                             */
    int32_t octave;    /* pyramid level                                               */
    int32_t class_id;  /* always -1                                                   */
} orb_keypoint_t;

typedef struct orb_extractor orb_extractor_t; /* opaque handle */

/* Last error message of the calling thread (never NULL). */
const char* orb_last_error(void);

/* Library build identifier, e.g. "orb_hip gfx950 <date>". */
const char* orb_version(void);

/* ---- ORBextractor ------------------------------------------------------------------ */
/* Replaces ORBextractor::ORBextractor(nfeatures, scaleFactor, nlevels, scoreType, fastTh)
 * (reference ORBextractor.h:38, ORBextractor.cc:457-511).  `device` is the HIP ordinal;
 * `max_batch` sizes the device workspace for orb_extract_batch_device (>= 1). */
int orb_extractor_create(int nfeatures, float scale_factor, int nlevels, int score_type, int fast_th,
                         int device, int max_batch, orb_extractor_t** out);
int orb_extractor_destroy(orb_extractor_t* h);

/* ORBextractor::GetLevels / GetScaleFactor (reference ORBextractor.h:47-51). */
int orb_get_levels(const orb_extractor_t* h);
float orb_get_scale_factor(const orb_extractor_t* h);
/* Per-frame keypoint capacity of the batched entry points: sum of the per-level quotas
 * (== nfeatures for every configuration whose rounded quotas do not overshoot). */
int orb_get_max_keypoints(const orb_extractor_t* h);
/* Per-level quotas (mnFeaturesPerLevel, ORBextractor.cc:476-487) and scale factors
 * (mvScaleFactor, ORBextractor.cc:462-465); arrays of length orb_get_levels(). */
int orb_get_level_info(const orb_extractor_t* h, int* features_per_level, float* scale_factors);

/* ORBextractor::operator()(image, mask=cv::Mat(), keypoints, descriptors)
 * (reference ORBextractor.cc:718-779) on ONE host image.
 *   img: u8 grayscale, w x h, row pitch `stride` bytes (continuous or strided, CV_8UC1).
 *   kps_out: capacity `kps_cap` records; desc_out: capacity kps_cap x 32 bytes (row-major).
 *   *n_out: number of keypoints written (<= nfeatures).  Order = the reference's order:
 *   level-major, cells row-major, libstdc++ nth_element permutation inside retainBest.
 * An empty image (w == 0 or h == 0) returns ORB_OK with *n_out = 0 and touches nothing,
 * like the reference's early return (ORBextractor.cc:721-722).  The mask is ignored by the
 * reference's FAST (ORBextractor.cc:601-607) and is not part of this ABI. */
int orb_extract(orb_extractor_t* h, const uint8_t* img, int w, int hgt, int stride, orb_keypoint_t* kps_out,
                int kps_cap, uint8_t* desc_out, int* n_out);

/* Batched extraction on device-resident frames (the GPU-native entry point).
 *   d_imgs: B frames, frame k at d_imgs + k*frame_pitch, each w x h at row pitch `stride`.
 *   d_kps: B x cap records, cap = orb_get_max_keypoints(h) (frame k at d_kps + k*cap);
 *   d_desc: B x cap x 32 bytes; d_counts: B int32 keypoint counts.
 *   stream: hipStream_t to enqueue on (NULL = the null stream, as in every HIP API; the
 *   handle's own stream serves only the host-buffer entry points).  Asynchronous: returns
 *   after enqueueing; work on other streams must be ordered against it by the caller
 *   (events), and the stream synchronised before reading outputs. */
int orb_extract_batch_device(orb_extractor_t* h, int B, const uint8_t* d_imgs, int w, int hgt, int stride,
                             int64_t frame_pitch, orb_keypoint_t* d_kps, uint8_t* d_desc, int32_t* d_counts,
                             void* stream);

/* Host-buffer batch: copies B host frames in, runs, copies results out (synchronous).
 * kps_out / desc_out / n_out laid out as for the device variant. */
int orb_extract_batch(orb_extractor_t* h, int B, const uint8_t* imgs, int w, int hgt, int stride,
                      int64_t frame_pitch, orb_keypoint_t* kps_out, uint8_t* desc_out, int32_t* n_out);

/* Colour frames: Tracking::GrabImage's cvtColor(image, im, mbRGB ? CV_RGB2GRAY : CV_BGR2GRAY)
 * (reference Tracking.cc:202-207; OpenCV 2.4 fixed-point luma, exact) fused into the level-0
 * pass, then the same extraction.  channels 3 or 4 (interleaved u8, row pitch `stride` bytes >=
 * w * channels); rgb != 0 for RGB channel order, 0 for BGR.  Otherwise as orb_extract_batch_device
 * / orb_extract. */
int orb_extract_batch_device_color(orb_extractor_t* h, int B, const uint8_t* d_imgs, int w, int hgt, int stride,
                                   int64_t frame_pitch, int channels, int rgb, orb_keypoint_t* d_kps, uint8_t* d_desc,
                                   int32_t* d_counts, void* stream);
int orb_extract_color(orb_extractor_t* h, const uint8_t* img, int w, int hgt, int stride, int channels, int rgb,
                      orb_keypoint_t* kps_out, int kps_cap, uint8_t* desc_out, int* n_out);

/* ---- ORBmatcher -------------------------------------------------------------------- */
/* ORBmatcher::DescriptorDistance (reference ORBmatcher.cc:1794-1810; DBoW2 FORB.cpp:81-101). */
int orb_descriptor_distance(const uint8_t* a, const uint8_t* b);

/* Frame geometry needed by Frame::GetFeaturesInArea / PosInGrid (reference Frame.cc:73-86,
 * 200-277): image bounds (mnMinX..mnMaxY, from the first frame) of the 64 x 48 grid. */
typedef struct orb_frame_bounds {
    int min_x, max_x, min_y, max_y;
} orb_frame_bounds_t;

/* ORBmatcher(nnratio, checkOri).SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12,
 * windowSize) (reference ORBmatcher.cc:598-713) for ONE frame pair, host buffers.
 *   kps1/desc1 (n1), kps2/desc2 (n2): the frames' mvKeysUn and mDescriptors.
 *   prev_xy: n1 x 2 floats, vbPrevMatched, updated in place (ORBmatcher.cc:707-710).
 *   matches12: n1 ints, vnMatches12 (-1 = unmatched).  Returns nmatches in *n_matches. */
int orb_search_for_initialization(const orb_keypoint_t* kps1, const uint8_t* desc1, int n1,
                                  const orb_keypoint_t* kps2, const uint8_t* desc2, int n2,
                                  orb_frame_bounds_t bounds, float nnratio, int check_ori, int window,
                                  float* prev_xy, int32_t* matches12, int* n_matches);

/* Batched SearchForInitialization on device-resident extractor output.
 * Pair p matches frame pair_f1[p] against frame pair_f2[p] of a batch laid out as by
 * orb_extract_batch_device (d_kps / d_desc / d_counts with per-frame capacity `cap`).
 *   d_prev_xy: P x cap x 2 floats (in/out); NULL means "vbPrevMatched = F1 keypoints"
 *              (Tracking::FirstInitialization, reference Tracking.cc:366-368) and no update.
 *   d_matches12: P x cap int32; d_nmatches: P int32.  d_desc 16-B aligned.  Asynchronous on
 *   `stream`.
 * cap <= 8192.  One workgroup per pair holds up to nmax octave-0 keypoints per frame in LDS:
 * nmax = min(cap, 1024) for P < 256 pairs, min(cap, 1024, max(256, ~9/40 cap)) otherwise (the
 * extractor keeps at most 0.217 nFeatures at level 0).  A pair over nmax (another producer, the
 * reference init extractor's nFeatures*2 at 1280x720) is redone exactly by the same workgroup
 * with its staged arrays in a grow-only scratch kept per (device, stream); every pair is exact
 * and there is one launch per call. */
int orb_search_for_initialization_batch_device(const orb_keypoint_t* d_kps, const uint8_t* d_desc,
                                               const int32_t* d_counts, int cap, int P, const int32_t* d_pair_f1,
                                               const int32_t* d_pair_f2, orb_frame_bounds_t bounds, float nnratio,
                                               int check_ori, int window, float* d_prev_xy, int32_t* d_matches12,
                                               int32_t* d_nmatches, void* stream);
/* Release the large-capacity scratch kept for `stream` on the current device (freed in stream
 * order, after the launches already queued on it).  Call before destroying a stream that ran
 * orb_search_for_initialization_batch_device; a later call on the stream re-creates it.  No
 * reference counterpart (resource hook of the batched entry point). */
int orb_match_release_stream_scratch(void* stream);
/* A HIP stream on the current device with a hardware queue of its own, for callers that
 * overlap H2D copies, extraction and D2H copies on separate streams (the host-fed step of
 * ORBextractor::operator() callers, bench.py host_fed).  Plain streams share the runtime's
 * GPU_MAX_HW_QUEUES hardware queues (4 by default) round-robin, so a copy stream can land on
 * the queue of an extraction stream and serialise behind it; this stream is created with a CU
 * mask naming every CU of the device (hipExtStreamCreateWithCUMask), which the runtime serves
 * from a queue of its own whatever GPU_MAX_HW_QUEUES says.  Non-blocking w.r.t. the null stream
 * is NOT implied (order it with events).  orb_stream_destroy releases it (and the matcher scratch
 * kept for it).  No reference counterpart (resource hook). */
int orb_stream_create_dedicated(void** out_stream);
int orb_stream_destroy(void* stream);

/* ---- the rest of the ORBmatcher family (GPU: csrc/orb_match.hip) ------------------- */
/* All entry points below take HOST buffers, run on the device of `device`, and are
 * synchronous.  Map state the reference reads through MapPoint / KeyFrame methods
 * (isBad, IsInKeyFrame, "already found" sets, outlier flags) arrives as caller-evaluated
 * per-element `usable` / `taken` flags; each entry point names the reference condition its
 * flags encode.  Results are indices (the caller maps them back to MapPoint*), so no map
 * object crosses the boundary.  Pose-level cv::Mat algebra the reference performs once per
 * call (Scw decomposition, Sim3 composition, -R^T t) is done by the caller with the
 * reference's own expressions and passed in; the per-point geometry runs on the device. */

#define ORB_MAX_VIEW_LEVELS 16

/* A Frame or KeyFrame as the matchers see it (reference Frame.h:43-138, KeyFrame.h). */
typedef struct orb_frame_view {
    const orb_keypoint_t* kps;  /* mvKeysUn, n records                                   */
    const uint8_t* desc;        /* mDescriptors, n x 32 bytes row-major                  */
    int32_t n;
    int32_t nlevels;            /* mnScaleLevels (<= ORB_MAX_VIEW_LEVELS)                */
    orb_frame_bounds_t bounds;  /* mnMinX .. mnMaxY; grid = 64 x 48 cells over them       */
    float scale_factors[ORB_MAX_VIEW_LEVELS]; /* mvScaleFactors (Frame.cc:95-103)        */
    float level_sigma2[ORB_MAX_VIEW_LEVELS];  /* mvLevelSigma2                           */
    float fx, fy, cx, cy;       /* calibration                                            */
    float Rcw[9];               /* rotation world->camera, row-major (mRcw / GetRotation) */
    float tcw[3];               /* translation (mtcw / GetTranslation)                    */
    float Ow[3];                /* camera centre (mOw / GetCameraCenter)                  */
} orb_frame_view_t;

/* MapPoint attributes read by the projection matchers (reference MapPoint.h). */
typedef struct orb_map_points {
    const float* pos;     /* n x 3 GetWorldPos                                            */
    const float* normal;  /* n x 3 GetNormal (NULL where unused)                          */
    const float* dmin;    /* n GetMinDistanceInvariance (NULL where unused)               */
    const float* dmax;    /* n GetMaxDistanceInvariance (NULL where unused)               */
    const uint8_t* desc;  /* n x 32 GetDescriptor (NULL where the frame's row is used)    */
    int32_t n;
} orb_map_points_t;

/* DBoW2::FeatureVector (std::map<NodeId, vector<unsigned>>, FeatureVector.h:21-49) as CSR:
 * ascending node ids nodes[n_nodes], offsets[n_nodes + 1], feature indices features[]. */
typedef struct orb_feature_vector {
    const uint32_t* nodes;
    const int32_t* offsets;
    const int32_t* features;
    int32_t n_nodes;
} orb_feature_vector_t;

/* Frame::GetFeaturesInArea (Frame.cc:200-265) for q query windows (min/max level -1 = any),
 * or KeyFrame::GetFeaturesInArea (KeyFrame.cc:612-652, no level filter, `<= r`) when
 * keyframe != 0.  Output CSR: out_offsets[q + 1], out_indices[capacity]; ORB_ERANGE if the
 * candidates exceed `capacity` (out_offsets[q] then holds the required size). */
int orb_features_in_area(const orb_frame_view_t* view, int keyframe, int q, const float* x, const float* y,
                         const float* r, const int32_t* min_level, const int32_t* max_level, int32_t* out_offsets,
                         int32_t* out_indices, int capacity, int device);

/* Frame::isInFrustum (Frame.cc:137-198) for every MapPoint: in_view[i] (mbTrackInView),
 * proj_x/proj_y (mTrackProjX/Y), level (mnTrackScaleLevel), view_cos (mTrackViewCos).
 * mps.normal/dmin/dmax required. */
int orb_frame_is_in_frustum(const orb_frame_view_t* F, orb_map_points_t mps, float viewing_cos_limit,
                            uint8_t* in_view, float* proj_x, float* proj_y, int32_t* level, float* view_cos,
                            int device);

/* SearchByBoW(KeyFrame*, Frame&, vpMapPointMatches) (ORBmatcher.cc:155-284).
 * kf_usable[i]: vpMapPointsKF[i] && !isBad().  f_match[j] = KF keypoint whose MapPoint is
 * matched to F keypoint j, or -1. */
int orb_search_by_bow_kf_f(const orb_frame_view_t* KF, const uint8_t* kf_usable, orb_feature_vector_t kf_fv,
                           const orb_frame_view_t* F, orb_feature_vector_t f_fv, float nnratio, int check_ori,
                           int32_t* f_match, int* n_matches, int device);

/* SearchByBoW(KeyFrame*, KeyFrame*, vpMatches12) (ORBmatcher.cc:715-850).
 * usable1/usable2: vpMapPoints[i] && !isBad().  match12[i1] = idx2 or -1. */
int orb_search_by_bow_kf_kf(const orb_frame_view_t* KF1, const uint8_t* usable1, orb_feature_vector_t fv1,
                            const orb_frame_view_t* KF2, const uint8_t* usable2, orb_feature_vector_t fv2,
                            float nnratio, int check_ori, int32_t* match12, int* n_matches, int device);

/* SearchByBoW over many pairs per launch, on device-resident extractor output
 * (orb_extract_batch_device: d_kps / d_desc [B][cap], d_counts[B]) and the FeatureVectors of the
 * same frames (orb_vocabulary_transform_batch_device: d_fv_nodes [B][cap], d_fv_offsets
 * [B][cap + 1], d_fv_features [B][cap], d_fv_n [B]).  Pair p = frames (d_pair_a[p], d_pair_b[p]):
 *   kf_kf = 0: SearchByBoW(KeyFrame* = frame a, Frame& = frame b, vpMapPointMatches)
 *              (ORBmatcher.cc:155-284; Tracking.cc:927 with nnratio 0.7): d_match[p][j] = the
 *              frame-a keypoint matched to frame-b keypoint j, or -1;
 *   kf_kf = 1: SearchByBoW(KeyFrame* = a, KeyFrame* = b, vpMatches12) (ORBmatcher.cc:715-850;
 *              LoopClosing.cc:278 with 0.75): d_match[p][i1] = idx2 in frame b, or -1.
 * d_usable [B][cap]: the frame's keypoint has a MapPoint that is not bad (both sides for kf_kf =
 * 1, the KF side for kf_kf = 0); NULL = every keypoint.  d_match rows are written whole (-1 past
 * the count); d_nmatches[p] = the reference's return value.  cap <= 8192, d_desc 16-B aligned.
 * Each feature of a frame must appear in exactly one node of its FeatureVector, as
 * orb_vocabulary_transform_batch_device produces it: the nodes of a pair are resolved
 * independently of each other (one wave each), which is the reference's node-by-node loop only
 * while no two nodes share a keypoint.  The host entry points (orb_search_by_bow_kf_f / _kf_kf)
 * check this and route a vector that lists a feature twice to the generic sequential resolver.
 * Asynchronous on `stream`. */
int orb_search_by_bow_batch_device(int kf_kf, const orb_keypoint_t* d_kps, const uint8_t* d_desc,
                                   const int32_t* d_counts, int cap, const uint32_t* d_fv_nodes,
                                   const int32_t* d_fv_offsets, const int32_t* d_fv_features, const int32_t* d_fv_n,
                                   int P, const int32_t* d_pair_a, const int32_t* d_pair_b, const uint8_t* d_usable,
                                   float nnratio, int check_ori, int32_t* d_match, int32_t* d_nmatches, void* stream);

/* SearchForTriangulation(KF1, KF2, F12, ...) (ORBmatcher.cc:852-1014) with
 * CheckDistEpipolarLine (136-153).  has_mp1/has_mp2: GetMapPointMatches()[i] != NULL.
 * F12 row-major 3x3.  match12[i1] = idx2 or -1 (vMatchedPairs = the i1 with match12 >= 0,
 * ascending). */
int orb_search_for_triangulation(const orb_frame_view_t* KF1, const uint8_t* has_mp1, orb_feature_vector_t fv1,
                                 const orb_frame_view_t* KF2, const uint8_t* has_mp2, orb_feature_vector_t fv2,
                                 const float* F12, float nnratio, int check_ori, int32_t* match12, int* n_matches,
                                 int device);

/* WindowSearch(F1, F2, windowSize, vpMapPointMatches2, minScaleLevel, maxScaleLevel)
 * (ORBmatcher.cc:409-516).  usable1[i1]: F1.mvpMapPoints[i1] && !isBad().
 * match21[i2] = i1 whose MapPoint lands on F2 keypoint i2, or -1. */
int orb_window_search(const orb_frame_view_t* F1, const uint8_t* usable1, const orb_frame_view_t* F2, int window,
                      int min_scale_level, int max_scale_level, float nnratio, int check_ori, int32_t* match21,
                      int* n_matches, int device);

/* SearchByProjection(Frame& F, vector<MapPoint*>, th) (ORBmatcher.cc:49-125) over MapPoints
 * already projected by Frame::isInFrustum.  usable[i]: mbTrackInView && !isBad();
 * f_taken[j]: F.mvpMapPoints[j] != NULL on entry.  f_match[j] = MapPoint index newly
 * assigned to F keypoint j, or -1. */
int orb_search_by_projection_local(const orb_frame_view_t* F, const uint8_t* f_taken, int n_mp, const uint8_t* usable,
                                   const float* proj_x, const float* proj_y, const int32_t* level,
                                   const float* view_cos, const uint8_t* mp_desc, float th, float nnratio,
                                   int32_t* f_match, int* n_matches, int device);

/* SearchByProjection(Frame& F1, Frame& F2, windowSize, vpMapPointMatches2)
 * (ORBmatcher.cc:519-594).  mp1.pos: F1's MapPoint positions (row i1); usable1[i1]:
 * pMP1 && !isBad() && not already in F2.mvpMapPoints; f2_taken[i2]: F2.mvpMapPoints[i2].
 * match2[i2] = i1 newly assigned, or -1. */
int orb_search_by_projection_f2f(const orb_frame_view_t* F1, orb_map_points_t mp1, const uint8_t* usable1,
                                 const orb_frame_view_t* F2, const uint8_t* f2_taken, int window, float nnratio,
                                 int32_t* match2, int* n_matches, int device);

/* SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th) (ORBmatcher.cc:
 * 1507-1620).  usable[i]: LastFrame.mvpMapPoints[i] && !mvbOutlier[i]; mp.pos row i.
 * cur_match[j] = LastFrame index newly assigned to Current keypoint j, or -1. */
int orb_search_by_projection_motion(const orb_frame_view_t* Cur, const uint8_t* cur_taken, const orb_frame_view_t* Last,
                                    orb_map_points_t mp, const uint8_t* usable, float th, int check_ori,
                                    int32_t* cur_match, int* n_matches, int device);

/* SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, sAlreadyFound, th, ORBdist)
 * (ORBmatcher.cc:1622-1746).  mp: the KF's MapPoints (pos, dmin, desc) row i; usable[i]:
 * pMP && !isBad() && !sAlreadyFound.count(pMP).  Cur->Ow = -Rcw^T tcw of the current pose. */
int orb_search_by_projection_reloc(const orb_frame_view_t* Cur, const uint8_t* cur_taken, const orb_frame_view_t* KF,
                                   orb_map_points_t mp, const uint8_t* usable, float th, int orb_dist,
                                   int check_ori, int32_t* cur_match, int* n_matches, int device);

/* SearchByProjection(KeyFrame* pKF, cv::Mat Scw, vpPoints, vpMatched, th) (ORBmatcher.cc:
 * 286-407).  KF->Rcw/tcw/Ow = the Scw decomposition of 297-302; usable[i]: !isBad() &&
 * !spAlreadyFound.count(pMP); kf_taken[j]: vpMatched[j].  kf_match[j] = point index or -1. */
int orb_search_by_projection_sim3(const orb_frame_view_t* KF, const uint8_t* kf_taken, orb_map_points_t pts,
                                  const uint8_t* usable, int th, int32_t* kf_match, int* n_matches, int device);

/* SearchBySim3(KF1, KF2, vpMatches12, s12, R12, t12, th) (ORBmatcher.cc:1267-1505).
 * mp1/mp2: the keyframes' MapPoints (pos, dmin, dmax, desc) by keypoint index; usable1/2:
 * pMP && !vbAlreadyMatched && !isBad().  sR12 = s12*R12, sR21 = (1/s12)*R12^T,
 * t21 = -sR21*t12 as the reference computes them (1288-1290).  match12[i1] = idx2 for the
 * mutually agreeing pairs, -1 elsewhere; *n_found = their count. */
int orb_search_by_sim3(const orb_frame_view_t* KF1, orb_map_points_t mp1, const uint8_t* usable1,
                       const orb_frame_view_t* KF2, orb_map_points_t mp2, const uint8_t* usable2, const float* sR12,
                       const float* t12, const float* sR21, const float* t21, float th, int32_t* match12,
                       int* n_found, int device);

/* Fuse(KeyFrame*, vector<MapPoint*>, th) (ORBmatcher.cc:1016-1134) when scw == 0, or
 * Fuse(KeyFrame*, cv::Mat Scw, vpPoints, th) (1136-1265) when scw != 0 (KF pose = the Scw
 * decomposition).  usable[i]: pMP && !isBad() && !IsInKeyFrame (resp. !spAlreadyFound).
 * best_idx[i] = KF keypoint the point fuses with (bestDist <= TH_LOW), or -1; the caller
 * applies Replace / AddObservation in point order (the map mutation stays on the host). */
int orb_fuse(const orb_frame_view_t* KF, orb_map_points_t pts, const uint8_t* usable, float th, int scw,
             int32_t* best_idx, int* n_fused, int device);

/* ---- Frame keypoint geometry (GPU: csrc/orb_frame.hip) ------------------------------ */
/* The camera as Tracking.cc:52-70 builds it: K4 = (fx, fy, cx, cy) of K = [fx 0 cx; 0 fy cy;
 * 0 0 1], dist4 = mDistCoef = (k1, k2, p1, p2).  cv::undistortPoints(pts, pts, K, mDistCoef,
 * noArray(), K) (OpenCV 2.4 cvUndistortPoints: double arithmetic, 5 fixed iterations) is
 * restated exactly on the device.  fx, fy must be finite and non-zero (ORB_EINVAL). */
/* Frame::UndistortKeyPoints (Frame.cc:289-319) over a [B][cap] extractor batch: slot i < counts[b]
 * of d_kps_un = that keypoint with pt undistorted, or copied unchanged when k1 == 0
 * (Frame.cc:291-295).  d_kps_un may equal d_kps.  Asynchronous on `stream`. */
int orb_undistort_keypoints_batch_device(const orb_keypoint_t* d_kps, const int32_t* d_counts, int cap, int B,
                                         const float* K4, const float* dist4, orb_keypoint_t* d_kps_un,
                                         void* stream);
/* The same for one frame's n keypoints in host buffers (synchronous; device -1 = current). */
int orb_undistort_keypoints(const orb_keypoint_t* kps, int n, const float* K4, const float* dist4, int device,
                            orb_keypoint_t* out);
/* cv::undistortPoints itself on n points xy[2n] -> out[2n] (no k1 == 0 shortcut). */
int orb_undistort_points(const float* xy, int n, const float* K4, const float* dist4, int device, float* out);
/* Frame::ComputeImageBounds (Frame.cc:321-349): the undistorted image corners' floor / ceil
 * when k1 != 0, else the image rectangle. */
int orb_compute_image_bounds(int cols, int rows, const float* K4, const float* dist4, int device,
                             orb_frame_bounds_t* out);

/* ---- the front end over a camera stream, overlapped (csrc/orb_pipeline.hip) ---------- */
/* B consecutive frames of one camera: ORBextractor::operator() on each (Frame::Frame,
 * Frame.cc:56-128) and SearchForInitialization(F_b, F_b+1) for b < B-1 with vbPrevMatched =
 * F_b's keypoints (Tracking.cc:366-368, 392-393).  The batch is cut into n_streams contiguous
 * chunks, each with its own extractor handle and HIP stream, so latency-bound kernels of
 * one chunk overlap the others; outputs equal the serial path's.  One handle = one caller. */
typedef struct orb_pipeline orb_pipeline_t; /* opaque handle */
int orb_pipeline_create(int nfeatures, float scale_factor, int nlevels, int score_type, int fast_th, int device,
                        int max_batch, int n_streams, orb_pipeline_t** out);
int orb_pipeline_destroy(orb_pipeline_t* p);
int orb_pipeline_max_keypoints(const orb_pipeline_t* p);
int orb_pipeline_streams(const orb_pipeline_t* p);
/* Outputs as orb_extract_batch_device (d_kps/d_desc/d_counts, per-frame capacity
 * orb_pipeline_max_keypoints) and orb_search_for_initialization_batch_device (pair b = (b, b+1):
 * d_matches12 (B-1) x cap, d_nmatches B-1).  Ordered after earlier work on `stream` and
 * before later work on it (events); asynchronous. */
int orb_pipeline_extract_and_match(orb_pipeline_t* p, int B, const uint8_t* d_imgs, int w, int hgt, int stride,
                                   int64_t frame_pitch, orb_keypoint_t* d_kps, uint8_t* d_desc, int32_t* d_counts,
                                   orb_frame_bounds_t bounds, float nnratio, int check_ori, int window,
                                   int32_t* d_matches12, int32_t* d_nmatches, void* stream);
/* The same step for a calibrated camera with distortion (Frame::Frame: UndistortKeyPoints,
 * Frame.cc:69): after each chunk's extraction its keypoints are undistorted into d_kps_un
 * (orb_undistort_keypoints_batch_device; K4 / dist4 as there) and the pairs are matched on
 * mvKeysUn, with `bounds` = orb_compute_image_bounds of the camera.  K4 = NULL is
 * orb_pipeline_extract_and_match (d_kps_un unused). */
int orb_pipeline_extract_undistort_and_match(orb_pipeline_t* p, int B, const uint8_t* d_imgs, int w, int hgt,
                                             int stride, int64_t frame_pitch, const float* K4, const float* dist4,
                                             orb_keypoint_t* d_kps, orb_keypoint_t* d_kps_un, uint8_t* d_desc,
                                             int32_t* d_counts, orb_frame_bounds_t bounds, float nnratio,
                                             int check_ori, int window, int32_t* d_matches12, int32_t* d_nmatches,
                                             void* stream);
/* Per-stage HIP-event timing summed over the chunk handles (see orb_profile_*). */
int orb_pipeline_profile_enable(orb_pipeline_t* p, int enable);
int orb_pipeline_profile_read(orb_pipeline_t* p, double* stage_ms, int64_t* stage_launches, int nstages);

/* ---- MapPoint descriptor maintenance (GPU: csrc/orb_mappoint.hip) ------------------- */
/* MapPoint::ComputeDistinctiveDescriptors (reference src/MapPoint.cc:185-250) for M points:
 * point m's observed descriptors are rows offsets[m] .. offsets[m+1]-1 of desc (32 B each), in
 * the order of its std::map<KeyFrame*, size_t> observations; usable[r] = !pKF->isBad() for the
 * keyframe of row r (NULL = all).  best_row[m] = the row chosen as mDescriptor and
 * out_desc[m] = its bytes, or best_row[m] = -1 and out_desc[m] untouched when no row is usable
 * (the reference returns without changing mDescriptor).  <= 4000 rows per point.
 * Host buffers, synchronous. */
int orb_compute_distinctive_descriptors(int M, const int32_t* offsets, const uint8_t* desc, const uint8_t* usable,
                                        int32_t* best_row, uint8_t* out_desc, int device);
/* The same on device buffers (desc 16-B aligned); max_obs = the largest row count of a point.
 * Asynchronous on `stream`. */
int orb_compute_distinctive_descriptors_device(int M, const int32_t* d_offsets, const uint8_t* d_desc,
                                               const uint8_t* d_usable, int max_obs, int32_t* d_best_row,
                                               uint8_t* d_out_desc, void* stream);

/* MapPoint::UpdateNormalAndDepth (reference src/MapPoint.cc:273-312) for M points: point m is seen
 * from the camera centres obs_Ow rows offsets[m] .. offsets[m+1]-1 (R x 3, GetCameraCenter of each
 * observing keyframe), in the order of its std::map<KeyFrame*, size_t> observations: the float
 * sum of the unit vectors depends on that order, which is the caller's, as for the descriptors.
 * pos M x 3 (mWorldPos), ref_Ow M x 3 (mpRefKF->GetCameraCenter()), ref_level M (the octave of the
 * point's keypoint in mpRefKF; clamped to the table), scale_factors / nlevels: the reference
 * keyframe's mvScaleFactors, one table for the call (2..16 levels: GetScaleFactor() is entry 1).
 * Outputs, each may be NULL: normal M x 3 (mNormalVector), dmin / dmax M (mfMinDistance,
 * mfMaxDistance).  A point without an observation yields a NaN normal (the reference's 0 * inf);
 * mbBad points are the caller's to leave out.  <= 4000 observations per point (ORB_ENOTSUP).
 * Host buffers, synchronous. */
int orb_update_normal_and_depth(int M, const int32_t* offsets, const float* obs_Ow, const float* pos,
                                const float* ref_Ow, const int32_t* ref_level, const float* scale_factors, int nlevels,
                                float* normal, float* dmin, float* dmax, int device);
/* The same on device buffers (scale_factors stays a host table); max_obs = the largest row count of
 * a point: no point is walked further.  Asynchronous on `stream`. */
int orb_update_normal_and_depth_device(int M, const int32_t* d_offsets, const float* d_obs_Ow, const float* d_pos,
                                       const float* d_ref_Ow, const int32_t* d_ref_level, const float* scale_factors,
                                       int nlevels, int max_obs, float* d_normal, float* d_dmin, float* d_dmax,
                                       void* stream);

/* ---- LocalMapping::CreateNewMapPoints (GPU: csrc/orb_localmap.hip) ----- */
/* LocalMapping::ComputeF12 (reference src/LocalMapping.cc:474-491) from the two views' Rcw, tcw and
 * calibration: F12 row-major 3 x 3, the matrix orb_search_for_triangulation takes.  Computed on the
 * host by the function the kernels use; nothing is refused but a NULL argument. */
int orb_compute_f12(const orb_frame_view_t* KF1, const orb_frame_view_t* KF2, float* F12);

/* KeyFrame::ComputeSceneMedianDepth(q) (reference src/KeyFrame.cc:659-689): sorted depths[(n - 1) / q]
 * of the MapPoints of KF (mp_pos n x 3 GetWorldPos, has_mp n: mvpMapPoints[i] != NULL).  A NaN depth
 * sorts after every number.  With no MapPoint the reference indexes an empty vector: ORB_EINVAL.
 * Host buffers, synchronous. */
int orb_scene_median_depth(const orb_frame_view_t* KF, const float* mp_pos, const uint8_t* has_mp, int q, float* depth,
                           int device);
/* The same for B keyframes on device buffers: d_counts B (clamped to [0, cap]), d_pose B x 12 (Rcw
 * row-major, tcw), d_mp_pos B x cap x 3, d_has_mp B x cap.  d_depth B (NaN for a keyframe without a
 * MapPoint) and d_n B (the number of depths) may be NULL.  cap <= 8192, B <= 65535.  Asynchronous on
 * `stream`. */
int orb_scene_median_depth_batch_device(const int32_t* d_counts, int cap, int B, const float* d_pose,
                                        const float* d_mp_pos, const uint8_t* d_has_mp, int q, float* d_depth,
                                        int32_t* d_n, void* stream);

/* The body of CreateNewMapPoints' neighbour loop for one pair (reference src/LocalMapping.cc:256-265,
 * 276-391): KF1 = mpCurrentKeyFrame, KF2 = the neighbour, match12[i1] = idx2 or -1 as
 * orb_search_for_triangulation leaves it (an entry outside [-1, n2) is ORB_EINVAL).  The matches are
 * walked in ascending i1, the order of vMatchedIndices.  mp_pos2 n2 x 3 / has_mp2 n2 (KF2's MapPoints, as
 * for orb_scene_median_depth) feed the baseline gate, baseline / ComputeSceneMedianDepth(2) < 0.01; both
 * NULL: no gate.  Outputs, each may be NULL:
 *   x3d n1 x 3      the point of slot i1 where the match got as far as the Euclidean point (status 1
 *                   and 4..9), zeros elsewhere
 *   status n1       0 no match, 1 accepted (the reference creates a MapPoint), 2 ray parallax, 3 w == 0,
 *                   4 z1 <= 0, 5 z2 <= 0, 6 reprojection in KF1, 7 reprojection in KF2, 8 a zero
 *                   distance, 9 scale ratio: the statement that ended the match
 *   cos_rays n1     cosParallaxRays of every match, NaN elsewhere
 *   n_new, new_idx1 / new_idx2 n1: the accepted pairs, dense, ascending i1, -1 past n_new
 *   skipped         0, or 1: the baseline gate's `continue` (nothing is triangulated, n_new = 0)
 *   median_depth    ComputeSceneMedianDepth(2) of KF2 where the gate ran, NaN otherwise
 * A NaN fails no comparison of the reference, so a NaN point passes every gate and is reported
 * accepted; a non-finite Rcw, tcw, Ow or calibration value is therefore refused here (ORB_EINVAL, naming
 * the argument), as is a gate on a KF2 without a MapPoint.  An octave outside the level table is clamped.
 * n <= 8192 (ORB_ENOTSUP), nlevels 2..16 (GetScaleFactor() is entry 1 of scale_factors).
 * Host buffers, synchronous. */
int orb_create_new_map_points(const orb_frame_view_t* KF1, const orb_frame_view_t* KF2, const int32_t* match12,
                              const float* mp_pos2, const uint8_t* has_mp2, float* x3d, uint8_t* status,
                              float* cos_rays, int32_t* n_new, int32_t* new_idx1, int32_t* new_idx2, int32_t* skipped,
                              float* median_depth, int device);
/* P pairs on device-resident data, laid out as for orb_optimize_sim3_batch_device: pair p = keyframes
 * (d_pair_a[p] = current, d_pair_b[p] = neighbour) of a batch (d_kps / d_counts, capacity cap; the
 * undistorted records), row p of d_match (P x cap, d_match[p][i1] = idx2), d_pose B x 12 (Rcw
 * row-major, tcw); the camera centres are -Rcw.t()*tcw computed as the reference's one gemm.
 * d_mp_pos B x cap x 3 and d_has_mp B x cap feed the baseline gate on keyframe d_pair_b[p]; both NULL:
 * no gate.  scale_factors / level_sigma2: nlevels (2..16) host floats, K4: fx, fy, cx, cy, one table and
 * one calibration for the call.  Outputs as above with rows of cap, each may be NULL: d_x3d P x cap x 3,
 * d_status P x cap, d_cos_rays P x cap, d_n_new P, d_new_idx1 / d_new_idx2 P x cap, d_skipped P (2: the
 * neighbour holds no MapPoint, where the reference indexes an empty vector; nothing is triangulated),
 * d_median_depth P (written only where the gate runs; NaN with skipped = 2), d_F12 P x 9 (ComputeF12 of
 * the pair, skipped or not).  Rows are written whole.
 * The match rows are taken as given because the reference's neighbour loop is sequential: a slot of
 * the current keyframe that neighbour i filled is not matched by neighbour i + 1, so the rows of one
 * current keyframe cannot be produced in one matching batch without that dependence.
 * A match entry outside [0, d_counts[b]), or at an index >= d_counts[a], is no match.  The batch form
 * cannot see its device-resident poses: a non-finite one ends as NaN points reported accepted, every
 * loop being bounded.  The pair indices are the caller's to keep in range.  cap <= 8192, P <= 65535
 * (ORB_ENOTSUP).  Asynchronous on `stream`; scratch is stream-ordered. */
int orb_create_new_map_points_batch_device(const orb_keypoint_t* d_kps, const int32_t* d_counts, int cap, int P,
                                           const int32_t* d_pair_a, const int32_t* d_pair_b, const int32_t* d_match,
                                           const float* d_pose, const float* d_mp_pos, const uint8_t* d_has_mp,
                                           const float* scale_factors, const float* level_sigma2, int nlevels,
                                           const float* K4, float* d_x3d, uint8_t* d_status, float* d_cos_rays,
                                           int32_t* d_n_new, int32_t* d_new_idx1, int32_t* d_new_idx2,
                                           int32_t* d_skipped, float* d_median_depth, float* d_F12, void* stream);

/* ---- keyframe feature records of the reference's map files (csrc/orb_persist.hip) ---- */
/* SaveWorldToFile / LoadWroldFromFile (reference include/SaveLoadWorld.h:1254, 2463) store each
 * keyframe's features as one record per stream, little-endian as written on x86-64:
 *   keypoint stream (kfKeyPoints.bin, kfKeyPointsUn.bin; SaveLoadWorld.h:1406-1443, read back at
 *   2098-2160):   0xEB 0x90 | uint64 nKeys | nKeys x 28-byte cv::KeyPoint (= orb_keypoint_t)
 *   descriptor stream (kfDescriptors.bin; SaveLoadWorld.h:1446-1460, read back at 2166-2189):
 *                 0xEB 0x90 | int32 nDes | nDes x 32 bytes
 * Readers report a wrong header through *header_ok = 0 and go on, as the reference's loader
 * prints "header error ..., shouldn't" and keeps reading; a record longer than `len` is
 * ORB_ERANGE.  *consumed = bytes of the record (the next record starts there). */
size_t orb_keypoint_record_bytes(size_t n);
size_t orb_descriptor_record_bytes(int n);
int orb_write_keypoint_record(const orb_keypoint_t* kps, size_t n, uint8_t* out, size_t cap, size_t* written);
int orb_read_keypoint_record(const uint8_t* in, size_t len, orb_keypoint_t* kps, size_t cap, size_t* n,
                             size_t* consumed, int* header_ok);
int orb_write_descriptor_record(const uint8_t* desc, int n, uint8_t* out, size_t cap, size_t* written);
int orb_read_descriptor_record(const uint8_t* in, size_t len, uint8_t* desc, int cap, int* n, size_t* consumed,
                               int* header_ok);
/* B frames of orb_extract_batch_device output (per-frame capacity cap) packed on the device into
 * both streams, one record per frame in frame order (what SaveWorldToFile writes for B keyframes):
 * frame b's keypoint record at d_keys_stream + d_key_offsets[b], its descriptor record at
 * d_des_stream + d_des_offsets[b]; d_*_offsets[B] = the stream lengths (B + 1 int64 each).
 * keys_cap >= B * orb_keypoint_record_bytes(cap), des_cap >= B * orb_descriptor_record_bytes(cap);
 * buffers 2-byte aligned.  Asynchronous on `stream`. */
int orb_pack_keyframe_records_device(const orb_keypoint_t* d_kps, const uint8_t* d_desc, const int32_t* d_counts,
                                     int cap, int B, uint8_t* d_keys_stream, size_t keys_cap, uint8_t* d_des_stream,
                                     size_t des_cap, int64_t* d_key_offsets, int64_t* d_des_offsets, void* stream);

/* ---- DBoW2 vocabulary (GPU: csrc/orb_voc.hip) -------------------------------------- */
/* The reference's ORBVocabulary = DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB>
 * (include/ORBVocabulary.h).  A handle holds the tree on `device`; host entry points are
 * serialised per handle, device entry points enqueue on the caller's stream.
 * Weighting: 0 TF_IDF, 1 TF, 2 IDF, 3 BINARY; scoring: 0 L1_NORM, 1 L2_NORM, 2 CHI_SQUARE,
 * 3 KL, 4 BHATTACHARYYA, 5 DOT_PRODUCT (BowVector.h:36-53). */
typedef struct orb_vocabulary orb_vocabulary_t; /* opaque handle */

/* TemplatedVocabulary::loadFromTextFile (TemplatedVocabulary.h:1338-1424): header
 * "k L scoring weighting", then one line per node "parent isLeaf d0 .. d31 weight".
 * Blank lines are skipped; a malformed line or a parent that does not
 * precede its child is ORB_EINVAL (the reference reads such files unchecked). */
int orb_vocabulary_load_text(const char* path, int device, orb_vocabulary_t** out);
/* The same tree from arrays: node i + 1 (i < n_nodes) has parent[i] (<= i), is_leaf[i],
 * desc[32 i .. 32 i + 31] and weight[i], i.e. the lines of the text format in order. */
int orb_vocabulary_create(int k, int L, int scoring, int weighting, int n_nodes, const int32_t* parent,
                          const uint8_t* is_leaf, const uint8_t* desc, const double* weight, int device,
                          orb_vocabulary_t** out);
int orb_vocabulary_destroy(orb_vocabulary_t* v);
/* info[7] = k, L, scoring, weighting, nodes (root included), words, tree height. */
int orb_vocabulary_info(const orb_vocabulary_t* v, int32_t* info);

/* transform(feature, word_id, weight, &nid, levelsup) (TemplatedVocabulary.h:1217-1259) for
 * n device descriptors (32 B rows, 16-B aligned): word id, weight and the node at level
 * L - levelsup (the root when that level is <= 0).  Asynchronous on `stream`. */
int orb_vocabulary_transform_features_device(const orb_vocabulary_t* v, int n, const uint8_t* d_desc, int levelsup,
                                             uint32_t* d_word, double* d_weight, uint32_t* d_node, void* stream);

/* transform(features, BowVector, FeatureVector, levelsup) (TemplatedVocabulary.h:1126-1194) for
 * B frames laid out as orb_extract_batch_device writes them (frame b: d_desc + b*cap*32,
 * d_counts[b] rows).  Per frame, capacity cap each: d_feat_* per-feature results (as above);
 * BowVector = d_bow_words / d_bow_values[d_bow_n[b]] in ascending word order; FeatureVector
 * = CSR d_fv_nodes[d_fv_n[b]], d_fv_offsets (cap + 1 per frame), d_fv_features.  cap <= 8192.
 * Asynchronous on `stream`. */
int orb_vocabulary_transform_batch_device(const orb_vocabulary_t* v, int B, const uint8_t* d_desc,
                                          const int32_t* d_counts, int cap, int levelsup, uint32_t* d_feat_word,
                                          double* d_feat_weight, uint32_t* d_feat_node, uint32_t* d_bow_words,
                                          double* d_bow_values, int32_t* d_bow_n, uint32_t* d_fv_nodes,
                                          int32_t* d_fv_offsets, int32_t* d_fv_features, int32_t* d_fv_n,
                                          void* stream);

/* The same for one frame of n host descriptors (synchronous); outputs sized n (offsets n + 1). */
int orb_vocabulary_transform(orb_vocabulary_t* v, const uint8_t* desc, int n, int levelsup, uint32_t* bow_words,
                             double* bow_values, int* bow_n, uint32_t* fv_nodes, int32_t* fv_offsets,
                             int32_t* fv_features, int* fv_n);

/* ---- BoW score and KeyFrameDatabase (GPU: csrc/orb_kfdb.hip) ------------------------ */
/* Only L1_NORM vocabularies (ORBvoc is one) are supported: every entry point of this section
 * returns ORB_EINVAL, with orb_last_error naming the scoring type, for a vocabulary of another
 * scoring (orb_kfdb_create refuses it, so no database handle of one exists).  DESIGN.md §8.
 *
 * TemplatedVocabulary::score = L1Scoring::score (ScoringObject.cpp:23-68) of two BowVectors
 * (words ascending): score += fabs(vi - wi) - fabs(vi) - fabs(wi) over the shared words in
 * ascending word order, in double, then -score / 2.  Host buffers, synchronous (computed on the
 * host). */
int orb_vocabulary_score(const orb_vocabulary_t* v, const uint32_t* words1, const double* values1, int n1,
                         const uint32_t* words2, const double* values2, int n2, double* score);
/* The same for P pairs of frames laid out as orb_vocabulary_transform_batch_device writes
 * BowVectors (frame f: d_bow_words / d_bow_values + f * cap, d_bow_n[f] entries):
 * d_score[p] = score(frame d_pair_a[p], frame d_pair_b[p]), the loop of LoopClosing.cc:138-150.
 * The pair indices are the caller's to keep in range.  Every double equals the sequential sum
 * bit for bit.  cap <= 8192.  Asynchronous on `stream`. */
int orb_vocabulary_score_pairs_device(const orb_vocabulary_t* v, int P, const uint32_t* d_bow_words,
                                      const double* d_bow_values, const int32_t* d_bow_n, int cap,
                                      const int32_t* d_pair_a, const int32_t* d_pair_b, double* d_score, void* stream);

/* KeyFrameDatabase (src/KeyFrameDatabase.cc): the keyframes' BowVectors on one device and the
 * two candidate queries.  Keyframe ids are dense integers 0 <= id < max_keyframes chosen by the
 * caller (id = slot; the wrappers map arbitrary ids).  max_keyframes <= 65536; max_entries bounds
 * the (word, value) entries of all live keyframes together.  A handle is serialised: one call at
 * a time.  Host entry points run on the handle's own stream and return when done; a device entry
 * point enqueues on the caller's stream (the default stream included) and records an event
 * there, and the next call on the handle, whichever stream it uses, is ordered after that event:
 * a host call waits for it, a device call makes its stream wait.  The caller's stream may be
 * destroyed once the call has returned. */
typedef struct orb_keyframe_db orb_keyframe_db_t; /* opaque handle */
int orb_kfdb_create(const orb_vocabulary_t* voc, int max_keyframes, int64_t max_entries, int device,
                    orb_keyframe_db_t** out);
int orb_kfdb_destroy(orb_keyframe_db_t* db);
/* KeyFrameDatabase::clear (KeyFrameDatabase.cc:68-72); also forgets every covisibility list. */
int orb_kfdb_clear(orb_keyframe_db_t* db);
/* The number of live keyframes. */
int orb_kfdb_size(const orb_keyframe_db_t* db);
/* KeyFrameDatabase::add (39-45) of a host BowVector: words strictly ascending and below the
 * vocabulary's word count, else ORB_EINVAL; a live id is ORB_EINVAL (the reference would list it
 * twice, and never does); more than 8192 words is ORB_ENOTSUP.  Every add takes the next value of
 * a monotonic counter `seq`, the keyframe's position in every inverted list of the reference.
 * The keyframe's stored reloc score starts at 0.0f (the reference leaves mRelocScore
 * uninitialised, KeyFrame.cc:33; its map loader sets 0, SaveLoadWorld.h:402).  When the pool's
 * tail has no room the pool is compacted on the device first; ORB_ERANGE only when live entries
 * + n > max_entries. */
int orb_kfdb_add(orb_keyframe_db_t* db, int id, const uint32_t* words, const double* values, int n);
/* B frames of a batched transform (layout as above) added as keyframes ids[0 .. B) (host array)
 * in that order, device to device; d_bow_n is read back on `stream`.  The words are trusted to
 * be what the transform wrote.  All of the batch is added or none. */
int orb_kfdb_add_batch_device(orb_keyframe_db_t* db, int B, const int32_t* ids, const uint32_t* d_bow_words,
                              const double* d_bow_values, const int32_t* d_bow_n, int cap, void* stream);
/* KeyFrameDatabase::erase (47-66); an id that is not live is a no-op. */
int orb_kfdb_erase(orb_keyframe_db_t* db, int id);
/* GetBestCovisibilityKeyFrames(10) of keyframe `id`, in its order (n <= 10).  Kept per slot, may
 * be set before the id is live; neighbours that are not live at query time are skipped. */
int orb_kfdb_set_covisible(orb_keyframe_db_t* db, int id, const int32_t* neighbour_ids, int n);
/* DetectRelocalisationCandidates (198-308) for a host BowVector; out_ids in the reference's
 * order.  Every call is a query id of its own (the reference accumulates word counts when a
 * caller reuses a frame id; that is not modelled).  Stateful as the reference: the score of every
 * keyframe with common > minCommon is stored, and a covisible neighbour that shares a word but
 * was not scored contributes the score it kept from an earlier query (or 0.0f).  n = 0 or nothing
 * shared: *n_out = 0.  More candidates than out_cap: ORB_ERANGE with *n_out = the count needed
 * and nothing written (the scores are stored all the same; the repeated call returns the same
 * candidates). */
int orb_kfdb_detect_relocalisation_candidates(orb_keyframe_db_t* db, const uint32_t* words, const double* values,
                                              int n, int32_t* out_ids, int out_cap, int* n_out);
/* DetectLoopCandidates (75-196): connected_ids = GetConnectedKeyFrames() of the query keyframe
 * (any ids; those not live are ignored), min_score as there.  Reads and writes no stored score. */
int orb_kfdb_detect_loop_candidates(orb_keyframe_db_t* db, const uint32_t* words, const double* values, int n,
                                    const int32_t* connected_ids, int n_connected, float min_score, int32_t* out_ids,
                                    int out_cap, int* n_out);
/* Q relocalisation queries in the batched-transform layout, without a host round trip: results
 * and final state are those of Q single calls in the order q = 0 .. Q-1.  d_n_out[q] = the true
 * count; at most out_cap ids are written to d_out_ids + q * out_cap (the caller checks).
 * The query rows are trusted to be what the transform wrote (words strictly ascending and below
 * the vocabulary's word count): nothing on this path validates them, where the host entry points
 * return ORB_EINVAL.  Asynchronous on `stream`. */
int orb_kfdb_detect_relocalisation_candidates_batch_device(orb_keyframe_db_t* db, int Q, const uint32_t* d_bow_words,
                                                           const double* d_bow_values, const int32_t* d_bow_n,
                                                           int cap, int32_t* d_out_ids, int out_cap,
                                                           int32_t* d_n_out, void* stream);

/* ---- Initializer: two-view model scoring (GPU: csrc/orb_initializer.hip) ------------- */
/* Initializer::CheckHomography (reference src/Initializer.cc:303-386) and CheckFundamental
 * (388-466) for all RANSAC hypotheses of a frame pair at once, with the "keep the best" rule of
 * FindHomography / FindFundamental (146-169, 197-220).  The hypotheses are the caller's:
 * ComputeH21 / ComputeF21 (224-301, cv::SVDecomp), Normalize and the T2inv*Hn*T1 / H21i.inv()
 * products stay on the host.  mvMatches12 is built as Initializer.cc:54-63 builds it: the pairs
 * (i, matches12[i]) with matches12[i] >= 0 in ascending i; N = their number, a match's ordinal its
 * position among them.  Every score is the reference's float sum bit for bit (one add chain per
 * hypothesis in match order, first-image term before second-image term); a NaN
 * chi-square is an inlier term and makes the score NaN, an infinite one is an outlier, and a NaN
 * score never wins.  Best hypothesis: score starts at 0.0 and is replaced on a strict >, so the
 * first maximum wins; when no hypothesis scores above 0 the best index is -1, the best score 0
 * and the mask all 0.
 * Limits: at most 8192 keypoints per frame (ORB_ENOTSUP), 1 <= n_hyp <= 1024 (ORB_EINVAL; the
 * reference runs 200, Tracking.cc:374).
 *
 * One pair, host buffers, synchronous.
 *   kps1 (n1), kps2 (n2): the frames' mvKeysUn; matches12: n1 ints, vnMatches12, each in
 *   [-1, n2) (ORB_EINVAL otherwise); sigma: mSigma (1.0, Tracking.cc:374).
 *   H21, H12, F21: n_hyp x 9 row-major floats each (H21i, H12i = H21i.inv(), F21i of iteration
 *   i).  H21 and H12 both NULL skips the homographies, F21 NULL the fundamental matrices; the
 *   outputs of a skipped model are not written.
 *   scores_h / scores_f: n_hyp floats, the currentScore of every iteration (may be NULL).
 *   best_h / best_f: the winning iteration or -1; best_score_*: its score (SH / SF,
 *   Initializer.cc:110); inliers_*: u8 of capacity n1, vbMatchesInliers of the winner, entries
 *   [0, *n_matches) written.  *n_matches = N.  Any output may be NULL. */
int orb_initializer_check(const orb_keypoint_t* kps1, int n1, const orb_keypoint_t* kps2, int n2,
                          const int32_t* matches12, float sigma, int n_hyp, const float* H21, const float* H12,
                          const float* F21, float* scores_h, float* scores_f, int32_t* best_h, float* best_score_h,
                          uint8_t* inliers_h, int32_t* best_f, float* best_score_f, uint8_t* inliers_f,
                          int* n_matches, int device);
/* The same for P pairs on device-resident extractor and matcher output: pair p = frames
 * (d_pair_f1[p], d_pair_f2[p]) of a batch laid out as by orb_extract_batch_device (d_kps /
 * d_counts, per-frame capacity cap; for a distorted camera the undistorted records), its
 * vnMatches12 = row p of d_matches12 (P x cap) as orb_search_for_initialization_batch_device
 * writes it.  Hypotheses d_H21 / d_H12 / d_F21: P x n_hyp x 9 floats.  Outputs per pair:
 * d_scores_* P x n_hyp, d_best_* / d_best_score_* / d_n_matches P, d_inliers_* P x cap (entries
 * [0, d_n_matches[p]) of row p written).  NULL rules as above; a model whose d_scores_* is NULL
 * keeps its scores in stream-ordered scratch for the length of the call.
 * Precondition: row p of d_matches12 holds vnMatches12 of the pair.  An entry outside
 * [0, d_counts[f2]), or at an index >= d_counts[f1], counts as unmatched (the host entry point
 * returns ORB_EINVAL instead); nothing outside the batch arrays is read.  The pair indices are
 * the caller's to keep in range.  P <= 65535.  Asynchronous on `stream`. */
int orb_initializer_check_batch_device(const orb_keypoint_t* d_kps, const int32_t* d_counts, int cap, int P,
                                       const int32_t* d_pair_f1, const int32_t* d_pair_f2,
                                       const int32_t* d_matches12, float sigma, int n_hyp, const float* d_H21,
                                       const float* d_H12, const float* d_F21, float* d_scores_h, float* d_scores_f,
                                       int32_t* d_best_h, float* d_best_score_h, uint8_t* d_inliers_h,
                                       int32_t* d_best_f, float* d_best_score_f, uint8_t* d_inliers_f,
                                       int32_t* d_n_matches, void* stream);

/* The hypotheses on the device: everything of Initializer::Initialize (Initializer.cc:44-221) up to
 * the point where H, F, SH, SF, the two inlier vectors and RH are known: mvMatches12, the minimal
 * sets (80-95), Normalize (747-793) over all keypoints of each frame, ComputeH21 / ComputeF21
 * (224-301) with cv::SVDecomp as OpenCV 2.4's JacobiSVDImpl_<float> is read, T2inv*Hn*T1,
 * H21i.inv() and T2t*Fn*T1, then the two checks above unchanged.  ReconstructH /
 * ReconstructF follow in orb_initializer_reconstruct* and, in the same call, orb_initializer_initialize*
 * below.
 * The draws are the caller's: rand31 holds the n_hyp x 8 values rand() returned, in the order the
 * reference consumes them; draw j of a set is RandomInt(0, N - j - 1) = (r * (N - j)) >> 31 on a
 * list that loses the drawn position (a set never repeats an index); one set serves both models.
 * N is the number of matches.  With N < 8 (the reference would pop from an empty vector) nothing
 * is generated: the hypothesis and set rows are written as zeros, so the best indices are -1, SH =
 * SF = 0, the masks 0, RH = 0/0 and no model is chosen.  Nothing is repaired: a frame with no
 * keypoints or no deviation in a coordinate gives inf / NaN, which flow on.
 * Limits as above: 8192 keypoints per frame, 1 <= n_hyp <= 1024.
 *
 * ComputeH21 / ComputeF21 alone, host buffers, synchronous.  Exactly one of `sets` (n_hyp x 8 match
 * ordinals, each in [0, N)) and `rand31` (each >= 0) is given (ORB_EINVAL otherwise).  Outputs, any
 * may be NULL: H21, H12, F21 (n_hyp x 9, the layout orb_initializer_check reads), Hn, Fn (the
 * normalised solutions), T1, T2 (9 floats each), sets_out (n_hyp x 8), *n_matches = N. */
int orb_initializer_compute_hypotheses(const orb_keypoint_t* kps1, int n1, const orb_keypoint_t* kps2, int n2,
                                       const int32_t* matches12, int n_hyp, const int32_t* sets, const int32_t* rand31,
                                       float* H21, float* H12, float* F21, float* Hn, float* Fn, float* T1, float* T2,
                                       int32_t* sets_out, int* n_matches, int device);
/* The whole of it for one pair, host buffers, synchronous: the outputs of orb_initializer_check for
 * the generated hypotheses, the hypotheses and sets themselves, and per pair best_H21 / best_F21 (9
 * floats: H and F of Initialize, NaN when the best index is -1), *RH = SH / (SH + SF) and *use_h =
 * (RH > 0.40), the model Initialize would reconstruct from (Initializer.cc:113).  A negative draw
 * is ORB_EINVAL.  Any output may be NULL. */
int orb_initializer_ransac(const orb_keypoint_t* kps1, int n1, const orb_keypoint_t* kps2, int n2,
                           const int32_t* matches12, float sigma, int n_hyp, const int32_t* rand31, float* H21,
                           float* H12, float* F21, int32_t* sets_out, float* scores_h, float* scores_f, int32_t* best_h,
                           float* best_score_h, uint8_t* inliers_h, int32_t* best_f, float* best_score_f,
                           uint8_t* inliers_f, float* best_H21, float* best_F21, float* RH, int32_t* use_h,
                           int* n_matches, int device);
/* The same for P pairs on device-resident extractor and matcher output: the arguments, limits and
 * precondition of orb_initializer_check_batch_device with d_rand31 (P x n_hyp x 8 int32; a
 * negative value counts as 0) in place of the hypotheses, and the outputs d_H21 / d_H12 / d_F21 (P
 * x n_hyp x 9), d_sets_out (P x n_hyp x 8), d_best_H21 / d_best_F21 (P x 9), d_RH (P floats),
 * d_use_h (P int32).  Any output may be NULL; what later kernels need of an absent one lives in
 * stream-ordered scratch for the length of the call.  Asynchronous on `stream`. */
int orb_initializer_ransac_batch_device(const orb_keypoint_t* d_kps, const int32_t* d_counts, int cap, int P,
                                        const int32_t* d_pair_f1, const int32_t* d_pair_f2,
                                        const int32_t* d_matches12, float sigma, int n_hyp, const int32_t* d_rand31,
                                        float* d_H21, float* d_H12, float* d_F21, int32_t* d_sets_out,
                                        float* d_scores_h, float* d_scores_f, int32_t* d_best_h, float* d_best_score_h,
                                        uint8_t* d_inliers_h, int32_t* d_best_f, float* d_best_score_f,
                                        uint8_t* d_inliers_f, int32_t* d_n_matches, float* d_best_H21,
                                        float* d_best_F21, float* d_RH, int32_t* d_use_h, void* stream);

/* The reconstruction: what Initialize does with the winning model (Initializer.cc:113-116):
 * ReconstructF (468-568: E21 = K.t()*F21*K, DecomposeE, 4 motion hypotheses) or ReconstructH
 * (570-730: Faugeras, 8 hypotheses, none when d1/d2 or d2/d3 < 1.00001), CheckRT (796-905) with
 * Triangulate (732-745) for every hypothesis over every inlier match, and the acceptance rule of
 * the model in use.  Everything is the statement-for-statement model's bit for bit
 * except parallax_deg, which goes through acosf (§18 records the bound).
 *
 * One pair, host buffers, synchronous.  kps1 / kps2 / matches12 as orb_initializer_check.  M21: the 9
 * floats of H21 (use_h = 1) or F21 (use_h = 0; anything else is ORB_EINVAL).  inliers: the model's
 * vbMatchesInliers over match ordinals as orb_initializer_check writes inliers_*, N entries, each 0
 * or 1 (ORB_EINVAL otherwise).  K4 = fx, fy, cx, cy of the reference camera's K (Tracking.cc:52-63),
 * finite, fx and fy not 0; sigma = mSigma, finite and not 0; min_parallax (1.0) finite;
 * min_triangulated (50) >= 0 (ORB_EINVAL with a message naming the argument).  At most 8192
 * keypoints per frame (ORB_ENOTSUP).
 * Outputs, any may be NULL: *ok (the return value of Reconstruct*); R21 (9) and t21 (3); P3D (n1 x 3)
 * and triangulated (n1 u8), vP3D / vbTriangulated indexed by frame-1 keypoint; all four are zeros
 * when *ok == 0.  Diagnostics, written either way: *n_motion (0, 4 or 8), motion_R (8 x 9) and
 * motion_t (8 x 3) in the order CheckRT sees them (rows >= n_motion zeros), n_good (8),
 * cos_parallax (8: vCosParallax[min(50, size - 1)] after the sort, a NaN sorted after every
 * number; NaN when nGood == 0), parallax_deg (8; 0 when nGood == 0), *best (the chosen hypothesis
 * or -1), *n_inliers (the N of Reconstruct*: the set entries of the mask). */
int orb_initializer_reconstruct(const orb_keypoint_t* kps1, int n1, const orb_keypoint_t* kps2, int n2,
                                const int32_t* matches12, const float* M21, int use_h, const uint8_t* inliers,
                                const float* K4, float sigma, float min_parallax, int min_triangulated, int32_t* ok,
                                float* R21, float* t21, float* P3D, uint8_t* triangulated, int32_t* n_motion,
                                float* motion_R, float* motion_t, int32_t* n_good, float* cos_parallax,
                                float* parallax_deg, int32_t* best, int32_t* n_inliers, int device);
/* The same for P pairs on what orb_initializer_ransac_batch_device wrote (d_best_H21, d_best_F21,
 * d_use_h, d_inliers_h, d_inliers_f: none NULL; d_n_matches may be NULL, when given no ordinal at or
 * above it is walked), next to the batch arrays of that call; K4 is host memory, one camera for
 * the batch.  Pair p uses the model and mask that d_use_h[p] names (non-zero: H); a mask entry
 * other than 0 counts as set; a NaN model (best index -1) ends with ok = 0.  Outputs per pair:
 * d_P3D P x cap x 3, d_triangulated P x cap (all cap rows written), d_R21 P x 9, d_t21 P x 3,
 * d_motion_R P x 72, d_motion_t P x 24, d_n_good / d_cos_parallax / d_parallax_deg P x 8, the rest
 * P; any may be NULL.  Scratch is stream-ordered, about 44 bytes x P x cap, freed with the call.
 * P <= 65535.  Asynchronous on `stream`. */
int orb_initializer_reconstruct_batch_device(const orb_keypoint_t* d_kps, const int32_t* d_counts, int cap, int P,
                                             const int32_t* d_pair_f1, const int32_t* d_pair_f2,
                                             const int32_t* d_matches12, const float* d_best_H21,
                                             const float* d_best_F21, const int32_t* d_use_h,
                                             const uint8_t* d_inliers_h, const uint8_t* d_inliers_f,
                                             const int32_t* d_n_matches, const float* K4, float sigma,
                                             float min_parallax, int min_triangulated, int32_t* d_ok, float* d_R21,
                                             float* d_t21, float* d_P3D, uint8_t* d_triangulated, int32_t* d_n_motion,
                                             float* d_motion_R, float* d_motion_t, int32_t* d_n_good,
                                             float* d_cos_parallax, float* d_parallax_deg, int32_t* d_best,
                                             int32_t* d_n_inliers, void* stream);
/* Initializer::Initialize in one call: orb_initializer_ransac followed by orb_initializer_reconstruct
 * on the model it chose; arguments and outputs are those of the two (any output may be NULL).  The
 * host form passes the winner, its mask and use_h through the host between the two chains. */
int orb_initializer_initialize(const orb_keypoint_t* kps1, int n1, const orb_keypoint_t* kps2, int n2,
                               const int32_t* matches12, float sigma, int n_hyp, const int32_t* rand31, const float* K4,
                               float min_parallax, int min_triangulated, float* H21, float* H12, float* F21,
                               int32_t* sets_out, float* scores_h, float* scores_f, int32_t* best_h,
                               float* best_score_h, uint8_t* inliers_h, int32_t* best_f, float* best_score_f,
                               uint8_t* inliers_f, float* best_H21, float* best_F21, float* RH, int32_t* use_h,
                               int* n_matches, int32_t* ok, float* R21, float* t21, float* P3D, uint8_t* triangulated,
                               int32_t* n_motion, float* motion_R, float* motion_t, int32_t* n_good,
                               float* cos_parallax, float* parallax_deg, int32_t* best, int32_t* n_inliers,
                               int device);
/* The batch form: both chains enqueued on `stream` with no host round trip between them; what the
 * second needs of an absent output of the first lives in stream-ordered scratch. */
int orb_initializer_initialize_batch_device(
    const orb_keypoint_t* d_kps, const int32_t* d_counts, int cap, int P, const int32_t* d_pair_f1,
    const int32_t* d_pair_f2, const int32_t* d_matches12, float sigma, int n_hyp, const int32_t* d_rand31,
    const float* K4, float min_parallax, int min_triangulated, float* d_H21, float* d_H12, float* d_F21,
    int32_t* d_sets_out, float* d_scores_h, float* d_scores_f, int32_t* d_best_h, float* d_best_score_h,
    uint8_t* d_inliers_h, int32_t* d_best_f, float* d_best_score_f, uint8_t* d_inliers_f, int32_t* d_n_matches,
    float* d_best_H21, float* d_best_F21, float* d_RH, int32_t* d_use_h, int32_t* d_ok, float* d_R21, float* d_t21,
    float* d_P3D, uint8_t* d_triangulated, int32_t* d_n_motion, float* d_motion_R, float* d_motion_t,
    int32_t* d_n_good, float* d_cos_parallax, float* d_parallax_deg, int32_t* d_best, int32_t* d_n_inliers,
    void* stream);

/* ---- Solvers: PnP / Sim3 RANSAC consensus (GPU: csrc/orb_solvers.hip) ---------------- */
/* PnPsolver::CheckInliers (reference src/PnPsolver.cc:280-311) and Sim3Solver::CheckInliers
 * (src/Sim3Solver.cc:335-359) for all RANSAC hypotheses of a solver at once, with the
 * per-correspondence set-up of the two constructors and the keep-the-best rule of the two
 * iterate() loops.  In these four entry points the hypotheses are the caller's; the minimal sets
 * and the hypotheses themselves (PnP: EPnP's compute_pose and Refine; Sim3: computeT) run on the
 * device in the orb_pnp_ransac / orb_sim3_ransac entry points below.  The iteration counters and the
 * random generator stay with the caller.  Counts and masks are the reference's bit for bit: a NaN
 * error is an outlier, a point behind the camera is not excluded.
 * Correspondence i of hypothesis h is bit i % 64 of word i / 64 of the h-th mask row (W words per
 * row); bits past n are zero.
 * Keep-the-best, over the hypotheses in order, starting from best_in (mnBestInliers of earlier
 * iterate() calls, 0 at first): best_at[h] = the hypothesis holding mvbBestInliers after iteration
 * h, -1 for none, -2 for "still the earlier calls' best" (best_in > 0 and not yet replaced).
 *   PnP  (PnPsolver.cc:181-196): h qualifies when counts[h] >= min_inliers; among those the best
 *        is replaced on a strict >, so the first maximum wins.  first_ok = the first qualifying h
 *        (where the reference goes on to Refine), or -1.  Refine's pose is scored by a call with
 *        one hypothesis.
 *   Sim3 (Sim3Solver.cc:183-200): the best is replaced on counts[h] >= best, so the last maximum
 *        wins.  first_accept = the first h that replaces the best with counts[h] > min_inliers
 *        (where the reference returns), or -1.
 * min_inliers is the adjusted mRansacMinInliers (SetRansacParameters; the wrappers compute it).
 * Limits: n, cap <= 8192 (ORB_ENOTSUP), 1 <= n_hyp <= 1024 (ORB_EINVAL), every sigma2 finite and
 * >= 0 and, for Sim3, 9.21 * sigma2 < 2^63 (ORB_EINVAL).
 *
 * One PnPsolver, host buffers, synchronous.  The n correspondences as the constructor compacts
 * them: p3d n x 3 (mvP3Dw), p2d n x 2 (mvP2D), sigma2 n (mvSigma2); mvMaxError = sigma2 * th2.
 * fu, fv, uc, vc: the calibration as the solver's doubles.  R n_hyp x 9, t n_hyp x 3 doubles (mRi,
 * mti of iteration h).  Outputs, each may be NULL: counts n_hyp (mnInliersi), masks n_hyp x W
 * with W = (n + 63) / 64 (mvbInliersi), best_at n_hyp, *first_ok. */
int orb_pnp_check_inliers(int n, const float* p3d, const float* p2d, const float* sigma2, float th2, double fu,
                          double fv, double uc, double vc, int n_hyp, const double* R, const double* t,
                          int min_inliers, int best_in, int32_t* counts, uint64_t* masks, int32_t* best_at,
                          int32_t* first_ok, int device);
/* One Sim3Solver, host buffers, synchronous.  x3dc1 / x3dc2 n x 3 (mvX3Dc1 / mvX3Dc2), sigma2_1 /
 * sigma2_2 n (GetSigma2 of the two keypoints' octaves): mvP1im1 / mvP2im2 (FromCameraToImage) and
 * the bounds mvnMaxError1/2 = (size_t)(9.210 * sigma2) are computed here.  K1 / K2: fx, fy, cx,
 * cy.  T12 / T21: n_hyp x 12 floats, rows 0-2 of mT12i / mT21i (row-major 3 x 4).  Outputs as
 * above with *first_accept. */
int orb_sim3_check_inliers(int n, const float* x3dc1, const float* x3dc2, const float* sigma2_1,
                           const float* sigma2_2, const float* K1, const float* K2, int n_hyp, const float* T12,
                           const float* T21, int min_inliers, int best_in, int32_t* counts, uint64_t* masks,
                           int32_t* best_at, int32_t* first_accept, int device);
/* S PnPsolvers on device-resident data: solver s = (keyframe d_pair_a[s], frame d_pair_b[s]) of
 * a batch laid out as by orb_extract_batch_device (d_kps / d_counts, per-frame capacity cap; the
 * undistorted records), row s of d_match (S x cap) as orb_search_by_bow_batch_device with
 * kf_kf = 0 writes it (d_match[s][j] = the keyframe keypoint matched to frame keypoint j).
 * d_mp_pos B x cap x 3: the world position of the MapPoint of each keypoint of the batch;
 * d_mp_bad B x cap u8 (may be NULL): its isBad().  level_sigma2: nlevels (1..16) host floats.
 * Correspondences, as PnPsolver.cc:51-73 builds them: the frame keypoints j in ascending order
 * whose match is a keyframe keypoint with a MapPoint that is not bad.  Hypotheses d_R S x n_hyp x
 * 9, d_t S x n_hyp x 3 doubles; d_best_in S (NULL = all 0).  Outputs per solver, each may be NULL:
 * d_n S (N), d_index S x cap (mvKeyPointIndices, -1 past N), d_counts_out S x n_hyp, d_masks S x
 * n_hyp x W with W = (cap + 63) / 64 (written whole), d_best_at S x n_hyp, d_first_ok S.
 * A match entry outside [0, d_counts[keyframe]), or at an index >= d_counts[frame], is no match;
 * an octave outside [0, nlevels) is clamped; nothing outside the batch arrays is read.  The pair
 * indices are the caller's to keep in range.  S <= 65535.  Asynchronous on `stream`. */
int orb_pnp_check_inliers_batch_device(const orb_keypoint_t* d_kps, const int32_t* d_counts, int cap, int S,
                                       const int32_t* d_pair_a, const int32_t* d_pair_b, const int32_t* d_match,
                                       const float* d_mp_pos, const uint8_t* d_mp_bad, const float* level_sigma2,
                                       int nlevels, float th2, double fu, double fv, double uc, double vc, int n_hyp,
                                       const double* d_R, const double* d_t, int min_inliers,
                                       const int32_t* d_best_in, int32_t* d_n, int32_t* d_index,
                                       int32_t* d_counts_out, uint64_t* d_masks, int32_t* d_best_at,
                                       int32_t* d_first_ok, void* stream);
/* S Sim3Solvers likewise: solver s = keyframes (d_pair_a[s], d_pair_b[s]), row s of d_match as
 * orb_search_by_bow_batch_device with kf_kf = 1 writes it (d_match[s][i1] = idx2).  d_mp_pos /
 * d_mp_bad apply to both keyframes; d_pose B x 12 floats, Rcw (row-major 3 x 3) then tcw, gives
 * mvX3Dc1/2 = Rcw * Pos + tcw.  K: fx, fy, cx, cy, one calibration for the call.  d_T12 / d_T21
 * S x n_hyp x 12 floats.  d_index = mvnIndices1.
 * Precondition: the pair (i1, idx2) stands for GetIndexInKeyFrame of the two MapPoints, i.e. each
 * MapPoint is observed in its keyframe at the keypoint the match row names (what SearchByBoW
 * matched), and a keypoint without a MapPoint is flagged in d_mp_bad. */
int orb_sim3_check_inliers_batch_device(const orb_keypoint_t* d_kps, const int32_t* d_counts, int cap, int S,
                                        const int32_t* d_pair_a, const int32_t* d_pair_b, const int32_t* d_match,
                                        const float* d_mp_pos, const uint8_t* d_mp_bad, const float* d_pose,
                                        const float* level_sigma2, int nlevels, const float* K, int n_hyp,
                                        const float* d_T12, const float* d_T21, int min_inliers,
                                        const int32_t* d_best_in, int32_t* d_n, int32_t* d_index,
                                        int32_t* d_counts_out, uint64_t* d_masks, int32_t* d_best_at,
                                        int32_t* d_first_accept, void* stream);

/* ---- Sim3Solver: the hypotheses and the whole RANSAC (GPU: csrc/orb_solvers.hip) */
/* The minimal sets of Sim3Solver::iterate (Sim3Solver.cc:163-177) and Horn's closed form
 * (Sim3Solver::computeT, 226-332, with centroid, 215-224), one lane per hypothesis, restated in the
 * reference's float pattern with OpenCV 2.4's primitives as DESIGN.md §15 reads them (cv::eigen is
 * JacobiImpl_<float>).  Nothing is repaired: a set whose best quaternion is exactly (+-1, 0, 0, 0)
 * gives a NaN hypothesis, which scores 0 inliers; a set may hold one correspondence twice.
 * Draws: either `sets`, n_hyp x 3 indices into the n correspondences, or `rand31`, n_hyp x 3 values
 * as rand() returned them, 0 <= r < 2^31; draw i of a set is RandomInt(0, size - 1) = (r * size) >>
 * 31 on the list of size n - i, and the drawn value, not the position, is overwritten with the
 * list's last entry, as the reference does.  The package owns no random generator.
 * A Sim3 is 13 floats: mR12i row-major, mt12i, ms12i (the layout of orb_optimize_sim3's sim3_in).
 *
 * computeT alone, host buffers, synchronous.  x3dc1 / x3dc2 n x 3.  Outputs, each may be NULL: T12 /
 * T21 n_hyp x 12 (rows 0-2 of mT12i / mT21i), sim3 n_hyp x 13, quat n_hyp x 4 (row 0 of cv::eigen's
 * eigenvectors), sets_out n_hyp x 3.  ORB_EINVAL: both or neither of sets / rand31, a set index
 * outside [0, n), a rand31 value outside [0, 2^31), n < 1, or n < 3 with rand31. */
int orb_sim3_compute_hypotheses(int n, const float* x3dc1, const float* x3dc2, int n_hyp, const int32_t* sets,
                                const int32_t* rand31, float* T12, float* T21, float* sim3, float* quat,
                                int32_t* sets_out, int device);
/* One Sim3Solver::iterate(n_hyp, ...) without its early return, host buffers, synchronous: the
 * arguments and outputs of orb_sim3_check_inliers with the draws in place of T12 / T21, which are
 * generated, scored and selected in one stream-ordered chain.  Further outputs, each may be NULL: T12,
 * T21, sim3, sets_out as above and accepted (13 floats): the Sim3 of hypothesis first_accept, or of
 * best_at[n_hyp - 1] when nothing was accepted (mBestRotation / mBestTranslation / mBestScale either
 * way); NaN when the best is still the earlier calls' (best_at[n_hyp - 1] < 0).  n < min_inliers is
 * bNoMore (Sim3Solver.cc:146-150): nothing is generated, the hypothesis and set rows are zeros, the
 * counts 0, first_accept -1.  ORB_EINVAL as above and for min_inliers < 3. */
int orb_sim3_ransac(int n, const float* x3dc1, const float* x3dc2, const float* sigma2_1, const float* sigma2_2,
                    const float* K1, const float* K2, int n_hyp, const int32_t* sets, const int32_t* rand31,
                    int min_inliers, int best_in, int32_t* counts, uint64_t* masks, int32_t* best_at,
                    int32_t* first_accept, float* T12, float* T21, float* sim3, int32_t* sets_out, float* accepted,
                    int device);
/* S Sim3Solvers on device-resident data: the arguments of orb_sim3_check_inliers_batch_device with
 * d_rand31 (S x n_hyp x 3 int32) in place of d_T12 / d_T21; the draws are mapped to sets on the
 * device, where each solver's n is.  A negative d_rand31 value is clamped to 0 (the host forms refuse
 * it).  Further outputs, each may be NULL: d_T12 / d_T21 S x n_hyp x 12, d_sim3 S x n_hyp x 13,
 * d_sets_out S x n_hyp x 3, d_accepted S x 13 (as `accepted` above; the layout
 * orb_optimize_sim3_batch_device takes as d_sim3_in) and d_accepted_mask S x W, the accepted
 * hypothesis's mask row: what iterate returns in vbInliers before the scatter through mvnIndices1
 * (zeros where d_accepted is NaN).  Asynchronous on `stream`; scratch is stream-ordered. */
int orb_sim3_ransac_batch_device(const orb_keypoint_t* d_kps, const int32_t* d_counts, int cap, int S,
                                 const int32_t* d_pair_a, const int32_t* d_pair_b, const int32_t* d_match,
                                 const float* d_mp_pos, const uint8_t* d_mp_bad, const float* d_pose,
                                 const float* level_sigma2, int nlevels, const float* K, int n_hyp,
                                 const int32_t* d_rand31, int min_inliers, const int32_t* d_best_in, int32_t* d_n,
                                 int32_t* d_index, int32_t* d_counts_out, uint64_t* d_masks, int32_t* d_best_at,
                                 int32_t* d_first_accept, float* d_T12, float* d_T21, float* d_sim3,
                                 int32_t* d_sets_out, float* d_accepted, uint64_t* d_accepted_mask, void* stream);

/* ---- PnPsolver: the hypotheses and the whole RANSAC (GPU: csrc/orb_solvers.hip) */
/* The minimal sets of PnPsolver::iterate (PnPsolver.cc:160-173), EPnP's compute_pose (449-497 with its
 * helpers, 347-922) and Refine (232-277), restated in double with the reference build's fused
 * operations and OpenCV 2.4's cvMulTransposed / cvSVD / cvInvert / cvSolve as DESIGN.md §17 reads them.
 * Nothing is repaired: coplanar or repeated points, a singular matrix, a zero beta and NaN flow on
 * (every loop is bounded; a NaN pose scores 0 inliers).  The one exception: gauss_newton's x starts
 * as zeros, where the reference reads it uninitialised when qr_solve returns early on its first call.
 * Draws: either `sets`, n_hyp x 4 indices into the n correspondences, or `rand31`, n_hyp x 4 values
 * as rand() returned them, mapped as for Sim3 above (the drawn value, not the position, is
 * overwritten, so a set may hold a correspondence twice).  The package owns no random generator.
 *
 * compute_pose on minimal sets alone, host buffers, synchronous.  p3d n x 3, p2d n x 2; fu, fv, uc, vc
 * the calibration.  Outputs, each may be NULL: R n_hyp x 9 and t n_hyp x 3 doubles (mRi, mti),
 * rep_error n_hyp doubles (compute_pose's return value), sets_out n_hyp x 4.  ORB_EINVAL: both or
 * neither of sets / rand31, a set index outside [0, n), a rand31 value outside [0, 2^31), n < 1, or
 * n < 4 with rand31. */
int orb_pnp_compute_hypotheses(int n, const float* p3d, const float* p2d, double fu, double fv, double uc, double vc,
                               int n_hyp, const int32_t* sets, const int32_t* rand31, double* R, double* t,
                               double* rep_error, int32_t* sets_out, int device);
/* compute_pose on the n_sel correspondences sel[0 .. n_sel) in that order (what Refine computes on
 * the set bits of a mask): R 9, t 3 doubles, *rep_error; each may be NULL.  1 <= n_sel <= 8192, every
 * sel[k] in [0, n) (ORB_EINVAL). */
int orb_pnp_compute_pose_n(int n, const float* p3d, const float* p2d, double fu, double fv, double uc, double vc,
                           int n_sel, const int32_t* sel, double* R, double* t, double* rep_error, int device);
/* One PnPsolver::iterate over n_hyp iterations, host buffers, synchronous: the arguments and outputs
 * of orb_pnp_check_inliers with the draws in place of R / t, which are generated, scored and selected
 * in one stream-ordered chain; then Refine at the iterations that replaced the best (best_at[h] == h:
 * the only ones with a mask not yet refined), its pose scored over all n, and the result of the call.
 * iterate's loop runs while mnIterations < mRansacMaxIts OR nCurrentIterations < nIterations
 * (PnPsolver.cc:154): n_hyp is the caller's max(mRansacMaxIts - mnIterations, nIterations).
 * Further outputs, each may be NULL: R, t, sets_out as above; refined_counts n_hyp (mnRefinedInliers at
 * the replacing iterations, -1 elsewhere); *first_refined = the first replacing iteration whose
 * refined count is > min_inliers (where iterate returns, having consumed first_refined + 1 sets of
 * draws), or -1; pose 12 floats (Rcw row-major then tcw, double narrowed to float: the input pose of
 * orb_pose_optimization_batch_device), pose_mask W words and *pose_inliers: mRefinedTcw,
 * mvbRefinedInliers, mnRefinedInliers of iteration first_refined, else mBestTcw, mvbBestInliers,
 * mnBestInliers of best_at[n_hyp - 1] when there is a best, else NaN, zeros and 0.  When the best is
 * still the earlier calls' (best_at[n_hyp - 1] == -2) the pose is NaN, the mask zeros and
 * *pose_inliers = best_in.  n < min_inliers is bNoMore (PnPsolver.cc:145-149): nothing is generated,
 * the hypothesis and set rows are zeros, the counts 0, the indices -1.  ORB_EINVAL as above and for
 * min_inliers < 4 (SetRansacParameters never yields it). */
int orb_pnp_ransac(int n, const float* p3d, const float* p2d, const float* sigma2, float th2, double fu, double fv,
                   double uc, double vc, int n_hyp, const int32_t* sets, const int32_t* rand31, int min_inliers,
                   int best_in, int32_t* counts, uint64_t* masks, int32_t* best_at, int32_t* first_ok, double* R,
                   double* t, int32_t* sets_out, int32_t* refined_counts, int32_t* first_refined, float* pose,
                   uint64_t* pose_mask, int32_t* pose_inliers, int device);
/* S PnPsolvers on device-resident data: the arguments of orb_pnp_check_inliers_batch_device with
 * d_rand31 (S x n_hyp x 4 int32) in place of d_R / d_t; the draws are mapped to sets on the device,
 * where each solver's n is.  A negative d_rand31 value is clamped to 0 (the host forms refuse it).
 * Further outputs, each may be NULL: d_R S x n_hyp x 9, d_t S x n_hyp x 3 doubles, d_sets_out S x
 * n_hyp x 4, d_refined_counts S x n_hyp, d_first_refined S, d_pose S x 12 floats, d_pose_mask S x W
 * (before the scatter through d_index), d_pose_inliers S, as above.  Asynchronous on `stream`;
 * scratch is stream-ordered. */
int orb_pnp_ransac_batch_device(const orb_keypoint_t* d_kps, const int32_t* d_counts, int cap, int S,
                                const int32_t* d_pair_a, const int32_t* d_pair_b, const int32_t* d_match,
                                const float* d_mp_pos, const uint8_t* d_mp_bad, const float* level_sigma2, int nlevels,
                                float th2, double fu, double fv, double uc, double vc, int n_hyp,
                                const int32_t* d_rand31, int min_inliers, const int32_t* d_best_in, int32_t* d_n,
                                int32_t* d_index, int32_t* d_counts_out, uint64_t* d_masks, int32_t* d_best_at,
                                int32_t* d_first_ok, double* d_R, double* d_t, int32_t* d_sets_out,
                                int32_t* d_refined_counts, int32_t* d_first_refined, float* d_pose,
                                uint64_t* d_pose_mask, int32_t* d_pose_inliers, void* stream);

/* ---- Optimizer: motion-only pose optimisation (GPU: csrc/orb_optimizer.hip) ----------- */
/* Optimizer::PoseOptimization(Frame*) (reference src/Optimizer.cc:154-285) with the parts of g2o
 * it runs, in double: one SE3 vertex (quaternion + translation), one EdgeSE3ProjectXYZ per
 * keypoint that has a MapPoint (fixed point, information invSigma2 * I, Huber kernel of delta
 * (float)sqrt(5.991)), four rounds of Levenberg ({10, 10, 7, 5} iterations, up to 10 trials each)
 * over the edges not flagged, each followed by the classification against chi2 = {9.210f, 7.378f,
 * 5.991f, 5.991f}.  The whole schedule runs in one launch, one workgroup per problem; DESIGN.md
 * §13 lists the semantics kept (the quirks included) and what a sum order may change.  Poses are
 * 12 values: Rcw row-major, then tcw.  pose_in goes through Converter::toSE3Quat (quaternion of R,
 * normalised), so pose_out of a problem without edges is pose_in after that round trip.
 * pose_out = (float)pose_out_f64.  outlier = mvbOutlier (0 where there is no MapPoint);
 * *n_inliers = nInitialCorrespondences - nBad of the last round run (an edge whose chi2 is NaN
 * keeps its flag and is not counted in nBad, as in the reference).
 * Limits: n, cap <= 8192, S <= 65535 (ORB_ENOTSUP); a non-finite pose or calibration value,
 * fx == 0 or fy == 0: ORB_EINVAL (the host entry point checks pose_in, both check K). */
typedef struct {
    int32_t n_initial;     /* nInitialCorrespondences: the edges                            */
    int32_t n_bad;         /* nBad of the last round run                                    */
    int32_t rounds;        /* rounds run: 4, or 1 when there are fewer than 10 edges        */
    int32_t iterations[4]; /* diagnostics: Levenberg iterations run per round ...           */
    int32_t trials;        /* ... trial steps in all ...                                    */
    double lambda;         /* ... the last lambda (-1: no round had an edge) ...            */
    double chi2;           /* ... and the robust chi2 the last iteration ended with         */
} orb_pose_opt_info_t;
/* One frame, host buffers, synchronous.  Keypoint i: p3d n x 3 (GetWorldPos), obs n x 2
 * (mvKeysUn[i].pt), inv_sigma2 n (mvInvLevelSigma2[octave]); has_mp n u8 (NULL: every keypoint has
 * a MapPoint).  pose_out_f64 and info may be NULL. */
int orb_pose_optimization(int n, const float* p3d, const float* obs, const float* inv_sigma2, const uint8_t* has_mp,
                          float fx, float fy, float cx, float cy, const float* pose_in, float* pose_out,
                          double* pose_out_f64, uint8_t* outlier, int32_t* n_inliers, orb_pose_opt_info_t* info,
                          int device);
/* S problems on device-resident data: problem s reads the undistorted records of frame
 * d_frame_of[s] of a batch laid out as by orb_extract_batch_device (d_kps / d_counts, capacity
 * cap) and its own row of d_mp_pos (S x cap x 3, the MapPoint of keypoint i) and d_has_mp (S x cap
 * u8), so one frame may serve several problems (relocalisation candidates).  inv_level_sigma2:
 * n_levels (1..16) host floats, mvInvLevelSigma2; K4: fx, fy, cx, cy host floats.  d_pose_in S x
 * 12.  Outputs: d_pose_out S x 12 f32, d_pose_out_f64 S x 12 (may be NULL), d_outlier S x cap
 * (written whole: 0 past the frame's count), d_n_inliers S, d_info S (may be NULL).
 * An index at or past the frame's count is no edge; an octave outside [0, n_levels) is clamped;
 * nothing outside the batch arrays is read.  The frame indices are the caller's to keep in range.
 * Asynchronous on `stream`; scratch is stream-ordered. */
int orb_pose_optimization_batch_device(const orb_keypoint_t* d_kps, const int32_t* d_counts, int cap, int S,
                                       const int32_t* d_frame_of, const float* d_mp_pos, const uint8_t* d_has_mp,
                                       const float* inv_level_sigma2, int n_levels, const float* K4,
                                       const float* d_pose_in, float* d_pose_out, double* d_pose_out_f64,
                                       uint8_t* d_outlier, int32_t* d_n_inliers, orb_pose_opt_info_t* d_info,
                                       void* stream);

/* ---- Optimizer: Sim3 optimisation of a loop candidate (GPU: csrc/orb_sim3opt.hip) ------ */
/* Optimizer::OptimizeSim3 (reference src/Optimizer.cc:1721-1917; LoopClosing.cc:340) with the parts
 * of g2o it runs, in double: one Sim3 vertex (quaternion, never normalised, translation, scale) and
 * per usable slot two edges over fixed camera-frame points, e12 = obs1 - cam1(project(S.map(X2)))
 * with information invSigma2(octave1) * I and e21 = obs2 - cam2(project(S^-1.map(X1))) with
 * information sigma2(octave2) * I (GetSigma2, Optimizer.cc:1842: the reference's behaviour, kept),
 * both with a Huber kernel of delta (float)sqrt(th2); the Jacobian is g2o's numeric one (central
 * differences at 1e-9 through oplus).  optimize(5); every pair with chi2(e12) > th2 || chi2(e21) >
 * th2 is removed and its slot cleared (n_bad); fewer than 10 pairs left: the result is 0 and the
 * Sim3 outputs are the input's (after the quaternion conversion), the cleared slots stay cleared;
 * else optimize(n_bad > 0 ? 10 : 5) and a second classification that clears slots and counts the
 * inliers.  The whole schedule runs in one launch, one workgroup per problem; DESIGN.md §14 lists
 * the semantics kept and what a sum order may change.  A Sim3 is 13 floats in and out (R row-major,
 * t, s; out = (float) of toRotationMatrix, t, s) and 8 doubles out (qx qy qz qw, t, s).  A pair whose
 * chi2 is NaN on both edges is not > th2: it stays and counts as an inlier, as in the reference.
 * Limits: n, cap <= 8192, S <= 65535 (ORB_ENOTSUP); a non-finite calibration value, fx == 0 or
 * fy == 0, th2 not finite or < 0, and in the host form a non-finite sim3_in: ORB_EINVAL. */
typedef struct {
    int32_t n_correspondences; /* nCorrespondences: the usable slots                           */
    int32_t n_bad;             /* nBad: the pairs removed by the first classification          */
    int32_t more_iterations;   /* nMoreIterations: 5 or 10; 0 when the routine returned early  */
    int32_t iterations[2];     /* diagnostics: Levenberg iterations run per optimize() ...     */
    int32_t trials;            /* ... trial steps in all ...                                   */
    double lambda;             /* ... the last lambda (-1: nothing ran) ...                    */
    double chi2;               /* ... and the robust chi2 the last iteration ended with        */
} orb_sim3_opt_info_t;
/* One candidate, host buffers, synchronous.  Slot i (i = keypoint of KF1): x3dc1 / x3dc2 n x 3 (P3D1c
 * / P3D2c: the two MapPoints in their own keyframe's camera frame), obs1 n x 2 (kpUn1.pt), obs2 n x
 * 2 (kpUn2.pt of keypoint i2 = GetIndexInKeyFrame(pKF2)), inv_sigma2_1 n (GetInvSigma2(octave1)),
 * sigma2_2 n (GetSigma2(octave2)); usable n u8 (NULL: all): vpMatches1[i] set, both MapPoints
 * there and not bad, i2 >= 0.  K1 / K2: fx, fy, cx, cy.  Outputs: kept n u8 (the slot is still
 * matched afterwards; 0 where not usable); sim3_out_f64 (8), sim3_out (13), n_inliers and info may
 * be NULL. */
int orb_optimize_sim3(int n, const float* x3dc1, const float* x3dc2, const float* obs1, const float* obs2,
                      const float* inv_sigma2_1, const float* sigma2_2, const uint8_t* usable, const float* K1,
                      const float* K2, float th2, const float* sim3_in, uint8_t* kept, double* sim3_out_f64,
                      float* sim3_out, int32_t* n_inliers, orb_sim3_opt_info_t* info, int device);
/* S candidates on device-resident data, laid out as for orb_sim3_check_inliers_batch_device:
 * problem s = keyframes (d_pair_a[s], d_pair_b[s]) of a batch (d_kps / d_counts, capacity cap; the
 * undistorted records), row s of d_match (S x cap, d_match[s][i1] = idx2) as
 * orb_search_by_bow_batch_device with kf_kf = 1 or SearchBySim3 leaves it.  d_mp_pos B x cap x 3
 * and d_mp_bad B x cap u8 (may be NULL) apply to both keyframes; d_pose B x 12 floats (Rcw row-major,
 * tcw) gives P3D1c / P3D2c = Rcw * Pos + tcw as float row sums.  level_sigma2 / inv_level_sigma2:
 * nlevels (1..16) host floats (mvLevelSigma2, mvInvLevelSigma2); K: fx, fy, cx, cy, one calibration
 * for the call.  d_sim3_in S x 13.  Outputs, each may be NULL: d_match_out S x cap (the row as it
 * came, the cleared slots at -1; may be d_match itself), d_sim3_out S x 13, d_sim3_out_f64 S x 8,
 * d_n_inliers S, d_info S.
 * Precondition, as there: the pair (i1, idx2) stands for GetIndexInKeyFrame of the two MapPoints,
 * and a keypoint without a MapPoint is flagged in d_mp_bad.  A match entry outside [0,
 * d_counts[b]), or at an index >= d_counts[a], is no correspondence (it is copied to d_match_out as
 * it is); an octave outside [0, nlevels) is clamped; nothing outside the batch arrays is read.  The
 * pair indices are the caller's to keep in range.  Asynchronous on `stream`; scratch is
 * stream-ordered. */
int orb_optimize_sim3_batch_device(const orb_keypoint_t* d_kps, const int32_t* d_counts, int cap, int S,
                                   const int32_t* d_pair_a, const int32_t* d_pair_b, const int32_t* d_match,
                                   const float* d_mp_pos, const uint8_t* d_mp_bad, const float* d_pose,
                                   const float* level_sigma2, const float* inv_level_sigma2, int nlevels,
                                   const float* K, float th2, const float* d_sim3_in, int32_t* d_match_out,
                                   float* d_sim3_out, double* d_sim3_out_f64, int32_t* d_n_inliers,
                                   orb_sim3_opt_info_t* d_info, void* stream);

/* Optimizer::LocalBundleAdjustment (Optimizer.cc:287-536, csrc/orb_localba.hip): the
 * graph of lines 356-447 as flat arrays, both optimize() calls and both classifications in one
 * launch, one workgroup per problem.  The map stays with the caller.
 *   keyframes  n_kf, local ones first, then fixed: kf_pose n_kf x 12 floats (Rcw row-major, tcw), kf_K
 *              n_kf x 4 (fx fy cx cy), kf_fixed n_kf u8 (mnId == 0, or a camera of lFixedCameras)
 *   points     n_pt: pt_pos n_pt x 3 (GetWorldPos), pt_nobs n_pt (mObservations.size() at entry,
 *              observations in bad keyframes included)
 *   edges      n_edge in the order lines 399-447 create them, the edges of a point contiguous and the
 *              points ascending: edge_pt, edge_kf (indices), edge_obs n_edge x 2 (kpUn.pt),
 *              edge_inv_sigma2 n_edge (GetInvSigma2(octave))
 * Outputs, each may be NULL: kf_pose_out n_kf x 12 (to_homogeneous_matrix narrowed; a fixed
 * keyframe's is its input after the quaternion round trip) and kf_pose_out_f64; pt_pos_out n_pt x 3
 * and pt_pos_out_f64; edge_erased n_edge u8 (0 kept, 1 / 2 the round after which the edge was erased:
 * walk them in edge order with EraseMapPointMatch + EraseObservation to reproduce the reference's map
 * mutation); pt_bad n_pt u8 (0, or the round after which the point's count reached 2); info.
 * ORB_EINVAL: an index out of range, edges not grouped by ascending point, a (point, keyframe) pair
 * twice, more edges of a point than pt_nobs, a non-finite pose or calibration value, fx or fy == 0.
 * ORB_ENOTSUP, with nothing written: no free keyframe, or more than ORB_LBA_MAX_FREE_KF of them.
 * n_edge == 0 or n_pt == 0: ORB_OK, the inputs after the round trip.  The reference's pbStopFlag is
 * not served: a call runs its schedule to the end. */
#define ORB_LBA_MAX_FREE_KF 64
typedef struct {
    int32_t iterations;       /* Levenberg iterations run by this optimize()                      */
    int32_t trials;           /* trial steps in all                                               */
    int32_t active_edges;     /* edges, points and free keyframes in this round's optimisation    */
    int32_t active_points;
    int32_t active_keyframes;
    int32_t refused;          /* trials whose reduced system was not positive definite            */
    double lambda;            /* lambda at the end (-1: nothing ran)                              */
    double chi2_before;       /* the robust chi2 the round started from ...                       */
    double chi2_after;        /* ... and ended with                                               */
} orb_local_ba_round_t;
typedef struct {
    int32_t status;           /* ORB_OK, or why the problem was refused (the batch form's report) */
    int32_t n_free_kf;
    orb_local_ba_round_t round[2];
} orb_local_ba_info_t;
/* One problem on host buffers, synchronous. */
int orb_local_bundle_adjustment(int n_kf, const float* kf_pose, const float* kf_K, const uint8_t* kf_fixed, int n_pt,
                                const float* pt_pos, const int32_t* pt_nobs, int n_edge, const int32_t* edge_pt,
                                const int32_t* edge_kf, const float* edge_obs, const float* edge_inv_sigma2,
                                float* kf_pose_out, double* kf_pose_out_f64, float* pt_pos_out, double* pt_pos_out_f64,
                                uint8_t* edge_erased, uint8_t* pt_bad, orb_local_ba_info_t* info, int device);
/* S problems on device arrays: problem s owns the keyframes [d_kf_off[s], d_kf_off[s + 1]) of the
 * concatenated keyframe arrays (n_kf_total rows), likewise its points and edges (S + 1 offsets each);
 * edge_pt / edge_kf are problem-local.  The outputs have the same concatenated layout; pose rows as
 * orb_pose_optimization_batch_device takes them and positions as orb_update_normal_and_depth does.
 * A problem that the host form would refuse is left unwritten and reports its status in d_info[s]
 * (the call itself returns ORB_OK); offsets that leave the arrays count as ORB_EINVAL and nothing of
 * that problem is read.  Asynchronous on `stream`; scratch is stream-ordered. */
int orb_local_bundle_adjustment_batch_device(int S, const int32_t* d_kf_off, const int32_t* d_pt_off,
                                             const int32_t* d_edge_off, int n_kf_total, int n_pt_total, int n_edge_total,
                                             const float* d_kf_pose, const float* d_kf_K, const uint8_t* d_kf_fixed,
                                             const float* d_pt_pos, const int32_t* d_pt_nobs, const int32_t* d_edge_pt,
                                             const int32_t* d_edge_kf, const float* d_edge_obs,
                                             const float* d_edge_inv_sigma2, float* d_kf_pose_out,
                                             double* d_kf_pose_out_f64, float* d_pt_pos_out, double* d_pt_pos_out_f64,
                                             uint8_t* d_edge_erased, uint8_t* d_pt_bad, orb_local_ba_info_t* d_info,
                                             void* stream);

/* Optimizer::OptimizeEssentialGraph (Optimizer.cc:1470-1719, csrc/orb_essgraph.hip): the
 * pose graph of lines 1498-1659 as flat arrays, optimize(n_iterations), the SE3 recovery and the point
 * correction.  The map stays with the caller, who also does the topological filtering of the edges.
 *   keyframes  n_kf (<= ORB_EG_MAX_KF) in the caller's order, bad ones left out: kf_pose n_kf x 12
 *              floats (Rcw row-major, tcw), entering as Sim3(R, t, 1.0); kf_corrected n_kf x 8 doubles
 *              (q x y z w, t, s: CorrectedSim3[pKF], taken bit for bit) where kf_has_corrected[i];
 *              kf_noncorrected / kf_has_noncorrected likewise (NonCorrectedSim3); either pair may be
 *              NULL (no entry); kf_fixed n_kf u8 (pLoopKF; any number)
 *   edges      n_edge in the order the reference adds them: edge_i (vertex 0), edge_j (vertex 1),
 *              edge_kind u8: 0 a loop connection of lines 1539-1567 (Sji = vScw[j] * vScw[i]^-1), 1 an
 *              edge of lines 1570-1659 (each factor from the non-corrected table where that keyframe
 *              has an entry).  A pair may come more than once, in either direction.
 *   points     n_pt: pt_pos n_pt x 3, pt_ref n_pt (the keyframe index of nIDr, -1: a keyframe without
 *              a vertex, the point comes back as it is), pt_skip n_pt u8 (NULL: none; a skipped
 *              point's output is not written)
 * Outputs, each may be NULL: kf_sim3_out n_kf x 8 doubles; kf_pose_out n_kf x 12 ([R | t (1 / s)]
 * narrowed) and kf_pose_out_f64; pt_pos_out n_pt x 3 and pt_pos_out_f64; info.
 * ORB_EINVAL: no fixed vertex among those an edge touches, a self-edge, an index out of range, a kind
 * other than 0 or 1, a non-finite pose or Sim3 value, a scale <= 0.  ORB_ENOTSUP, nothing written and
 * no scratch of that size requested: more than ORB_EG_MAX_KF keyframes, or a factor profile above
 * ORB_EG_MAX_PROFILE_BYTES.  n_edge == 0 or no free vertex with an edge: ORB_OK, the inputs after the
 * round trip, the points corrected through it.  One graph per call, host buffers, synchronous; the
 * reference has neither a stop flag nor a batch here, and neither has this. */
#define ORB_EG_MAX_KF 65536
#define ORB_EG_MAX_PROFILE_BYTES (256ull << 20)
#define ORB_EG_MAX_TRIALS 200
typedef struct {
    int32_t status;
    int32_t n_active;         /* vertices that an edge touches                                    */
    int32_t n_free;           /* ... of which not fixed: the block rows of the system             */
    int32_t n_edges;
    int64_t profile_bytes;    /* the factor's block profile                                       */
    int32_t iterations;       /* Levenberg iterations run                                         */
    int32_t trials;           /* trial steps in all                                               */
    int32_t refused;          /* trials whose system was not positive definite                    */
    int32_t reserved;
    double lambda;            /* lambda at the end (-1: nothing ran)                              */
    double chi2_before;
    double chi2_after;
    double trial_rho[ORB_EG_MAX_TRIALS];   /* the first ORB_EG_MAX_TRIALS trials                  */
    double trial_chi2[ORB_EG_MAX_TRIALS];
    uint8_t trial_accepted[ORB_EG_MAX_TRIALS];
} orb_essential_graph_info_t;
int orb_optimize_essential_graph(int n_kf, const float* kf_pose, const double* kf_corrected,
                                 const uint8_t* kf_has_corrected, const double* kf_noncorrected,
                                 const uint8_t* kf_has_noncorrected, const uint8_t* kf_fixed, int n_edge,
                                 const int32_t* edge_i, const int32_t* edge_j, const uint8_t* edge_kind, int n_pt,
                                 const float* pt_pos, const int32_t* pt_ref, const uint8_t* pt_skip, int n_iterations,
                                 double* kf_sim3_out, float* kf_pose_out, double* kf_pose_out_f64, float* pt_pos_out,
                                 double* pt_pos_out_f64, orb_essential_graph_info_t* info, int device);
/* Host arithmetic, no device: Sim3(R, t, 1.0) of a keyframe's Tcw (12 floats) as 8 doubles, with the bits
 * of the device's conversion, and [R | t (1 / s)] of a Sim3 as orb_optimize_essential_graph writes it
 * (LoopClosing::CorrectLoop lines 498-506 need both); pose / pose_f64 may be NULL. */
void orb_sim3_from_pose(const float* Tcw, double* sim3);
void orb_sim3_to_pose(const double* sim3, float* pose, double* pose_f64);
/* The point pass on its own (LoopClosing::CorrectLoop lines 466-495): out = to[pair]^-1.map(from[pair].map(P))
 * with P widened, pair = pt_pair[p] in [0, n_pair); pt_pair[p] == -1 returns the point as it is (bit for
 * bit in the float output).  sim3_from / sim3_to: n_pair x 8 doubles.  ORB_EINVAL: a pair index out of
 * range, a non-finite Sim3 value or a scale <= 0.  Host buffers, synchronous. */
int orb_sim3_correct_points(int n_pt, const float* pt_pos, const int32_t* pt_pair, int n_pair,
                            const double* sim3_from, const double* sim3_to, float* pt_pos_out,
                            double* pt_pos_out_f64, int device);

/* The local map of a tracked frame and a keyframe's covisibility (csrc/orb_localmapref.hip, DESIGN.md
 * §23): the counting, thresholding, ordering and de-duplicating of Tracking::UpdateReference and
 * KeyFrame::UpdateConnections over flat tables.  Integer only: parity is exact.  The caller owns the
 * map, hands the tables over with every call (the calls keep nothing) and mutates its map from what
 * comes back.  std::map<KeyFrame*, ...>'s pointer order is ASCENDING KEYFRAME INDEX here: the caller's
 * numbering decides ties for the reference keyframe, who is inside the limit of 80 and the order of
 * the local points.
 *   keyframes  n_kf (<= ORB_LM_MAX_KF): kf_bad n_kf u8 (isBad()); kf_mp_off n_kf + 1 offsets into kf_mp
 *              (n_kf_mp entries in all): GetMapPointMatches() per keypoint, a point index or -1 for
 *              NULL, at most ORB_LM_MAX_ROW per keyframe; kf_cov n_kf x 10:
 *              GetBestCovisibilityKeyFrames(10) in its order, the first -1 ends a row
 *   points     n_pt: pt_bad n_pt u8; pt_obs_off n_pt + 1 offsets into pt_obs_kf (n_obs entries in all):
 *              the keys of mObservations, each row strictly ascending
 * ORB_EINVAL: an index out of range anywhere, an offset table that is not monotone or leaves its
 * array, an observation row that is not strictly ascending.  ORB_ENOTSUP: more than ORB_LM_MAX_KF
 * keyframes, a row above ORB_LM_MAX_ROW, more than 65535 frames / keyframes in a batch, or scratch for
 * a single frame / keyframe above ORB_LM_MAX_SCRATCH_BYTES (decided from the sizes alone). */
#define ORB_LM_MAX_KF 65536
#define ORB_LM_MAX_ROW 8192
#define ORB_LM_MAX_SCRATCH_BYTES (256ull << 20)
typedef struct {
    const uint8_t* kf_bad;
    const int32_t* kf_mp_off;
    const int32_t* kf_mp;
    const int32_t* kf_cov;
    const uint8_t* pt_bad;
    const int32_t* pt_obs_off;
    const int32_t* pt_obs_kf;
    int32_t n_kf, n_pt, n_kf_mp, n_obs;
} orb_local_map_tables_t;
typedef struct {
    int32_t status;      /* ORB_OK, or why the frame was refused (counts 0, ref_kf -1; ORB_ERANGE: the counts needed) */
    int32_t n_voted;     /* voted keyframes that are not bad: the list before the neighbour step      */
    int32_t n_local_kf;  /* mvpLocalKeyFrames.size()                                                   */
    int32_t ref_kf;      /* mpReferenceKF: the first keyframe with the strict maximum, -1: none voted  */
    int32_t ref_votes;
    int32_t n_local_pt;  /* mvpLocalMapPoints.size()                                                   */
    int32_t n_cleared;   /* bad points of the frame set to NULL (Tracking.cc:821)                      */
} orb_local_map_info_t;
/* Tracking::UpdateReferenceKeyFrames (Tracking.cc:804-879), UpdateReferencePoints (778-801) and the
 * "already matched" pass of SearchReferencePointsInFrustum (718-734) for one frame on host buffers,
 * synchronous.  f_mp n entries (n <= ORB_LM_MAX_ROW): mCurrentFrame.mvpMapPoints, a point index or -1.
 * Outputs: f_mp_out n (bad points -1); local_kf cap_kf (mvpLocalKeyFrames: the voted keyframes in
 * ascending index, then the neighbours in the order they were appended); local_pt cap_pt
 * (mvpLocalMapPoints in order); local_pt_seen cap_pt u8 (1: the frame already holds the point, i.e.
 * mnLastFrameSeen == mnId at line 744: pass !seen as `usable` to orb_frame_is_in_frustum and
 * orb_search_by_projection_local); kf_votes n_kf (keyframeCounter, 0 where absent, bad keyframes
 * included; may be NULL); info.  ORB_ERANGE: a capacity too small; info holds the counts needed and
 * nothing else is written.  A frame that is empty or whose points are all bad: ORB_OK, empty lists,
 * ref_kf -1. */
int orb_local_map_reference(const orb_local_map_tables_t* map, int n, const int32_t* f_mp, int cap_kf, int cap_pt,
                            int32_t* f_mp_out, int32_t* local_kf, int32_t* local_pt, uint8_t* local_pt_seen,
                            int32_t* kf_votes, orb_local_map_info_t* info, int device);
/* B (<= 65535) frames on device arrays: d_map is a host struct of device pointers; d_f_mp B x cap with
 * d_counts[b] entries used (what lies past them is neither read nor written); outputs strided by cap,
 * cap_kf, cap_pt and n_kf.  A frame that the host form would refuse is left unwritten and reports its
 * status in d_info[b] (the call itself returns ORB_OK); a bad table refuses every frame.  Each
 * frame's result is the host form's bit for bit.  Frames run in chunks so that scratch stays under
 * ORB_LM_MAX_SCRATCH_BYTES.  Asynchronous on `stream`; scratch is stream-ordered. */
int orb_local_map_reference_batch_device(const orb_local_map_tables_t* d_map, int B, int cap, const int32_t* d_f_mp,
                                         const int32_t* d_counts, int cap_kf, int cap_pt, int32_t* d_f_mp_out,
                                         int32_t* d_local_kf, int32_t* d_local_pt, uint8_t* d_local_pt_seen,
                                         int32_t* d_kf_votes, orb_local_map_info_t* d_info, void* stream);
typedef struct {
    int32_t status;
    int32_t n_conn;     /* KFcounter.size()                                                            */
    int32_t n_ord;      /* mvpOrderedConnectedKeyFrames.size()                                         */
    int32_t unchanged;  /* 1: KFcounter was empty, the early return of KeyFrame.cc:365: write nothing back */
} orb_update_connections_info_t;
/* KeyFrame::UpdateConnections (KeyFrame.cc:332-411) for K (<= 65535) keyframes kf_idx, each on its own
 * (the function reads observations only).  Votes over the keyframe's non-NULL, non-bad points, itself
 * excluded, bad keyframes counted (the reference does not test them here); threshold >= 15, else the
 * first strict maximum alone.  Outputs, strided by cap_conn / cap_ord: conn_kf / conn_w
 * (mConnectedKeyFrameWeights in ascending index), ord_kf / ord_w (mvpOrderedConnectedKeyFrames /
 * mvOrderedWeights: weight descending, index descending among equal weights), info K records.  The
 * reverse AddConnection calls, the mbFirstConnection / mpParent step (ord_kf[0]) and the map mutation
 * stay with the caller.  Host form: synchronous; every record is returned, the rows
 * of the keyframes whose status is ORB_OK are written, and the first other status is the return
 * value.  ORB_ERANGE per keyframe: a capacity too small, counts in the record, its rows unwritten. */
int orb_keyframe_update_connections(const orb_local_map_tables_t* map, int K, const int32_t* kf_idx, int cap_conn,
                                    int cap_ord, int32_t* conn_kf, int32_t* conn_w, int32_t* ord_kf, int32_t* ord_w,
                                    orb_update_connections_info_t* info, int device);
/* The same on device arrays (d_map: a host struct of device pointers); statuses in d_info, the call
 * returns ORB_OK.  Asynchronous on `stream`; scratch is stream-ordered. */
int orb_keyframe_update_connections_batch_device(const orb_local_map_tables_t* d_map, int K, const int32_t* d_kf_idx,
                                                 int cap_conn, int cap_ord, int32_t* d_conn_kf, int32_t* d_conn_w,
                                                 int32_t* d_ord_kf, int32_t* d_ord_w,
                                                 orb_update_connections_info_t* d_info, void* stream);

/* ---- measurement ------------------------------------------------------------------- */
/* Per-stage HIP-event timing of the extraction kernels: when enabled, every
 * orb_extract_batch_device records an event pair around each stage on its launch stream.
 * orb_profile_read synchronises and returns cumulative milliseconds and launch counts per
 * stage (stage names via orb_profile_stage_name); the return value is the stage count.
 * Enabling (or re-enabling) resets the counters. */
int orb_profile_enable(orb_extractor_t* h, int enable);
/* The same for a subset of stages (bit k = stage k): every event pair is a stream boundary
 * (≈10 µs measured), so a timed run brackets only the stage it reports. */
int orb_profile_enable_stages(orb_extractor_t* h, unsigned stage_mask);
int orb_profile_read(orb_extractor_t* h, double* stage_ms, int64_t* stage_launches, int nstages);
const char* orb_profile_stage_name(int i);

/* Split orb_extract_batch_device into its two phases (scheduling only; results unchanged):
 * bit 0 = the image pyramid (ComputePyramid, ORBextractor.cc:781-822), bit 1 = detection,
 * selection, orientation and descriptors (ComputeKeyPoints + the descriptor loop,
 * ORBextractor.cc:522-707, 749-778), which read the pyramid that bit 0 left in the extractor's
 * workspace.  A caller running phase 1 then phase 2 for the same batch, on one stream or
 * event-ordered, gets exactly the mask-3 result; the gap between them lets other work (the
 * previous batch's matching) overlap the pyramid.  Default 3.  Applies to
 * orb_extract_batch_device only; every other extraction entry point runs both phases.
 * No reference counterpart. */
int orb_extract_set_phases(orb_extractor_t* h, unsigned phase_mask);

/* Test and diagnostic hooks (orb_debug_*): include/orb_debug.h. */

#ifdef __cplusplus
}
#endif
#endif /* ORB_ABI_H */
