/* liborb_hip.so test and diagnostic hooks: NOT part of the reference's API surface.
 *
 * Exported by the product library so that the GPU parity tests can inspect intermediate
 * results (pyramid levels, the descriptor image, per-cell FAST counts), force a code path that
 * ordinary frames rarely reach (k_fast's plane-scan fallback, the per-level pyramid kernels) and
 * check the libstdc++ nth_element replays in isolation.  None of them changes a result.  The
 * per-phase timing probes of the kernels (orb_debug_{ps,km,kr,ks,kf}_timing) exist only in
 * experiment builds (-DPS_TIMING=1 etc.), never in the product library; each is defined in its
 * kernel's unit (ps, kf: csrc/orb_ilp.hip; kr, ks: csrc/orb_hip.hip; km: csrc/orb_sfi.hip).
 */
#ifndef ORB_DEBUG_H
#define ORB_DEBUG_H
#include "orb_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- test hooks (no device work unless stated) ------------------------------------- */
/* Host instantiation of the kernels' libstdc++ nth_element replay on packed u32 elements
 * (score in bits 24..31), for CPU unit tests against std::nth_element. */
int orb_debug_nth_element_u32(uint32_t* a, int n, int nth);
/* The one-wave (ballot-partition) replay k_select uses, run on `device` (n <= 8192). */
int orb_debug_nth_element_wave_u32(uint32_t* a, int n, int nth, int device);
/* Padded pyramid level l of batch frame b after the last extraction (device sync). */
int orb_debug_level_image(orb_extractor_t* h, int b, int l, uint8_t* out, int* w, int* hgt);
/* The rest of each of that level's rows up to the row pitch: (h+32) rows of pitch - (w+32) bytes
 * (the return value, 0 .. 15; out may be NULL to ask for it).  Every pyramid builder writes zeros
 * there, so that the workspace is the same bytes whichever builder ran (device sync). */
int orb_debug_level_row_slack(orb_extractor_t* h, int b, int l, uint8_t* out);
/* Descriptor image (blurred ROI + un-blurred padding ring) of level l, frame b, padded
 * (w+32) x (h+32) layout; defined over [-3, w+3) x [-3, h+3) at least (wider where a dense
 * cell grid lets keypoints sit past the FAST border) (device sync). */
int orb_debug_blur_image(orb_extractor_t* h, int b, int l, uint8_t* out);
/* Per-cell FAST keypoint counts of frame b, level l (device sync); returns #cells. */
int orb_debug_cell_counts(orb_extractor_t* h, int b, int l, int* counts, int cap);
/* Pyramid kernels used by the next extractions (results are identical): 0 = automatic (the
 * one-pass streaming kernel k_pyr_stream for batches >= 256 grey frames, per-level launches
 * otherwise), 1 = per-level launches always, 2 = k_pyr_stream at every batch size of grey
 * frames whenever the current geometry has a stream plan. */
int orb_debug_set_pyramid_path(orb_extractor_t* h, int mode);
/* k_fast keeps each wave's corners in a list of up to 256 entries and falls back to scanning the
 * whole strength plane of its tile when a wave finds more; cap (0 .. 256) lowers that list's
 * capacity for the next extractions so the fallback runs on ordinary frames (results are
 * identical; test hook, tests/test_gpu_fast_fallback.py).  The default is 256. */
int orb_debug_set_fast_corner_list(orb_extractor_t* h, int cap);
/* The current geometry's k_pyr_stream plan: returns 1 (and level-0 rows per round, rounds,
 * LDS bytes) when there is one, 0 when the geometry only runs per-level launches. */
int orb_debug_pyramid_plan(const orb_extractor_t* h, int* rows_per_round, int* rounds, int* lds_bytes);
/* Per level of that plan (0 and nothing written when there is none; else the number of levels,
 * the first min(levels, cap) written): nq = tasks per padded row (16-byte chunks at level 0,
 * 4-pixel quads above), n_waves = the workgroup's waves that build the level (a level whose
 * nq <= 64 * n_waves decodes its columns once, hoisted out of the rounds; the others decode per
 * round), ring_rows = rows of the level's LDS ring (0 for the last level, which has none). */
int orb_debug_pyramid_plan_levels(const orb_extractor_t* h, int* nq, int* n_waves, int* ring_rows, int cap);
/* Set every byte of the handle's pyramid workspace (all levels of all max_batch frames, padding
 * and slack included) to `value` (0 .. 255), ordered after the handle's last launch and before
 * its next.  A test that poisons the workspace before a build then compares bytes that this
 * build wrote, not what an earlier one left.  The pyramid of phase 1 is gone afterwards. */
int orb_debug_fill_pyramid(orb_extractor_t* h, int value);
/* Per-slot tables of the database's last host query (q = 0) or of query q of its last batch, for
 * slots 0 .. min(cap, highest id used + 1) - 1 (the return value): common = shared words (0 for a
 * slot that is not live), first_word = the smallest shared word (0xFFFFFFFF: none), seq = the
 * slot's add counter now, scored = 1 where common > minCommon in the sharing list, score = the
 * L1 score of the scan (every sharing keyframe has one).  Tests use it to tell a wrong count from
 * a wrong score from a wrong order (device sync). */
int orb_debug_kfdb_last_query(orb_keyframe_db_t* db, int q, int32_t* common, uint32_t* first_word, uint32_t* seq,
                              uint8_t* scored, double* score, int cap);
/* The byte cap under which orb_local_map_reference* and orb_keyframe_update_connections* keep their
 * per-chunk scratch, for the calls that follow in this process (0: ORB_LM_MAX_SCRATCH_BYTES).  A small
 * cap makes a small batch run in several chunks, and a cap below one frame's scratch shows the
 * ORB_ENOTSUP answer; results are identical (tests/test_gpu_local_map.py). */
int orb_debug_set_local_map_scratch_cap(size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* ORB_DEBUG_H */
