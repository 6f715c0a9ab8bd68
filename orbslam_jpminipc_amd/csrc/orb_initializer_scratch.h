// orb_initializer_scratch.h — which arrays the two initializer chains of orb_initializer.hip keep in
// scratch.  No HIP here, and the kernels' argument structs are template parameters, so that
// tests/native/staging_host.cpp runs these very statements on the host.
#pragma once
#include "orb_staging.h"

constexpr int HY_NORM = 16;  // floats per (pair, side): T, meanX, meanY, sX, sY

// The device outputs of run_chain, each may be NULL.
struct ChainOut {
    float *H21, *H12, *F21, *Hn, *Fn, *norm;
    int32_t* sets_out;
    float *scores_h, *scores_f;
    int32_t* best_h;
    float* best_score_h;
    uint8_t* inliers_h;
    int32_t* best_f;
    float* best_score_f;
    uint8_t* inliers_f;
    int32_t* n_matches;
    float *best_H21, *best_F21, *RH;
    int32_t* use_h;
};

// The chain's arrays in `h` and, with `score`, `a`: the caller's where `o` has one, else a region of L.
template <class HypArgs, class InitArgs>
void chain_regions(OrbLayout& L, const ChainOut& o, bool score, int cap, int P, int n_hyp, HypArgs& h, InitArgs& a) {
    const size_t p = (size_t)P, hyp = p * n_hyp * 9;
    h.ord_i = L.take<int32_t>(p * cap);
    h.nmatch = L.given_or_take(o.n_matches, p);
    h.norm = L.given_or_take(o.norm, p * 2 * HY_NORM);
    h.H21 = o.H21 || !score ? o.H21 : L.take<float>(hyp);
    h.H12 = o.H12 || !score ? o.H12 : L.take<float>(hyp);
    h.F21 = o.F21 || !score ? o.F21 : L.take<float>(hyp);
    if (!score) return;
    a.scores[0] = L.given_or_take(o.scores_h, p * n_hyp);
    a.scores[1] = L.given_or_take(o.scores_f, p * n_hyp);
    a.best[0] = L.given_or_take(o.best_h, p);
    a.best[1] = L.given_or_take(o.best_f, p);
    a.best_score[0] = L.given_or_take(o.best_score_h, p);
    a.best_score[1] = L.given_or_take(o.best_score_f, p);
}

// The device outputs of run_reconstruct, each may be NULL.
struct RecOut {
    int32_t* ok;
    float *R21, *t21, *P3D;
    uint8_t* triangulated;
    int32_t* n_motion;
    float *motion_R, *motion_t;
    int32_t* n_good;
    float *cos_parallax, *parallax_deg;
    int32_t *best, *n_inliers;
};

// The reconstruction's arrays in `a`: the caller's where `o` has one, else a region of L.
template <class RecArgs>
void rec_regions(OrbLayout& L, const RecOut& o, int cap, int P, RecArgs& a) {
    const size_t p = (size_t)P, pc = p * cap;
    a.ord_i = L.take<int32_t>(pc);
    a.nwalk = L.take<int32_t>(p);
    a.flags = L.take<uint8_t>(pc * 8);
    a.cosv = L.take<float>(pc * 8);
    a.n_motion = L.given_or_take(o.n_motion, p);
    a.n_inliers = L.given_or_take(o.n_inliers, p);
    a.best = L.given_or_take(o.best, p);
    a.motion_R = L.given_or_take(o.motion_R, p * 72);
    a.motion_t = L.given_or_take(o.motion_t, p * 24);
    a.n_good = L.given_or_take(o.n_good, p * 8);
    a.cos_sel = L.given_or_take(o.cos_parallax, p * 8);
    a.parallax = L.given_or_take(o.parallax_deg, p * 8);
}
