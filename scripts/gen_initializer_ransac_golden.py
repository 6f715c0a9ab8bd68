#!/usr/bin/env python3
"""Writes tests/golden/initializer_ransac_320x240.npz: 200 x 8 rand() values for the committed
frame pair (scene_320x240_nf500 / _f1 with the matches of match_320x240_f0_f1) and the CPU model's
answer for them (tests/initializer_ransac_model.py: sets, hypotheses; tests/initializer_model.py:
scores, bests, masks; RH).

Thirteen of the 200 sets are made to draw, as their second draw (some as their third too), the
position their first draw emptied, which then holds the entry moved there from the back of the
list; at this pair's N = 54 random draws often do so as well.  The script refuses the data unless at least 8 sets draw a moved entry again, at
least one hypothesis of each model scores above 0, and the best of each model beats the runner-up
by a margin in score.
"""
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import initializer_ransac_model as model  # noqa: E402
from test_initializer_model import golden_inputs  # noqa: E402
from test_initializer_ransac_model import draw_for, replay_sets  # noqa: E402

GOLD = ROOT / "tests" / "golden"
SEED = 20261022
N_HYP = 200
SIGMA = 1.0
MARGIN = 1e-3  # relative, between the best score of a model and the next distinct one
f32 = np.float32


def main():
    k1, k2, m12, _ = golden_inputs()
    N = int((m12 >= 0).sum())
    assert N >= 16, N
    rng = np.random.default_rng(SEED)
    rand31 = rng.integers(0, 1 << 31, (N_HYP, 8), dtype=np.int64)
    for k, it in enumerate(range(5, N_HYP, 16)):  # 13 sets: the second draw lands where the first did
        q = int(rng.integers(0, N - 2))
        rand31[it, 0] = draw_for(q, N)
        rand31[it, 1] = draw_for(q, N - 1)
        if k % 3 == 0:  # ... and the third once more
            rand31[it, 2] = draw_for(q, N - 2)
    rand31 = rand31.astype(np.int32)
    sets, moved = replay_sets(N, rand31)
    print(f"N = {N}; {int(moved.sum())} sets draw a moved entry again")
    assert moved.sum() >= 8
    r = model.find(k1, k2, m12, rand31, SIGMA)
    assert np.array_equal(r["sets"], sets) and r["n_matches"] == N
    for t in "hf":
        s = r["scores_" + t]
        assert not np.isnan(s).any() and (s > 0).any() and r["best_" + t] >= 0
        top = np.unique(s)[::-1]
        gap = (top[0] - top[1]) / top[0]
        print(f"{t}: best {r['best_' + t]} score {r['best_score_' + t]!r}, {int(r['inliers_' + t].sum())}/{N} inliers, "
              f"margin to the runner-up {gap:.3e}")
        assert (s == top[0]).sum() == 1 and gap > MARGIN, "change SEED: the best is not unique by a margin"
    print(f"RH = {r['RH']!r}, use_h = {r['use_h']}")
    np.savez_compressed(
        GOLD / "initializer_ransac_320x240.npz", sigma=f32(SIGMA), rand31=rand31, sets=r["sets"], H21=r["H21"],
        H12=r["H12"], F21=r["F21"], n_matches=np.int32(N), scores_h=r["scores_h"], scores_f=r["scores_f"],
        best_h=np.int32(r["best_h"]), best_f=np.int32(r["best_f"]), best_score_h=r["best_score_h"],
        best_score_f=r["best_score_f"], inliers_h=r["inliers_h"], inliers_f=r["inliers_f"], H=r["H"], F=r["F"],
        RH=f32(r["RH"]), use_h=np.bool_(r["use_h"]))
    print("wrote", GOLD / "initializer_ransac_320x240.npz")


if __name__ == "__main__":
    main()
