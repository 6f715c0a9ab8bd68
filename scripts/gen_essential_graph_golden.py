#!/usr/bin/env python3
"""tests/golden/essential_graph_ring.npz: the CPU model's recorded answer for one ring (the scene's arrays
and what tests/native/essential_graph_model.cpp returns for them), and with --spread the model's own
spread, which the GPU tests' tolerances are 100 x of.

  gen_essential_graph_golden.py            write the fixture
  gen_essential_graph_golden.py --spread   the largest difference, over every listed case and the fixture,
                                           between the model's three sum orders and between its
                                           -ffp-contract=off and -ffp-contract=fast -mfma builds, of a Sim3
                                           entry, a pose entry, a point coordinate relative to the scene's
                                           scale and the final chi2 relative to the chi2 at the start
"""
from __future__ import annotations

import argparse
import pathlib
import subprocess
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import __graft_entry__ as entry  # noqa: E402
import essential_graph_model as egm  # noqa: E402
import essential_graph_scenes as egs  # noqa: E402

GOLDEN = ROOT / "tests" / "golden" / "essential_graph_ring.npz"
ARRAYS = ("kf_pose", "kf_fixed", "kf_corrected", "kf_has_corrected", "kf_noncorrected", "kf_has_noncorrected", "edge_i",
          "edge_j", "edge_kind", "pt_pos", "pt_ref", "pt_skip")


def deviations(a, b, scale):
    """(sim3, pose, point / scale, chi2 / chi2 at the start) between two answers of one scene."""
    before = max(a["info"]["chi2_before"], np.finfo(float).tiny)
    return (float(np.abs(a["kf_sim3"] - b["kf_sim3"]).max(initial=0.0)),
            float(np.abs(a["kf_pose_f64"] - b["kf_pose_f64"]).max(initial=0.0)),
            float(np.abs(a["pt_pos_f64"] - b["pt_pos_f64"]).max(initial=0.0)) / scale,
            abs(a["info"]["chi2_after"] - b["info"]["chi2_after"]) / before)


def write_golden():
    g, res, n_it, _ = egs.case(egs.GOLDEN_CASE)
    GOLDEN.parent.mkdir(exist_ok=True)
    np.savez_compressed(GOLDEN, **{k: np.asarray(g[k]) for k in ARRAYS}, scale=g["scale"], n_iterations=n_it,
                        model_kf_sim3=res["kf_sim3"], model_kf_pose_f64=res["kf_pose_f64"],
                        model_pt_pos_f64=res["pt_pos_f64"], model_chi2=np.array([res["info"]["chi2_before"],
                                                                                 res["info"]["chi2_after"]]),
                        model_counts=np.array([res["info"][k] for k in ("n_active", "n_free", "n_edges", "profile_bytes")]))
    print(f"wrote {GOLDEN} ({GOLDEN.stat().st_size} bytes)")


def spread():
    fma = ROOT / "build" / "libessential_graph_model_fma.so"
    subprocess.run(entry.ESSENTIAL_GRAPH_MODEL_CMD(fma, flags=("-ffp-contract=fast", "-mfma")), check=True)
    worst = np.zeros(4)
    for name in egs.CASES:
        g, res, n_it, _ = egs.case(name)
        row = np.zeros(4)
        for other in (egm.run(g, n_it, sum_order=egm.PAIRWISE), egm.run(g, n_it, sum_order=egm.REVERSED),
                      egm.run(g, n_it, path=fma)):
            row = np.maximum(row, deviations(res, other, g["scale"]))
        print(f"{name:28s} sim3 {row[0]:.3e}  pose {row[1]:.3e}  point {row[2]:.3e}  chi2 {row[3]:.3e}")
        worst = np.maximum(worst, row)
    print(f"{'worst':28s} sim3 {worst[0]:.3e}  pose {worst[1]:.3e}  point {worst[2]:.3e}  chi2 {worst[3]:.3e}")
    return worst


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--spread", action="store_true")
    a = ap.parse_args()
    if a.spread:
        spread()
    else:
        write_golden()
