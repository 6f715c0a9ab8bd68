#!/usr/bin/env python3
"""Timing of Optimizer::OptimizeEssentialGraph on the GPU against the C++ model on one CPU thread
(DESIGN.md §22).  Ring graphs of 100, 500 and 2000 keyframes with 5 edges per keyframe (the chain and
four covisibility edges), 20 loop rows and 50 points per keyframe.  The results are compared with the
model first; then medians of 7 of the host clock around the synchronous call, and of the model (its
profile solve, -O3, one thread) on the same host in the same run.  Prints one JSON line; the raw line
is kept in profiles/optimizer/essential_graph_timing.json.

Not measured: g2o and CHOLMOD themselves (they cannot be built here), and kernel time apart from the
staging and the copies of the host call."""
from __future__ import annotations

import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import essential_graph_model as egm  # noqa: E402
import essential_graph_scenes as egs  # noqa: E402

SHAPES = (100, 500, 2000)
REPEATS = 7
PANEL_COLUMNS = 28  # EG_PW of csrc/orb_essgraph.hip


def main():
    import orbslam_jpminipc_amd as orb

    opt = orb.Optimizer(0)
    tables = ("kf_corrected", "kf_has_corrected", "kf_noncorrected", "kf_has_noncorrected", "pt_pos", "pt_ref", "pt_skip")
    rows = []
    for n_kf in SHAPES:
        g, want = egs.ring(n_kf, n_corrected=20, n_loop_to=3, seed=7, covis=(2, 3, 4, 5), pts_per_kf=50)

        def call():
            return opt.OptimizeEssentialGraph(g["kf_pose"], g["kf_fixed"], g["edge_i"], g["edge_j"], g["edge_kind"],
                                              **{k: g[k] for k in tables})

        got = call()
        dev = {"sim3": float(np.abs(got["kf_sim3"] - want["kf_sim3"]).max()),
               "pose": float(np.abs(got["kf_pose_f64"] - want["kf_pose_f64"]).max()),
               "point": float(np.abs(got["pt_pos_f64"] - want["pt_pos_f64"]).max()) / g["scale"],
               "chi2": abs(got["info"]["chi2_after"] - want["info"]["chi2_after"]) / want["info"]["chi2_before"]}
        assert dev["sim3"] <= 1e-4 and dev["pose"] <= 3e-4 and dev["point"] <= 6e-6 and dev["chi2"] <= 1e-5, dev
        assert got["info"]["trials"] == want["info"]["trials"], (got["info"]["trials"], want["info"]["trials"])
        gpu, cpu = [], []
        for _ in range(REPEATS):
            t = time.perf_counter()
            call()
            gpu.append(time.perf_counter() - t)
            t = time.perf_counter()
            egm.run(g)
            cpu.append(time.perf_counter() - t)
        I = got["info"]
        n_cols = 7 * I["n_free"]
        panels = -(-n_cols // PANEL_COLUMNS)
        rows.append({"keyframes": n_kf, "edges": int(I["n_edges"]), "points": int(len(g["pt_pos"])),
                     "free": I["n_free"], "profile_bytes": int(I["profile_bytes"]), "iterations": I["iterations"],
                     "trials": I["trials"], "launches_per_trial": 2 * panels - 1 + 5,
                     "gpu_ms": 1e3 * float(np.median(gpu)), "model_ms": 1e3 * float(np.median(cpu)),
                     "cpu_over_gpu": float(np.median(cpu) / np.median(gpu)), "deviation": dev, "seed": g["seed"]})
    print(json.dumps({"essential_graph_timing": rows, "repeats": REPEATS}))


if __name__ == "__main__":
    main()
