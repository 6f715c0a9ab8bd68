#!/usr/bin/env python3
"""Time Optimizer::LocalBundleAdjustment (csrc/orb_localba.hip) on the GPU against the single-threaded
C++ model of the same routine (tests/native/local_ba_model.cpp, -O3), in one run.  Reports only;
gates nothing.

Measured, each after a warm-up as the median over --runs windows:
  host call   orb_local_bundle_adjustment on one window of 5 free + 3 fixed keyframes with 300 points,
              20 + 20 with 2000 and 64 + 40 with 5000 (tests/local_ba_scenes.py, 8 observations per
              point, 10 % gross outliers), host clock around the synchronous call;
  batch       orb_local_bundle_adjustment_batch_device over S = 16 windows of the middle shape, device
              events around the enqueued calls;
  model       the C++ model on one CPU thread on the same inputs (all S windows for the batch).
Before anything is timed the GPU results are compared with the model's (flags and counts exactly,
the f64 poses and points within the tests' tolerances).

Prints one JSON line; --out also writes it to a file."""
import argparse
import json
import pathlib
import statistics
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

POSE_TOL, POINT_TOL = 1.0e-8, 2.0e-6  # tests/test_gpu_local_ba.py
SHAPES = {"5+3_300": (5, 3, 300), "20+20_2000": (20, 20, 2000), "64+40_5000": (64, 40, 5000)}
OBS_PER_POINT = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=16)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5, help="host calls per timed window")
    ap.add_argument("--batch-iters", type=int, default=3, help="batched calls per timed window")
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()

    import torch

    import __graft_entry__ as ge

    if not torch.cuda.is_available():
        sys.exit("local_ba_timing: no GPU; a time taken elsewhere says nothing")
    if not (ROOT / "orbslam_jpminipc_amd" / "liborb_hip.so").exists():
        ge.build()
    import orbslam_jpminipc_amd as orb
    import local_ba_model as lbm
    import local_ba_scenes as sc

    med = statistics.median
    opt = orb.Optimizer(0)
    res = {"device": torch.cuda.get_device_name(0), "runs": a.runs, "obs_per_point": OBS_PER_POINT, "host_call": {}}
    worst = {"pose": 0.0, "point": 0.0}

    def row(ts):
        return {"ms": round(med(ts) * 1e3, 3), "min_ms": round(min(ts) * 1e3, 3), "max_ms": round(max(ts) * 1e3, 3)}

    def agree(got, want, scale):
        assert lbm.decisive(want, scale)
        assert np.array_equal(got["edge_erased"], want["edge_erased"]) and np.array_equal(got["pt_bad"], want["pt_bad"])
        dp = float(np.abs(got["kf_pose_f64"] - want["kf_pose_f64"]).max())
        dx = float(np.abs(got["pt_pos_f64"] - want["pt_pos_f64"]).max())
        assert dp <= POSE_TOL and dx <= POINT_TOL, (dp, dx)
        worst["pose"], worst["point"] = max(worst["pose"], dp), max(worst["point"], dx)

    # ---- one window, host buffers -------------------------------------------------------------------
    scenes = {}
    for name, (nf, nx, npt) in SHAPES.items():
        g = scenes[name] = sc.make_scene(7000 + npt, nf, nx, npt, OBS_PER_POINT)
        gpu = lambda: opt.local_bundle_adjustment(*[g[k] for k in sc.GRAPH_KEYS])  # noqa: E731
        cpu = lambda: lbm.local_bundle_adjustment(g)  # noqa: E731
        r = gpu()
        agree(r, g["model"], g["scale"])
        for _ in range(2):
            gpu()
        t_gpu, t_cpu = [], []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            for _ in range(a.iters):
                gpu()  # synchronous: returns after the device is done
            t_gpu.append((time.perf_counter() - t0) / a.iters)
            t0 = time.perf_counter()
            cpu()
            t_cpu.append(time.perf_counter() - t0)
        rounds = r["info"]["round"]
        res["host_call"][name] = {"edges": int(len(g["edge_pt"])), "gpu": row(t_gpu), "cpu_model_1thread": row(t_cpu),
                                  "cpu_over_gpu": round(med(t_cpu) / med(t_gpu), 2),
                                  "iterations": [x["iterations"] for x in rounds], "trials": [x["trials"] for x in rounds]}

    # ---- S windows of the middle shape ---------------------------------------------------------------
    S = a.problems
    nf, nx, npt = SHAPES["20+20_2000"]
    probs = [sc.make_scene(8000 + 30 * s, nf, nx, npt, OBS_PER_POINT) for s in range(S)]
    arrays = [lbm.graph_arrays(g) for g in probs]
    cat = {k: torch.from_numpy(np.concatenate([x[k] for x in arrays])).cuda() for k in sc.GRAPH_KEYS}
    off = {f: torch.from_numpy(np.concatenate([[0], np.cumsum([len(x[k]) for x in arrays])]).astype(np.int32)).cuda()
           for f, k in (("kf", "kf_pose"), ("pt", "pt_pos"), ("edge", "edge_pt"))}
    gpu = lambda: opt.local_bundle_adjustment_batch_device(off["kf"], off["pt"], off["edge"],  # noqa: E731
                                                           *[cat[k] for k in sc.GRAPH_KEYS])
    out = gpu()
    torch.cuda.synchronize()
    o = {k: v.cpu().numpy() for k, v in out.items()}
    ho = {f: v.cpu().numpy() for f, v in off.items()}
    span = {"kf_pose_f64": "kf", "pt_pos_f64": "pt", "edge_erased": "edge", "pt_bad": "pt"}
    for s, g in enumerate(probs):
        agree({k: o[k][ho[f][s]:ho[f][s + 1]] for k, f in span.items()}, g["model"], g["scale"])
    gpu()
    torch.cuda.synchronize()
    t_gpu, t_cpu = [], []
    for _ in range(a.runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.batch_iters):
            gpu()
        e1.record()
        e1.synchronize()
        t_gpu.append(e0.elapsed_time(e1) * 1e-3 / a.batch_iters)
        t0 = time.perf_counter()
        for g in probs:
            lbm.local_bundle_adjustment(g)
        t_cpu.append(time.perf_counter() - t0)
    res["batch"] = {"problems": S, "shape": "20+20_2000", "gpu": row(t_gpu),
                    "gpu_ms_per_problem": round(med(t_gpu) * 1e3 / S, 3), "cpu_model_1thread": row(t_cpu),
                    "cpu_over_gpu": round(med(t_cpu) / med(t_gpu), 2)}
    res["results_equal_model"] = True
    res["worst_pose_deviation"], res["worst_point_deviation"] = worst["pose"], worst["point"]
    line = json.dumps(res)
    print(line)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
