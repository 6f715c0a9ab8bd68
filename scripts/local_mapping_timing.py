#!/usr/bin/env python3
"""Time CreateNewMapPoints' triangulation on the GPU (csrc/orb_localmap.hip) against the C++ model of the
same job on one thread (tests/native/local_mapping_model.cpp, -O3), in one run.  Reports only; gates
nothing.

Measured, each after a warm-up as the median over --runs windows:
  batch      orb_create_new_map_points_batch_device over --pairs pairs of --matches matches each (keyframes
             of --keypoints keypoints, the baseline gate on), by device events around the enqueued calls;
  host call  orb_create_new_map_points on one such pair, by the host clock (the call ends in a synchronise);
  model      local_mapping_model_create on the same pair, and looped over all --pairs pairs of the batch
             inside one timed window (measured, not multiplied), by the host clock, through its ctypes wrapper
             (the wrapper's array preparation is inside the window: it is part of what a caller of the
             model pays, and small against the 4 x 4 decompositions).
Before anything is timed the results are compared with the model's.  Kernel time alone is not measured.

Prints one JSON line; --out also writes it to a file."""
import argparse
import copy
import json
import pathlib
import statistics
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--matches", type=int, default=300)
    ap.add_argument("--keypoints", type=int, default=1000)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20, help="calls per timed window")
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()

    import torch

    import __graft_entry__ as ge

    if not torch.cuda.is_available():
        sys.exit("local_mapping_timing: no GPU; a time taken elsewhere says nothing")
    if not (ROOT / "orbslam_jpminipc_amd" / "liborb_hip.so").exists():
        ge.build()
    import local_mapping_model as model
    import local_mapping_scenes as scenes
    import orbslam_jpminipc_amd as orb
    from orbslam_jpminipc_amd._native import KEYPOINT_DTYPE

    med = statistics.median
    lm = orb.LocalMapping(0)
    n, m, P = a.keypoints, a.matches, a.pairs
    cap = 1 << (n - 1).bit_length()
    s = scenes.accept_scene(m, n, n - 8)
    views = [copy.copy(s["V1"]), copy.copy(s["V2"])]
    for V in views:
        V.Ow = model.center(model.pose12(V))
    pos2, has2 = scenes.map_points_of(views[1], 3)

    def row(ts):
        return {"us": round(med(ts) * 1e6, 2), "min_us": round(min(ts) * 1e6, 2), "max_us": round(max(ts) * 1e6, 2)}

    def timed(f, iters):
        f()
        ts = []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            for _ in range(iters):
                f()
            ts.append((time.perf_counter() - t0) / iters)
        return ts

    want = model.create(views[0], views[1], s["match12"], pos2, has2)
    model.same_result(lm.triangulate(views[0], views[1], s["match12"], pos2, has2), want)
    t_host = timed(lambda: lm.triangulate(views[0], views[1], s["match12"], pos2, has2), a.iters)
    t_model = timed(lambda: model.create(views[0], views[1], s["match12"], pos2, has2), a.iters)

    kps = np.zeros((2, cap), KEYPOINT_DTYPE)
    mp_pos, has_mp = np.zeros((2, cap, 3), np.float32), np.zeros((2, cap), np.uint8)
    for b, V in enumerate(views):
        kps[b, :V.n] = V.kps
    mp_pos[1, :views[1].n], has_mp[1, :views[1].n] = pos2, has2
    match = np.full((P, cap), -1, np.int32)
    match[:, :n] = s["match12"]
    tc = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
    d_kps = tc(kps.view(np.uint8).reshape(2, cap * 28))
    d_cnt, d_pose = tc(np.array([V.n for V in views], np.int32)), tc(np.stack([model.pose12(V) for V in views]))
    d_a, d_b, d_match = tc(np.zeros(P, np.int32)), tc(np.ones(P, np.int32)), tc(match)
    d_pos, d_has = tc(mp_pos), tc(has_mp)
    sf, s2, K4 = scenes.SF[:scenes.NLEVELS], scenes.SIGMA2[:scenes.NLEVELS], np.array(scenes.CALIB, np.float32)
    out = lm.create_new_map_points_batch_device(d_kps, d_cnt, cap, d_a, d_b, d_match, d_pose, sf, s2, K4, d_pos, d_has)
    torch.cuda.synchronize()
    for p in (0, P - 1):
        got = dict(x3d=out["x3d"][p, :n].cpu().numpy(), status=out["status"][p, :n].cpu().numpy(),
                   cos_rays=out["cos_rays"][p, :n].cpu().numpy(), n_new=int(out["n_new"][p]),
                   new_idx1=out["new_idx1"][p, :want["n_new"]].cpu().numpy(),
                   new_idx2=out["new_idx2"][p, :want["n_new"]].cpu().numpy(), skipped=int(out["skipped"][p]),
                   median_depth=float(out["median_depth"][p]))
        model.same_result(got, want)

    def enqueue():
        lm.create_new_map_points_batch_device(d_kps, d_cnt, cap, d_a, d_b, d_match, d_pose, sf, s2, K4, d_pos, d_has, out)

    enqueue()
    torch.cuda.synchronize()
    ev = []
    for _ in range(a.runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            enqueue()
        e1.record()
        e1.synchronize()
        ev.append(e0.elapsed_time(e1) * 1e-3 / a.iters)
    def model_all():  # the batch's job on one thread: every pair, one after the other
        for _ in range(P):
            model.create(views[0], views[1], s["match12"], pos2, has2)

    t_model_all = timed(model_all, 1)
    res = {"device": torch.cuda.get_device_name(0), "runs": a.runs, "iters": a.iters, "keypoints": n, "matches": m,
           "accepted": want["n_new"], "cap": cap,
           "host_call_one_pair": row(t_host), "model_one_pair_1thread": row(t_model),
           "batch": {"pairs": P, "device_events": row(ev), "per_pair_us": round(med(ev) * 1e6 / P, 3),
                     "model_1thread_same_job": row(t_model_all),
                     "model_over_batch": round(med(t_model_all) / med(ev), 1),
                     "note": "every pair of the batch is the same two keyframes with the same match row"},
           "model_over_host_call": round(med(t_model) / med(t_host), 2), "results_equal_model": True,
           "not_measured": "kernel time alone (no profiler run)"}
    line = json.dumps(res)
    print(line)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
