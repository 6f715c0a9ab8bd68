#!/usr/bin/env python3
"""Time Optimizer::PoseOptimization (csrc/orb_optimizer.hip) on the GPU against the single-threaded
C++ model of the same routine (tests/native/pose_optimization_model.cpp, -O3), in one run.  Reports
only; gates nothing.

Measured, each after a warm-up as the median over --runs windows:
  host call   orb_pose_optimization on one frame with n = 100, 300, 1000 edges (synthetic, 20 %
              outliers), host clock around the synchronous call;
  batch       orb_pose_optimization_batch_device over S = --problems problems on the frames of a
              640x480 / 1000-keypoint batch of synthetic frames (MapPoints back-projected from each
              frame's own keypoints), device events around the enqueued calls;
  model       the C++ model on one CPU thread on the same inputs (all S problems for the batch).
Before anything is timed the GPU results are compared with the model's (flags and counts exactly,
the f64 pose within the tests' tolerance).

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

POSE_TOL = 7.0e-8  # tests/test_gpu_pose_optimization.py


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=50)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50, help="host calls per timed window")
    ap.add_argument("--batch-iters", type=int, default=20, help="batched calls per timed window")
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()

    import torch

    import __graft_entry__ as ge

    if not torch.cuda.is_available():
        sys.exit("pose_optimization_timing: no GPU; a time taken elsewhere says nothing")
    if not (ROOT / "orbslam_jpminipc_amd" / "liborb_hip.so").exists():
        ge.build()
    import orbslam_jpminipc_amd as orb
    import pose_optimization_model as pom
    from orbslam_jpminipc_amd._native import KEYPOINT_DTYPE
    from orbslam_jpminipc_amd.optimizer import INFO_DTYPE

    med = statistics.median
    opt = orb.Optimizer(0)
    res = {"device": torch.cuda.get_device_name(0), "runs": a.runs, "host_call": {}}
    worst = 0.0

    def row(ts):
        return {"us": round(med(ts) * 1e6, 2), "min_us": round(min(ts) * 1e6, 2), "max_us": round(max(ts) * 1e6, 2)}

    def agree(got_flags, got_pose64, got_inl, want):
        nonlocal worst
        assert pom.decisive(want)
        assert np.array_equal(np.asarray(got_flags, np.uint8), want["outlier"]) and got_inl == want["n_inliers"]
        dev = float(np.abs(got_pose64 - want["pose_f64"]).max())
        assert dev <= POSE_TOL, dev
        worst = max(worst, dev)

    # ---- one frame, host buffers -------------------------------------------------------------------
    for n in (100, 300, 1000):
        c = pom.make_case(7000 + n, n)
        args = (c["p3d"], c["obs"], c["inv_sigma2"], c["has_mp"], c["K"], c["pose_in"])
        gpu = lambda: opt.pose_optimization(c["obs"], c["p3d"], c["has_mp"], pose_in=c["pose_in"], K=c["K"],  # noqa: E731
                                            inv_sigma2=c["inv_sigma2"])
        cpu = lambda: pom.pose_optimization(*args)  # noqa: E731
        r = gpu()
        agree(r["outlier"], r["pose_f64"], r["n_inliers"], c["model"])
        for _ in range(10):
            gpu()
        t_gpu, t_cpu = [], []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            for _ in range(a.iters):
                gpu()  # synchronous: returns after the device is done
            t_gpu.append((time.perf_counter() - t0) / a.iters)
            t0 = time.perf_counter()
            for _ in range(5):
                cpu()
            t_cpu.append((time.perf_counter() - t0) / 5)
        res["host_call"][str(n)] = {"gpu": row(t_gpu), "cpu_model_1thread": row(t_cpu),
                                    "cpu_over_gpu": round(med(t_cpu) / med(t_gpu), 2),
                                    "iterations": r["info"]["iterations"], "trials": r["info"]["trials"]}

    # ---- S problems over one 640x480 batch -----------------------------------------------------------
    W, H, S = 640, 480, a.problems
    K = np.float32([517.3, 516.5, 318.6, 239.5])
    inv_ls2 = (np.float32(1.0) / pom.LEVEL_SIGMA2).astype(np.float32)
    frames = orb.synth_stream(W, H, stream=0, first=0, count=S)
    ext = orb.ORBextractor(1000, 1.2, 8, orb.FAST_SCORE, 20, device=0, max_batch=S)
    kps, _, cnt = ext.extract_batch_device(torch.from_numpy(frames).cuda())
    cap = int(kps.shape[1])
    h_kps = kps.cpu().numpy().view(KEYPOINT_DTYPE).reshape(S, cap)
    h_cnt = cnt.cpu().numpy()
    for seed in range(40):
        rng = np.random.default_rng(seed)
        pos, has, pose_in = np.zeros((S, cap, 3), np.float32), np.zeros((S, cap), np.uint8), np.zeros((S, 12), np.float32)
        want, cpu_args = [], []
        for s in range(S):
            n = int(h_cnt[s])
            Rt, tt = pom.rot(rng.normal(0, 0.2, 3)), rng.normal(0, 0.5, 3)
            z = rng.uniform(4, 12, n)
            u = h_kps["x"][s, :n] + rng.normal(0, 0.7, n)
            v = h_kps["y"][s, :n] + rng.normal(0, 0.7, n)
            bad = rng.random(n) < 0.2
            u[bad] += rng.uniform(-40, 40, int(bad.sum()))
            Xc = np.stack([(u - K[2]) / K[0] * z, (v - K[3]) / K[1] * z, z], 1)
            pos[s, :n] = ((Xc - tt) @ Rt).astype(np.float32)
            has[s, :n] = rng.random(n) < 0.5
            pose_in[s] = np.concatenate([(pom.rot(rng.normal(0, 0.02, 3)) @ Rt).reshape(9),
                                         tt + rng.normal(0, 0.1, 3)]).astype(np.float32)
            k = h_kps[s, :n]
            cpu_args.append((pos[s, :n].copy(), np.stack([k["x"], k["y"]], 1), inv_ls2[np.clip(k["octave"], 0, 7)],
                             has[s, :n].copy(), K, pose_in[s].copy()))
            want.append(pom.pose_optimization(*cpu_args[-1]))
        if all(pom.decisive(w) for w in want):
            break
    else:
        sys.exit("no decisive seed")
    tc = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
    d_frame_of = torch.arange(S, dtype=torch.int32, device="cuda")
    d_pos, d_has, d_pose = tc(pos), tc(has), tc(pose_in)
    gpu = lambda: opt.pose_optimization_batch_device(kps, cnt, d_frame_of, d_pos, d_has, inv_ls2, K, d_pose)  # noqa: E731
    out = gpu()
    torch.cuda.synchronize()
    o = {k: v.cpu().numpy() for k, v in out.items()}
    ns = []
    for s in range(S):
        n = int(h_cnt[s])
        agree(o["outlier"][s, :n], o["pose_f64"][s], int(o["n_inliers"][s]), want[s])
        ns.append(int(o["info"][s].view(INFO_DTYPE)[0]["n_initial"]))
    for _ in range(3):
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
        for s in range(S):
            pom.pose_optimization(*cpu_args[s])
        t_cpu.append(time.perf_counter() - t0)
    res["batch"] = {"problems": S, "cap": cap, "edges_median": float(np.median(ns)), "edges_max": int(max(ns)),
                    "gpu": row(t_gpu), "gpu_us_per_problem": round(med(t_gpu) * 1e6 / S, 3),
                    "cpu_model_1thread": row(t_cpu), "cpu_over_gpu": round(med(t_cpu) / med(t_gpu), 1)}
    res["results_equal_model"] = True
    res["worst_pose_deviation"] = worst
    line = json.dumps(res)
    print(line)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
