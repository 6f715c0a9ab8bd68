#!/usr/bin/env python3
"""Time Optimizer::OptimizeSim3 (csrc/orb_sim3opt.hip) on the GPU against the single-threaded C++
model of the same routine (tests/native/sim3_optimization_model.cpp, -O3), in one run.  Reports
only; gates nothing.

Measured, each after a warm-up as the median over --runs windows:
  host call   orb_optimize_sim3 on one candidate with n = 30, 100, 300 pairs (synthetic, 10 % gross
              outliers: the range loop closing sees), host clock around the synchronous call;
  batch       orb_optimize_sim3_batch_device over S = 1, 10, 50 candidate pairs of keyframes of a
              640x480 / 1000-keypoint batch of synthetic frames (match rows built on the host, the
              MapPoints placed so that each pair is consistent with a Sim3 of its own), device events
              around the enqueued calls;
  model       the C++ model on one CPU thread on the same inputs (all S problems for the batch).
Before anything is timed the GPU results are compared with the model's (kept, counts and
more_iterations exactly, the f64 Sim3 within the tests' tolerance).

Not measured: kernel time alone; a multi-threaded CPU baseline.

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

SIM3_TOL = 3.1e-5  # tests/test_gpu_sim3_optimization.py


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50, help="host calls per timed window")
    ap.add_argument("--batch-iters", type=int, default=20, help="batched calls per timed window")
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()

    import torch

    import __graft_entry__ as ge

    if not torch.cuda.is_available():
        sys.exit("sim3_optimization_timing: no GPU; a time taken elsewhere says nothing")
    if not (ROOT / "orbslam_jpminipc_amd" / "liborb_hip.so").exists():
        ge.build()
    import orbslam_jpminipc_amd as orb
    import sim3_optimization_model as s3m
    from orbslam_jpminipc_amd._native import KEYPOINT_DTYPE
    from orbslam_jpminipc_amd.optimizer import SIM3_INFO_DTYPE

    med = statistics.median
    opt = orb.Optimizer(0)
    res = {"device": torch.cuda.get_device_name(0), "runs": a.runs, "host_call": {}, "batch": {}}
    worst = 0.0

    def row(ts):
        return {"us": round(med(ts) * 1e6, 2), "min_us": round(min(ts) * 1e6, 2), "max_us": round(max(ts) * 1e6, 2)}

    def agree(kept, s64, n_in, info, want):
        nonlocal worst
        assert s3m.decisive(want)
        assert np.array_equal(np.asarray(kept, np.uint8), want["kept"]) and n_in == want["n_inliers"]
        wi = want["info"]
        assert (info["n_correspondences"], info["n_bad"], info["more_iterations"]) == \
            (wi.n_correspondences, wi.n_bad, wi.more_iterations)
        dev = float(np.abs(s64 - want["sim3_f64"]).max())
        assert dev <= SIM3_TOL, dev
        worst = max(worst, dev)

    # ---- one candidate, host buffers ---------------------------------------------------------------
    for n in (30, 100, 300):
        c = s3m.make_case(7000 + n, n)
        gpu = lambda: opt.optimize_sim3(c["x3dc1"], c["x3dc2"], c["obs1"], c["obs2"], c["inv_sigma2_1"],  # noqa: E731
                                        c["sigma2_2"], c["K1"], c["K2"], c["sim3_in"], th2=c["th2"],
                                        usable=c["usable"])
        cpu = lambda: s3m.run_case(c)  # noqa: E731
        r = gpu()
        agree(r["kept"], r["sim3_f64"], r["n_inliers"], r["info"], c["model"])
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

    # ---- S candidates over one 640x480 batch ---------------------------------------------------------
    W, H, B, PER = 640, 480, 12, 150
    K = np.float32([517.3, 516.5, 318.6, 239.5])
    frames = orb.synth_stream(W, H, stream=0, first=0, count=B)
    ext = orb.ORBextractor(1000, 1.2, 8, orb.FAST_SCORE, 20, device=0, max_batch=B)
    kps, _, cnt = ext.extract_batch_device(torch.from_numpy(frames).cuda())
    cap = int(kps.shape[1])
    h_kps = kps.cpu().numpy().view(KEYPOINT_DTYPE).reshape(B, cap)
    h_cnt = cnt.cpu().numpy()
    tc = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
    for S in (1, 10, 50):
        # candidate s pairs keyframe s % B with (s + 1 + s // B) % B; every candidate has positions of
        # its own, so the batch arrays are laid out per candidate: B' = 2 S pseudo-keyframes
        Bp = 2 * S
        src = np.array([[s % B, (s + 1 + s // B) % B] for s in range(S)]).reshape(-1)
        d_kps2, d_cnt2 = kps[torch.from_numpy(src).cuda()].contiguous(), cnt[torch.from_numpy(src).cuda()].contiguous()
        for seed in range(40):
            rng = np.random.default_rng(1000 * S + seed)
            pos, pose = np.zeros((Bp, cap, 3), np.float32), np.zeros((Bp, 12), np.float32)
            rows, sim3_in = np.full((S, cap), -1, np.int32), np.zeros((S, 13), np.float32)
            want, cases = [], []
            for s in range(S):
                fa, fb = 2 * s, 2 * s + 1
                na, nb = int(h_cnt[src[fa]]), int(h_cnt[src[fb]])
                for f in (fa, fb):
                    pose[f] = np.concatenate([s3m.rot(rng.normal(0, 0.05, 3)).reshape(9), rng.normal(0, 0.1, 3)])
                k = min(na, nb, PER)
                ia, ib = np.sort(rng.choice(na, k, replace=False)), rng.choice(nb, k, replace=False)
                rows[s, ia] = ib
                R12, t12, sc = s3m.rot(rng.normal(0, 0.1, 3)), rng.normal(0, 0.3, 3), float(rng.uniform(0.8, 1.25))
                ka, kb = h_kps[src[fa], ia], h_kps[src[fb], ib]
                za, zb = rng.uniform(4, 12, k), rng.uniform(4, 12, k)
                ua, va = ka["x"] + rng.normal(0, 0.5, k), ka["y"] + rng.normal(0, 0.5, k)
                ua[rng.random(k) < 0.1] += 40
                P1 = np.stack([(ua - K[2]) / K[0] * za, (va - K[3]) / K[1] * za, za], 1)
                X2c = ((P1 - t12) @ R12) / sc
                sg = s3m.LEVEL_SIGMA2[np.clip(kb["octave"], 0, 7)].astype(np.float64)
                ub, vb = kb["x"] + rng.normal(0, 0.5, k) / np.sqrt(sg), kb["y"] + rng.normal(0, 0.5, k) / np.sqrt(sg)
                P2 = np.stack([(ub - K[2]) / K[0] * zb, (vb - K[3]) / K[1] * zb, zb], 1)
                X1c = sc * (P2 @ R12.T) + t12
                Ra, ta = pose[fa, :9].reshape(3, 3).astype(np.float64), pose[fa, 9:].astype(np.float64)
                Rb, tb = pose[fb, :9].reshape(3, 3).astype(np.float64), pose[fb, 9:].astype(np.float64)
                pos[fa, ia] = ((X1c - ta) @ Ra).astype(np.float32)
                pos[fb, ib] = ((X2c - tb) @ Rb).astype(np.float32)
                sim3_in[s] = s3m.sim3_13(s3m.rot(rng.normal(0, 0.02, 3)) @ R12, t12 + rng.normal(0, 0.05, 3),
                                         sc * (1 + rng.normal(0, 0.02)))
                su = s3m.batch_setup(h_kps[src[fa]], na, h_kps[src[fb]], nb, rows[s], pos[fa], None, pos[fb], None,
                                     pose[fa], pose[fb])
                su.update(K1=K, K2=K, th2=s3m.TH2, sim3_in=sim3_in[s])
                cases.append(su)
                want.append(s3m.run_case(su))
            if all(s3m.decisive(w) for w in want):
                break
        else:
            sys.exit("no decisive seed")
        pa = torch.arange(0, Bp, 2, dtype=torch.int32, device="cuda")
        pb = torch.arange(1, Bp, 2, dtype=torch.int32, device="cuda")
        d_rows, d_pos, d_pose, d_in = tc(rows), tc(pos), tc(pose), tc(sim3_in)
        gpu = lambda: opt.optimize_sim3_batch_device(d_kps2, d_cnt2, pa, pb, d_rows, d_pos, None, d_pose,  # noqa: E731
                                                     s3m.LEVEL_SIGMA2, K, d_in)
        out = gpu()
        torch.cuda.synchronize()
        o = {k: v.cpu().numpy() for k, v in out.items()}
        ns = []
        for s in range(S):
            n = len(cases[s]["usable"])
            inf = o["info"][s].view(SIM3_INFO_DTYPE)[0]
            info = {k: int(inf[k]) for k in ("n_correspondences", "n_bad", "more_iterations")}
            agree((cases[s]["usable"] == 1) & (o["match"][s, :n] >= 0), o["sim3_f64"][s], int(o["n_inliers"][s]), info,
                  want[s])
            ns.append(info["n_correspondences"])
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
                s3m.run_case(cases[s])
            t_cpu.append(time.perf_counter() - t0)
        res["batch"][str(S)] = {"problems": S, "cap": cap, "pairs_median": float(np.median(ns)), "pairs_max": int(max(ns)),
                                "gpu": row(t_gpu), "gpu_us_per_problem": round(med(t_gpu) * 1e6 / S, 3),
                                "cpu_model_1thread": row(t_cpu), "cpu_over_gpu": round(med(t_cpu) / med(t_gpu), 2)}
    res["results_equal_model"] = True
    res["worst_sim3_deviation"] = worst
    line = json.dumps(res)
    print(line)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
