#!/usr/bin/env python3
"""Time the PnP / Sim3 consensus (csrc/orb_solvers.hip) on the GPU against the single-threaded C++
model of the same checks (tests/native/solvers_model.cpp, -O3), in one run.  Reports only; gates
nothing.

Measured, each after a warm-up as the median over --runs windows:
  host call   orb_pnp_check_inliers / orb_sim3_check_inliers on one solver with n = 100, 300, 1000
              correspondences and --n-hyp hypotheses (synthetic), host clock around the synchronous
              call;
  batch       orb_*_check_inliers_batch_device over S = --solvers candidates (keyframes 1..S
              against frame 0 of a 640x480 / 1000-keypoint batch of synthetic frames) with the rows
              orb_search_by_bow_batch_device wrote for them, device events around the enqueued
              calls;
  model       the C++ model on one CPU thread on the same inputs (set-up and consensus of all S
              solvers for the batch).
Before anything is timed the GPU results are compared with the model's.

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-hyp", type=int, default=300)
    ap.add_argument("--solvers", type=int, default=50)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50, help="host calls per timed window")
    ap.add_argument("--batch-iters", type=int, default=50, help="batched calls per timed window")
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()

    import torch

    import __graft_entry__ as ge

    if not torch.cuda.is_available():
        sys.exit("solvers_timing: no GPU; a time taken elsewhere says nothing")
    if not (ROOT / "orbslam_jpminipc_amd" / "liborb_hip.so").exists():
        ge.build()
    import orbslam_jpminipc_amd as orb
    import solvers_model as model
    from orbslam_jpminipc_amd._native import KEYPOINT_DTYPE
    from vocab_util import random_vocabulary

    med = statistics.median
    res = {"device": torch.cuda.get_device_name(0), "n_hyp": a.n_hyp, "runs": a.runs, "host_call": {"pnp": {}, "sim3": {}}}

    def row(ts):
        return {"us": round(med(ts) * 1e6, 2), "min_us": round(min(ts) * 1e6, 2), "max_us": round(max(ts) * 1e6, 2)}

    def timed(gpu, cpu):
        for _ in range(10):
            gpu()
        t_gpu, t_cpu = [], []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            for _ in range(a.iters):
                gpu()  # synchronous: returns after the device is done
            t_gpu.append((time.perf_counter() - t0) / a.iters)
            t0 = time.perf_counter()
            for _ in range(3):
                cpu()
            t_cpu.append((time.perf_counter() - t0) / 3)
        return {"gpu": row(t_gpu), "cpu_model_1thread": row(t_cpu), "cpu_over_gpu": round(med(t_cpu) / med(t_gpu), 2)}

    # ---- one solver, host buffers --------------------------------------------------------------
    for n in (100, 300, 1000):
        c = model.pnp_case(n, a.n_hyp, seed=n)
        cons = orb.PnPConsensus(*c["K"], min_inliers=n // 2)
        pa = (c["p3d"], c["p2d"], c["sigma2"], c["R"], c["t"])
        cpu = lambda: model.pnp(c["p3d"], c["p2d"], c["sigma2"], 5.991, c["K"], c["R"], c["t"], n // 2)  # noqa: E731
        model.same_result(cons.check(*pa), cpu(), "first_ok")
        res["host_call"]["pnp"][str(n)] = timed(lambda: cons.check(*pa), cpu)
        s = model.sim3_case(n, a.n_hyp, seed=n + 1)
        scons = orb.Sim3Consensus(s["K1"], s["K2"], n // 2)
        sa = (s["x3dc1"], s["x3dc2"], s["sigma2_1"], s["sigma2_2"])
        scpu = lambda: model.sim3(*sa, s["K1"], s["K2"], s["T12"], s["T21"], n // 2)  # noqa: E731
        model.same_result(scons.check(*sa, s["T12"], s["T21"]), scpu(), "first_accept")
        res["host_call"]["sim3"][str(n)] = timed(lambda: scons.check(*sa, s["T12"], s["T21"]), scpu)

    # ---- S candidates of one 640x480 batch ---------------------------------------------------------
    W, H, S, n_hyp = 640, 480, a.solvers, a.n_hyp
    B = S + 1
    K = np.float32([517.3, 516.5, 318.6, 239.5])
    ls2 = model.LEVEL_SIGMA2
    frames = orb.synth_stream(W, H, stream=0, first=0, count=B)
    ext = orb.ORBextractor(1000, 1.2, 8, orb.FAST_SCORE, 20, device=0, max_batch=B)
    kps, desc, cnt = ext.extract_batch_device(torch.from_numpy(frames).cuda())
    voc = orb.ORBVocabulary.from_arrays(8, 3, 0, 0, *random_vocabulary(8, 3, seed=3))
    fv = voc.transform_batch_device(desc, cnt, 1)
    pa_ = torch.arange(1, B, dtype=torch.int32, device="cuda")
    pb_ = torch.zeros(S, dtype=torch.int32, device="cuda")
    cap = int(kps.shape[1])
    rng = np.random.default_rng(5)
    pos = np.stack([rng.uniform(-2, 2, (B, cap)), rng.uniform(-1.5, 1.5, (B, cap)), rng.uniform(2, 8, (B, cap))],
                   2).astype(np.float32)
    bad = (rng.random((B, cap)) < 0.1).astype(np.uint8)
    pose = np.zeros((B, 12), np.float32)
    pose[:, [0, 4, 8]] = 1
    pose[:, 9:] = rng.normal(0, 0.1, (B, 3))
    R = np.stack([model.rodrigues(rng.normal(0, 0.02, 3)) for _ in range(S * n_hyp)]).reshape(S, n_hyp, 9)
    t = rng.normal(0, 0.05, (S, n_hyp, 3))
    T12 = np.concatenate([R.reshape(S, n_hyp, 3, 3), t[..., None]], 3).astype(np.float32)
    T21 = np.concatenate([R.reshape(S, n_hyp, 3, 3).transpose(0, 1, 3, 2),
                          -np.einsum("shji,shj->shi", R.reshape(S, n_hyp, 3, 3), t)[..., None]], 3).astype(np.float32)
    tc = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
    d_pos, d_bad, d_pose, d_R, d_t, d_T12, d_T21 = (tc(x) for x in (pos, bad, pose, R, t, T12, T21))
    h_kps = kps.cpu().numpy().view(KEYPOINT_DTYPE).reshape(B, cap)
    h_cnt = cnt.cpu().numpy()
    pnp = orb.PnPConsensus(*K, min_inliers=10)
    sim = orb.Sim3Consensus(K, None, 20)
    res["batch"] = {"solvers": S, "cap": cap}
    for name in ("pnp", "sim3"):
        rows, _ = orb.ORBmatcher(0.75, True).search_by_bow_batch_device(name == "sim3", kps, desc, cnt, fv, pa_, pb_)
        torch.cuda.synchronize()
        h_rows = rows.cpu().numpy()
        if name == "pnp":
            gpu = lambda: pnp.check_batch_device(kps, cnt, pa_, pb_, rows, d_pos, d_bad, ls2, d_R, d_t)  # noqa: E731

            def cpu(s):
                su = model.pnp_setup(h_kps[0], h_cnt[0], h_cnt[s + 1], h_rows[s], pos[s + 1], bad[s + 1], ls2)
                return su, model.pnp(su["p3d"], su["p2d"], su["sigma2"], 5.991, K, R[s], t[s], 10)
        else:
            gpu = lambda: sim.check_batch_device(kps, cnt, pa_, pb_, rows, d_pos, d_bad, d_pose, ls2, d_T12, d_T21)  # noqa: E731

            def cpu(s):
                su = model.sim3_setup(h_kps[s + 1], h_cnt[s + 1], h_kps[0], h_cnt[0], h_rows[s], pos[s + 1], bad[s + 1],
                                      pos[0], bad[0], pose[s + 1], pose[0], ls2)
                return su, model.sim3(su["x3dc1"], su["x3dc2"], su["sigma2_1"], su["sigma2_2"], K, K, T12[s], T21[s], 20)
        out = gpu()
        torch.cuda.synchronize()
        o = {k: v.cpu().numpy() for k, v in out.items()}
        first = "first_ok" if name == "pnp" else "first_accept"
        ns = []
        for s in range(S):
            su, want = cpu(s)
            wm = want["masks"].shape[1]
            assert su["n"] == o["n"][s] and np.array_equal(su["index"], o["index"][s]), (name, s)
            assert np.array_equal(want["counts"], o["counts"][s]) and np.array_equal(want["best_at"], o["best_at"][s])
            m = o["masks"][s].view(np.uint64)
            assert np.array_equal(m[:, :wm], want["masks"]) and not m[:, wm:].any() and want[first] == o[first][s]
            ns.append(su["n"])
        for _ in range(3):
            gpu()
        torch.cuda.synchronize()
        t_gpu, t_cpu = [], []
        for r in range(a.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.batch_iters):
                gpu()
            e1.record()
            e1.synchronize()
            t_gpu.append(e0.elapsed_time(e1) * 1e-3 / a.batch_iters)
            t0 = time.perf_counter()
            for s in range(S):
                cpu(s)
            t_cpu.append(time.perf_counter() - t0)
        res["batch"][name] = {"n_median": float(np.median(ns)), "n_max": int(max(ns)), "gpu": row(t_gpu),
                              "gpu_us_per_solver": round(med(t_gpu) * 1e6 / S, 3), "cpu_model_1thread": row(t_cpu),
                              "cpu_over_gpu": round(med(t_cpu) / med(t_gpu), 1)}
    res["results_equal_model"] = True
    line = json.dumps(res)
    print(line)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
