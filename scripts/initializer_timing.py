#!/usr/bin/env python3
"""Time the Initializer scoring (csrc/orb_initializer.hip) on the GPU against the single-threaded
C++ model of the same checks (tests/native/initializer_model.cpp, -O3), in one run.  Reports
only; gates nothing.

Measured, each after a warm-up as the median over --runs windows:
  host call   orb_initializer_check on one pair with N = 100, 300, 1000 matches (synthetic
              keypoints, 2 x n_hyp hypotheses), host clock around the synchronous call;
  batch       orb_initializer_check_batch_device over the P = B - 1 consecutive pairs of a
              640x480 / 1000-keypoint batch of B = 512 synthetic frames (the c3 step of bench.py)
              with the matches orb_search_for_initialization_batch_device wrote for them, device
              events around the enqueued calls;
  model       the C++ model on one CPU thread on the same inputs (all P pairs for the batch).
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
    ap.add_argument("--n-hyp", type=int, default=200)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50, help="host calls per timed window")
    ap.add_argument("--batch-iters", type=int, default=100, help="batched calls per timed window")
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()

    import torch

    import __graft_entry__ as ge

    if not torch.cuda.is_available():
        sys.exit("initializer_timing: no GPU; a time taken elsewhere says nothing")
    if not (ROOT / "orbslam_jpminipc_amd" / "liborb_hip.so").exists():
        ge.build()
    import initializer_model as model
    import orbslam_jpminipc_amd as orb
    from orbslam_jpminipc_amd._native import KEYPOINT_DTYPE
    from test_gpu_initializer import synth_case

    med = statistics.median
    init = orb.Initializer(1.0, a.n_hyp)
    res = {"device": torch.cuda.get_device_name(0), "n_hyp": a.n_hyp, "runs": a.runs, "host_call": {}}

    def row(ts):
        return {"us": round(med(ts) * 1e6, 2), "min_us": round(min(ts) * 1e6, 2), "max_us": round(max(ts) * 1e6, 2)}

    # ---- one pair, host buffers ---------------------------------------------------------------
    for N in (100, 300, 1000):
        case = synth_case(N, a.n_hyp)
        got = init.check(*case)
        want = model.check(case[0], case[1], case[2], 1.0, *case[3:])
        model.same_result(got, want)
        for _ in range(10):
            init.check(*case)
        t_gpu, t_cpu = [], []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            for _ in range(a.iters):
                init.check(*case)  # synchronous: returns after the device is done
            t_gpu.append((time.perf_counter() - t0) / a.iters)
            t0 = time.perf_counter()
            for _ in range(5):
                model.check(case[0], case[1], case[2], 1.0, *case[3:])
            t_cpu.append((time.perf_counter() - t0) / 5)
        res["host_call"][str(N)] = {"gpu": row(t_gpu), "cpu_model_1thread": row(t_cpu),
                                    "cpu_over_gpu": round(med(t_cpu) / med(t_gpu), 2)}

    # ---- the c3 batch ----------------------------------------------------------------------------
    W, H, B = 640, 480, a.batch
    frames = orb.synth_stream(W, H, stream=0, first=0, count=B)
    ext = orb.ORBextractor(1000, 1.2, 8, orb.FAST_SCORE, 20, device=0, max_batch=B)
    kps, desc, cnt = ext.extract_batch_device(torch.from_numpy(frames).cuda())
    f1 = torch.arange(0, B - 1, dtype=torch.int32, device="cuda")
    f2 = f1 + 1
    m12, nm = orb.ORBmatcher(0.9, True).search_for_initialization_batch_device(kps, desc, cnt, f1, f2, W, H, 100)
    torch.cuda.synchronize()
    P, cap = m12.shape
    hyp = synth_case(200, a.n_hyp)[3:]  # any values serve; the same set for every pair
    d_hyp = [torch.from_numpy(np.ascontiguousarray(np.broadcast_to(h, (P,) + h.shape))).cuda() for h in hyp]
    out = init.check_batch_device(kps, cnt, f1, f2, m12, *d_hyp)
    torch.cuda.synchronize()
    h_kps = kps.cpu().numpy().view(KEYPOINT_DTYPE).reshape(B, cap)
    h_cnt, h_m12 = cnt.cpu().numpy(), m12.cpu().numpy()
    o = {k: v.cpu().numpy() for k, v in out.items()}

    def model_pair(p):
        return model.check(h_kps[p, : h_cnt[p]], h_kps[p + 1, : h_cnt[p + 1]], h_m12[p, : h_cnt[p]], 1.0, *hyp)

    for p in range(P):
        want = model_pair(p)
        n = want["n_matches"]
        assert n == o["n_matches"][p] == nm[p].item()
        for t in "hf":
            assert model.same_scores(o["scores_" + t][p], want["scores_" + t]), (p, t)
            assert o["best_" + t][p] == want["best_" + t]
            assert np.array_equal(o["inliers_" + t][p, :n].astype(bool), want["inliers_" + t])
    for _ in range(3):
        init.check_batch_device(kps, cnt, f1, f2, m12, *d_hyp)
    torch.cuda.synchronize()
    t_gpu, t_cpu = [], []
    for r in range(a.runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.batch_iters):
            init.check_batch_device(kps, cnt, f1, f2, m12, *d_hyp)
        e1.record()
        e1.synchronize()
        t_gpu.append(e0.elapsed_time(e1) * 1e-3 / a.batch_iters)
        if r < 3:
            t0 = time.perf_counter()
            for p in range(P):
                model_pair(p)
            t_cpu.append(time.perf_counter() - t0)
    res["batch"] = {"pairs": int(P), "cap": int(cap), "matches_total": int(o["n_matches"].sum()),
                    "matches_median": float(np.median(o["n_matches"])), "gpu": row(t_gpu),
                    "gpu_us_per_pair": round(med(t_gpu) * 1e6 / P, 3), "cpu_model_1thread": row(t_cpu),
                    "cpu_over_gpu": round(med(t_cpu) / med(t_gpu), 1)}
    res["results_equal_model"] = True
    line = json.dumps(res)
    print(line)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
