#!/usr/bin/env python3
"""Time one PnPsolver::iterate of --n-hyp iterations on the GPU (csrc/orb_solvers.hip: orb_pnp_ransac,
orb_pnp_ransac_batch_device) against the path the same job took before the hypotheses moved to the
device, in one run.  Reports only; gates nothing.

Measured, each after a warm-up as the median over --runs windows, by the host clock (both paths end in
a synchronise, and the earlier path has host work in it):
  fused        orb_pnp_ransac on one solver with n = 100 and 300 correspondences (synthetic);
               orb_pnp_ransac_batch_device over S = --solvers candidates of a synthetic batch (a
               keyframe and a frame of --cap keypoints, about --matches matches per candidate, a quarter
               of them gross outliers), the upload of the rand() values included;
  earlier path the C++ model (tests/native/pnp_solver_model.cpp, -O3, one thread) drawing the sets,
               running compute_pose per set and Refine as the reference's loop does, then
               orb_pnp_check_inliers[_batch_device] on its hypotheses, their upload included.  For the
               batch the compact correspondences are already on the host: the copy back that a caller
               would also pay is not charged.  (The model's own CheckInliers runs inside its loop and is
               charged: Refine needs the masks.)
The batch form is also timed by device events around the enqueued calls alone; kernel-only time is not
measured.  Before anything is timed the fused results are compared with the model's.

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
    ap.add_argument("--cap", type=int, default=1024)
    ap.add_argument("--matches", type=int, default=150)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10, help="calls per timed window")
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()

    import torch

    import __graft_entry__ as ge

    if not torch.cuda.is_available():
        sys.exit("pnp_solver_timing: no GPU; a time taken elsewhere says nothing")
    if not (ROOT / "orbslam_jpminipc_amd" / "liborb_hip.so").exists():
        ge.build()
    import orbslam_jpminipc_amd as orb
    import pnp_solver_model as pm
    import solvers_model as model
    from orbslam_jpminipc_amd._native import KEYPOINT_DTYPE

    med = statistics.median
    n_hyp, f32 = a.n_hyp, np.float32
    K32 = f32(pm.K_CAM)
    K64 = np.float64(K32)
    TH2 = 5.991
    res = {"device": torch.cuda.get_device_name(0), "n_hyp": n_hyp, "runs": a.runs, "host_call": {}}

    def row(ts):
        return {"us": round(med(ts) * 1e6, 2), "min_us": round(min(ts) * 1e6, 2), "max_us": round(max(ts) * 1e6, 2)}

    def timed(fns, iters):
        for f in fns.values():
            f()
        ts = {k: [] for k in fns}
        for _ in range(a.runs):
            for k, f in fns.items():
                t0 = time.perf_counter()
                for _ in range(iters):
                    f()
                ts[k].append((time.perf_counter() - t0) / iters)
        return ts

    def same(got, want, what):
        for k in ("sets", "counts", "best_at", "refined_counts"):
            assert np.array_equal(got[k], want[k]), (what, k)
        for k in ("first_ok", "first_refined", "pose_inliers"):
            assert int(got[k]) == int(want[k]), (what, k)
        for k in ("R", "t", "pose"):
            assert np.array_equal(np.asarray(got[k]).reshape(np.shape(want[k])), want[k], equal_nan=True), (what, k)

    # ---- one solver, host buffers --------------------------------------------------------------
    for n in (100, 300):
        p3, p2, _, _ = pm.scene(n, n, noise=1.0, outliers=0.3)
        s2 = np.ones(n, f32)
        mi = orb.pnp_ransac_parameters(n, 0.99, 10, 300, 4, 0.5, TH2)["min_inliers"]
        rs, cons = orb.PnPRansac(*K32, min_inliers=mi, th2=TH2), orb.PnPConsensus(*K32, min_inliers=mi, th2=TH2)
        r = pm.draws(n_hyp, n)
        same(rs.iterate(p3, p2, s2, rand31=r), pm.ransac(p3, p2, s2, TH2, K64, mi, rand31=r), f"host n={n}")

        def earlier():
            m = pm.ransac(p3, p2, s2, TH2, K64, mi, rand31=r)
            return cons.check(p3, p2, s2, m["R"], m["t"])

        ts = timed({"fused": lambda: rs.iterate(p3, p2, s2, rand31=r), "earlier": earlier,
                    "model": lambda: pm.ransac(p3, p2, s2, TH2, K64, mi, rand31=r)}, a.iters)
        res["host_call"][str(n)] = {"fused": row(ts["fused"]), "earlier_path": row(ts["earlier"]),
                                    "of_which_model_1thread": row(ts["model"]),
                                    "earlier_over_fused": round(med(ts["earlier"]) / med(ts["fused"]), 2)}

    # ---- S candidates of one synthetic batch ---------------------------------------------------------
    S, cap = a.solvers, a.cap
    ls2 = model.LEVEL_SIGMA2
    rng = np.random.default_rng(5)
    p3, p2, _, _ = pm.scene(cap, 9, noise=1.0, outliers=0.25)
    perm = rng.permutation(cap)
    pos = np.zeros((2, cap, 3), f32)
    pos[0, perm] = p3
    kps = np.zeros((2, cap), KEYPOINT_DTYPE)
    kps["x"][1], kps["y"][1] = p2[:, 0], p2[:, 1]
    kps["octave"][1] = rng.integers(0, 3, cap)
    rows = np.full((S, cap), -1, np.int32)
    for s in range(S):
        j = np.sort(rng.choice(cap, int(rng.integers(a.matches // 2, a.matches * 3 // 2)), replace=False))
        rows[s, j] = perm[j]
    r = rng.integers(0, 2 ** 31, (S, n_hyp, 4)).astype(np.int32)
    tc = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
    d_kps, d_cnt = tc(kps.view(np.uint8).reshape(2, cap, -1)), tc(np.int32([cap, cap]))
    pa_, pb_ = tc(np.zeros(S, np.int32)), tc(np.ones(S, np.int32))
    d_rows, d_pos = tc(rows), tc(pos)
    mi = 30
    rs, cons = orb.PnPRansac(*K32, min_inliers=mi, th2=TH2), orb.PnPConsensus(*K32, min_inliers=mi, th2=TH2)
    sus = [model.pnp_setup(kps[1], cap, cap, rows[s], pos[0], None, ls2) for s in range(S)]

    def fused():
        out = rs.iterate_batch_device(d_kps, d_cnt, pa_, pb_, d_rows, d_pos, None, ls2, tc(r))
        torch.cuda.synchronize()
        return out

    R = np.zeros((S, n_hyp, 9))
    t = np.zeros((S, n_hyp, 3))

    def model_all():
        for s, su in enumerate(sus):
            m = pm.ransac(su["p3d"], su["p2d"], su["sigma2"], TH2, K64, mi, rand31=r[s])
            R[s], t[s] = m["R"], m["t"]

    def earlier():
        model_all()
        out = cons.check_batch_device(d_kps, d_cnt, pa_, pb_, d_rows, d_pos, None, ls2, tc(R), tc(t))
        torch.cuda.synchronize()
        return out

    out = {k: v.cpu().numpy() for k, v in fused().items()}
    for s, su in enumerate(sus):
        want = pm.ransac(su["p3d"], su["p2d"], su["sigma2"], TH2, K64, mi, rand31=r[s])
        same({k: out[k][s] for k in ("sets", "counts", "best_at", "refined_counts", "first_ok", "first_refined",
                                     "pose_inliers", "R", "t", "pose")}, want, f"batch solver {s}")
    ts = timed({"fused": fused, "earlier": earlier, "model": model_all}, max(1, a.iters // 5))
    d_r = tc(r)
    ev = []
    for _ in range(a.runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            rs.iterate_batch_device(d_kps, d_cnt, pa_, pb_, d_rows, d_pos, None, ls2, d_r)
        e1.record()
        e1.synchronize()
        ev.append(e0.elapsed_time(e1) * 1e-3 / a.iters)
    ns = [su["n"] for su in sus]
    res["batch"] = {"solvers": S, "cap": cap, "n_median": float(np.median(ns)), "n_max": int(max(ns)),
                    "refined_median": float(np.median((out["refined_counts"] >= 0).sum(1))),
                    "fused": row(ts["fused"]), "fused_device_events": row(ev), "kernel_only": "not measured",
                    "earlier_path": row(ts["earlier"]), "of_which_model_1thread": row(ts["model"]),
                    "earlier_over_fused": round(med(ts["earlier"]) / med(ts["fused"]), 2)}
    res["results_equal_model"] = True
    line = json.dumps(res)
    print(line)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
