#!/usr/bin/env python3
"""Time one Sim3Solver::iterate of --n-hyp iterations on the GPU (csrc/orb_solvers.hip:
orb_sim3_ransac, orb_sim3_ransac_batch_device) against the path the same job took before the
hypotheses moved to the device, in one run.  Reports only; gates nothing.

Measured, each after a warm-up as the median over --runs windows, by the host clock (both paths end
in a synchronise, and the earlier path has host work in it):
  fused        orb_sim3_ransac on one solver with n = 100, 300, 1000 correspondences (synthetic);
               orb_sim3_ransac_batch_device over S = --solvers candidates of a 640x480 /
               1000-keypoint batch, the upload of the rand() values included;
  earlier path the C++ model (tests/native/sim3_solver_model.cpp, -O3, one thread) drawing the sets
               and running computeT, then orb_sim3_check_inliers[_batch_device] on its hypotheses,
               their upload included.  For the batch the compact correspondences are already on the
               host: the copy back that a caller would also pay is not charged.
The batch form is also timed by device events around the enqueued calls alone.
Before anything is timed the fused results are compared with the model's.

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
    ap.add_argument("--iters", type=int, default=30, help="calls per timed window")
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()

    import torch

    import __graft_entry__ as ge

    if not torch.cuda.is_available():
        sys.exit("sim3_solver_timing: no GPU; a time taken elsewhere says nothing")
    if not (ROOT / "orbslam_jpminipc_amd" / "liborb_hip.so").exists():
        ge.build()
    import orbslam_jpminipc_amd as orb
    import sim3_solver_model as s3
    import solvers_model as model
    from orbslam_jpminipc_amd._native import KEYPOINT_DTYPE
    from vocab_util import random_vocabulary

    med = statistics.median
    n_hyp = a.n_hyp
    res = {"device": torch.cuda.get_device_name(0), "n_hyp": n_hyp, "runs": a.runs, "host_call": {}}

    def row(ts):
        return {"us": round(med(ts) * 1e6, 2), "min_us": round(min(ts) * 1e6, 2), "max_us": round(max(ts) * 1e6, 2)}

    def timed(fns, iters):
        for f in fns.values():
            for _ in range(3):
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
        for k in ("sets", "counts", "best_at"):
            assert np.array_equal(got[k], want[k]), (what, k)
        assert got["first_accept"] == want["first_accept"], what
        for k in ("T12", "T21", "sim3"):
            assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), (what, k)
            assert np.allclose(got[k], want[k], rtol=0, atol=1e-5, equal_nan=True), (what, k)

    # ---- one solver, host buffers --------------------------------------------------------------
    for n in (100, 300, 1000):
        c = s3.cloud(n, seed=n, outliers=0.3)
        K = np.asarray(model.K_TUM, np.float32)
        mi = n // 2
        rs, cons = orb.Sim3Ransac(K, K, mi), orb.Sim3Consensus(K, K, mi)
        sa = (c["x3dc1"], c["x3dc2"], c["sigma2_1"], c["sigma2_2"])
        r = np.random.default_rng(n).integers(0, 2 ** 31, (n_hyp, 3)).astype(np.int32)
        same(rs.iterate(*sa, rand31=r), s3.iterate(*sa, K, K, r, mi), f"host n={n}")

        def earlier():
            hyp = s3.compute(sa[0], sa[1], s3.sets(n, r))
            return cons.check(*sa, hyp["T12"], hyp["T21"])

        ts = timed({"fused": lambda: rs.iterate(*sa, rand31=r), "earlier": earlier,
                    "model_hypotheses": lambda: s3.compute(sa[0], sa[1], s3.sets(n, r))}, a.iters)
        res["host_call"][str(n)] = {"fused": row(ts["fused"]), "earlier_path": row(ts["earlier"]),
                                    "of_which_model_hypotheses_1thread": row(ts["model_hypotheses"]),
                                    "earlier_over_fused": round(med(ts["earlier"]) / med(ts["fused"]), 2)}

    # ---- S candidates of one 640x480 batch ---------------------------------------------------------
    W, H, S = 640, 480, a.solvers
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
    r = rng.integers(0, 2 ** 31, (S, n_hyp, 3)).astype(np.int32)
    tc = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
    d_pos, d_bad, d_pose = tc(pos), tc(bad), tc(pose)
    rows, _ = orb.ORBmatcher(0.75, True).search_by_bow_batch_device(True, kps, desc, cnt, fv, pa_, pb_)
    torch.cuda.synchronize()
    h_kps = kps.cpu().numpy().view(KEYPOINT_DTYPE).reshape(B, cap)
    h_cnt, h_rows = cnt.cpu().numpy(), rows.cpu().numpy()
    mi = 20
    rs, cons = orb.Sim3Ransac(K, None, mi), orb.Sim3Consensus(K, None, mi)
    sus = [model.sim3_setup(h_kps[s + 1], h_cnt[s + 1], h_kps[0], h_cnt[0], h_rows[s], pos[s + 1], bad[s + 1], pos[0],
                            bad[0], pose[s + 1], pose[0], ls2) for s in range(S)]

    def fused():
        out = rs.iterate_batch_device(kps, cnt, pa_, pb_, rows, d_pos, d_bad, d_pose, ls2, tc(r))
        torch.cuda.synchronize()
        return out

    T12 = np.zeros((S, n_hyp, 12), np.float32)
    T21 = np.zeros((S, n_hyp, 12), np.float32)

    def model_hypotheses():
        for s, su in enumerate(sus):
            if su["n"] >= mi:
                hyp = s3.compute(su["x3dc1"], su["x3dc2"], s3.sets(su["n"], r[s]))
                T12[s], T21[s] = hyp["T12"].reshape(n_hyp, 12), hyp["T21"].reshape(n_hyp, 12)

    def earlier():
        model_hypotheses()
        out = cons.check_batch_device(kps, cnt, pa_, pb_, rows, d_pos, d_bad, d_pose, ls2, tc(T12), tc(T21))
        torch.cuda.synchronize()
        return out

    out = {k: v.cpu().numpy() for k, v in fused().items()}
    for s, su in enumerate(sus):
        want = s3.iterate(su["x3dc1"], su["x3dc2"], su["sigma2_1"], su["sigma2_2"], K, K, r[s], mi)
        got = {k: out[k][s] for k in ("sets", "counts", "best_at")}
        got.update(first_accept=int(out["first_accept"][s]), T12=out["T12"][s].reshape(n_hyp, 3, 4),
                   T21=out["T21"][s].reshape(n_hyp, 3, 4), sim3=out["sim3"][s])
        same(got, want, f"batch solver {s}")
    ts = timed({"fused": fused, "earlier": earlier, "model_hypotheses": model_hypotheses}, max(1, a.iters // 10))
    d_r = tc(r)
    ev = []
    for _ in range(a.runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            rs.iterate_batch_device(kps, cnt, pa_, pb_, rows, d_pos, d_bad, d_pose, ls2, d_r)
        e1.record()
        e1.synchronize()
        ev.append(e0.elapsed_time(e1) * 1e-3 / a.iters)
    ns = [su["n"] for su in sus]
    res["batch"] = {"solvers": S, "cap": cap, "n_median": float(np.median(ns)), "n_max": int(max(ns)),
                    "fused": row(ts["fused"]), "fused_device_events": row(ev), "earlier_path": row(ts["earlier"]),
                    "of_which_model_hypotheses_1thread": row(ts["model_hypotheses"]),
                    "earlier_over_fused": round(med(ts["earlier"]) / med(ts["fused"]), 2)}
    res["results_equal_model"] = True
    line = json.dumps(res)
    print(line)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
