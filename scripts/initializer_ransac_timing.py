#!/usr/bin/env python3
"""Time one Initializer::Initialize up to RH (--n-hyp iterations) on the GPU
(csrc/orb_initializer.hip: orb_initializer_ransac, orb_initializer_ransac_batch_device) against the
path the same job took before the hypotheses moved to the device, in one run.  Reports only; gates
nothing.

Measured, each after a warm-up as the median over --runs windows, by the host clock (both paths end
in a synchronise, and the earlier path has host work in it):
  fused        orb_initializer_ransac on one pair with N = 100, 300, 1000 matches (synthetic);
               orb_initializer_ransac_batch_device over the B - 1 consecutive pairs of a B-frame
               640x480 / 1000-keypoint batch matched on the device, the upload of the rand() values
               included;
  earlier path the C++ model (tests/native/initializer_ransac_model.cpp, -O3, one thread) drawing
               the sets and computing the hypotheses, then orb_initializer_check[_batch_device] on
               them, their upload included.  For the batch the keypoints and matches are already on
               the host: the copy back that a caller would also pay is not charged.
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
    ap.add_argument("--n-hyp", type=int, default=200)
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20, help="calls per timed window (host call)")
    ap.add_argument("--batch-iters", type=int, default=1, help="calls per timed window (batch)")
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()

    import torch

    import __graft_entry__ as ge

    if not torch.cuda.is_available():
        sys.exit("initializer_ransac_timing: no GPU; a time taken elsewhere says nothing")
    if not (ROOT / "orbslam_jpminipc_amd" / "liborb_hip.so").exists():
        ge.build()
    import initializer_ransac_model as model
    import orbslam_jpminipc_amd as orb
    from orbslam_jpminipc_amd._native import KEYPOINT_DTYPE
    from test_initializer_ransac_model import draws, same_find, two_view_case

    med = statistics.median
    n_hyp = a.n_hyp
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

    init = orb.InitializerRansac(1.0, n_hyp)

    # ---- one pair, host buffers ----------------------------------------------------------------
    for N in (100, 300, 1000):
        k1, k2, m12 = two_view_case(N)
        r = draws(n_hyp, N)
        same_find(init.find(k1, k2, m12, r), model.find(k1, k2, m12, r))

        def earlier():
            h = model.hypotheses(k1, k2, m12, rand31=r)
            return init.check(k1, k2, m12, h["H21"], h["H12"], h["F21"])

        ts = timed({"fused": lambda: init.find(k1, k2, m12, r), "earlier": earlier,
                    "model_hypotheses": lambda: model.hypotheses(k1, k2, m12, rand31=r)}, a.iters)
        res["host_call"][str(N)] = {"fused": row(ts["fused"]), "earlier_path": row(ts["earlier"]),
                                    "of_which_model_hypotheses_1thread": row(ts["model_hypotheses"]),
                                    "earlier_over_fused": round(med(ts["earlier"]) / med(ts["fused"]), 2)}

    # ---- the consecutive pairs of one 640x480 batch ---------------------------------------------
    W, H, B = 640, 480, a.frames
    P = B - 1
    frames = orb.synth_stream(W, H, stream=0, first=0, count=B)
    ext = orb.ORBextractor(1000, 1.2, 8, orb.FAST_SCORE, 20, device=0, max_batch=B)
    kps, desc, cnt = ext.extract_batch_device(torch.from_numpy(frames).cuda())
    f1 = torch.arange(0, P, dtype=torch.int32, device="cuda")
    f2 = f1 + 1
    m12, nm = orb.ORBmatcher(0.9, True).search_for_initialization_batch_device(kps, desc, cnt, f1, f2, W, H, 100)
    torch.cuda.synchronize()
    cap = int(kps.shape[1])
    h_kps = kps.cpu().numpy().view(KEYPOINT_DTYPE).reshape(B, cap)
    h_cnt, h_m12, h_nm = cnt.cpu().numpy(), m12.cpu().numpy(), nm.cpu().numpy()
    r = np.random.default_rng(5).integers(0, 2 ** 31, (P, n_hyp, 8)).astype(np.int32)
    tc = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731

    def fused():
        out = init.find_batch_device(kps, cnt, f1, f2, m12, tc(r), hypotheses=False)
        torch.cuda.synchronize()
        return out

    hyp = {k: np.zeros((P, n_hyp, 9), np.float32) for k in ("H21", "H12", "F21")}

    def model_hypotheses():
        for p in range(P):
            h = model.hypotheses(h_kps[p, : h_cnt[p]], h_kps[p + 1, : h_cnt[p + 1]], h_m12[p, : h_cnt[p]], rand31=r[p])
            for k in hyp:
                hyp[k][p] = h[k]

    def earlier():
        model_hypotheses()
        out = init.check_batch_device(kps, cnt, f1, f2, m12, tc(hyp["H21"]), tc(hyp["H12"]), tc(hyp["F21"]))
        torch.cuda.synchronize()
        return out

    full = {k: v.cpu().numpy() for k, v in init.find_batch_device(kps, cnt, f1, f2, m12, tc(r)).items()}
    for p in range(0, P, max(1, P // 16)):  # a sample of the pairs against the model, all fields
        want = model.find(h_kps[p, : h_cnt[p]], h_kps[p + 1, : h_cnt[p + 1]], h_m12[p, : h_cnt[p]], r[p])
        n = int(full["n_matches"][p])
        got = {"n_matches": n, "sets": full["sets"][p], "H": full["best_H21"][p].reshape(3, 3),
               "F": full["best_F21"][p].reshape(3, 3), "RH": full["RH"][p], "use_h": bool(full["use_h"][p])}
        for k in ("H21", "H12", "F21"):
            got[k] = full[k][p]
        for t in "hf":
            got.update({"scores_" + t: full["scores_" + t][p], "best_" + t: int(full["best_" + t][p]),
                        "best_score_" + t: full["best_score_" + t][p],
                        "inliers_" + t: full["inliers_" + t][p, :n].astype(bool)})
        same_find(got, want)
    ts = timed({"fused": fused, "earlier": earlier, "model_hypotheses": model_hypotheses}, a.batch_iters)
    d_r = tc(r)
    ev = []
    for _ in range(a.runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            init.find_batch_device(kps, cnt, f1, f2, m12, d_r, hypotheses=False)
        e1.record()
        e1.synchronize()
        ev.append(e0.elapsed_time(e1) * 1e-3 / a.iters)
    res["batch"] = {"pairs": P, "cap": cap, "n_median": float(np.median(h_nm)), "n_max": int(h_nm.max()),
                    "pairs_below_8": int((h_nm < 8).sum()), "fused": row(ts["fused"]), "fused_device_events": row(ev),
                    "earlier_path": row(ts["earlier"]), "of_which_model_hypotheses_1thread": row(ts["model_hypotheses"]),
                    "earlier_over_fused": round(med(ts["earlier"]) / med(ts["fused"]), 2)}
    res["results_equal_model"] = True
    line = json.dumps(res)
    print(line)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
