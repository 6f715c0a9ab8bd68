#!/usr/bin/env python3
"""Time one whole Initializer::Initialize (--n-hyp iterations, then ReconstructH / ReconstructF) on
the GPU (csrc/orb_initializer.hip: orb_initializer_initialize, orb_initializer_initialize_batch_device)
against the path the same job took before the reconstruction moved to the device, in one run.
Reports only; gates nothing.

Measured, each after a warm-up as the median over --runs windows, by the host clock (both paths end
in a synchronise, and the earlier path has host work in it):
  fused        orb_initializer_initialize on one pair with N = 100, 300, 1000 matches (synthetic);
               orb_initializer_initialize_batch_device over the B - 1 consecutive pairs of a B-frame
               640x480 / 1000-keypoint batch matched on the device, the upload of the rand() values
               included;
  earlier path orb_initializer_ransac[_batch_device], the copy back of what Reconstruct* reads (the
               winners, use_h, the masks, and for the batch the keypoints and matches), then the C++
               model (tests/native/initializer_reconstruct_model.cpp, -O3, one thread).
The batch form is also timed by device events around the enqueued calls alone, and so is
orb_initializer_reconstruct_batch_device on its own.  Kernel time alone is not measured.
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
    ap.add_argument("--iters", type=int, default=20, help="calls per timed window (host call, device events)")
    ap.add_argument("--batch-iters", type=int, default=1, help="calls per timed window (batch)")
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()

    import torch

    import __graft_entry__ as ge

    if not torch.cuda.is_available():
        sys.exit("initializer_reconstruct_timing: no GPU; a time taken elsewhere says nothing")
    if not (ROOT / "orbslam_jpminipc_amd" / "liborb_hip.so").exists():
        ge.build()
    import initializer_reconstruct_model as model
    import orbslam_jpminipc_amd as orb
    from orbslam_jpminipc_amd._native import KEYPOINT_DTYPE
    from test_initializer_ransac_model import draws, two_view_case

    med = statistics.median
    n_hyp = a.n_hyp
    bound = float(np.load(ROOT / "tests" / "golden" / "initializer_reconstruct.npz")["parallax_bound"])
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

    def model_reconstruct(k1, k2, m12, f):
        use_h = bool(f["use_h"])
        return model.reconstruct(k1, k2, m12, f["H"] if use_h else f["F"], use_h,
                                 f["inliers_h"] if use_h else f["inliers_f"], K4)

    # ---- one pair, host buffers ----------------------------------------------------------------
    K4 = np.array([500.0, 500.0, 160.0, 120.0], np.float32)  # the camera of two_view_case
    for N in (100, 300, 1000):
        k1, k2, m12 = two_view_case(N)
        r = draws(n_hyp, N)
        got = init.initialize(k1, k2, m12, r, K4)
        with np.errstate(all="ignore"):
            model.same_reconstruction(got, model_reconstruct(k1, k2, m12, got), bound)
        found = init.find(k1, k2, m12, r)

        def earlier():
            return model_reconstruct(k1, k2, m12, init.find(k1, k2, m12, r))

        ts = timed({"fused": lambda: init.initialize(k1, k2, m12, r, K4), "earlier": earlier,
                    "model_reconstruct": lambda: model_reconstruct(k1, k2, m12, found)}, a.iters)
        res["host_call"][str(N)] = {"n_inliers": got["n_inliers"], "n_motion": got["n_motion"], "ok": got["ok"],
                                    "fused": row(ts["fused"]), "earlier_path": row(ts["earlier"]),
                                    "of_which_model_reconstruct_1thread": row(ts["model_reconstruct"]),
                                    "earlier_over_fused": round(med(ts["earlier"]) / med(ts["fused"]), 2)}

    # ---- the consecutive pairs of one 640x480 batch ---------------------------------------------
    W, H, B = 640, 480, a.frames
    P = B - 1
    K4 = np.array([500.0, 500.0, 320.0, 240.0], np.float32)
    frames = orb.synth_stream(W, H, stream=0, first=0, count=B)
    ext = orb.ORBextractor(1000, 1.2, 8, orb.FAST_SCORE, 20, device=0, max_batch=B)
    kps, desc, cnt = ext.extract_batch_device(torch.from_numpy(frames).cuda())
    f1 = torch.arange(0, P, dtype=torch.int32, device="cuda")
    f2 = f1 + 1
    m12, nm = orb.ORBmatcher(0.9, True).search_for_initialization_batch_device(kps, desc, cnt, f1, f2, W, H, 100)
    torch.cuda.synchronize()
    cap = int(kps.shape[1])
    r = np.random.default_rng(5).integers(0, 2 ** 31, (P, n_hyp, 8)).astype(np.int32)
    tc = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
    REC = ("ok", "R21", "t21", "P3D", "triangulated", "n_motion", "motion_R", "motion_t", "n_good", "cos_parallax",
           "parallax_deg", "best", "n_inliers")

    def fused():
        out = init.initialize_batch_device(kps, cnt, f1, f2, m12, tc(r), K4)
        torch.cuda.synchronize()
        return out

    def copy_back(found):
        h = {k: found[k].cpu().numpy() for k in ("best_H21", "best_F21", "use_h", "inliers_h", "inliers_f", "n_matches")}
        h["kps"] = kps.cpu().numpy().view(KEYPOINT_DTYPE).reshape(B, cap)
        h["cnt"], h["m12"] = cnt.cpu().numpy(), m12.cpu().numpy()
        return h

    def model_pair(h, p):
        n1, n = int(h["cnt"][p]), int(h["n_matches"][p])
        use_h = bool(h["use_h"][p])
        return model.reconstruct(h["kps"][p, :n1], h["kps"][p + 1, : h["cnt"][p + 1]], h["m12"][p, :n1],
                                 h["best_H21" if use_h else "best_F21"][p], use_h,
                                 h["inliers_h" if use_h else "inliers_f"][p, :n], K4)

    def earlier():
        h = copy_back(init.find_batch_device(kps, cnt, f1, f2, m12, tc(r), hypotheses=False))
        with np.errstate(all="ignore"):
            return [model_pair(h, p) for p in range(P)]

    full = fused()
    hb = copy_back(full)
    host = {k: full[k].cpu().numpy() for k in REC}
    oks = 0
    with np.errstate(all="ignore"):
        for p in range(P):  # every pair against the model, all fields
            n1 = int(hb["cnt"][p])
            got = dict(ok=bool(host["ok"][p]), R21=host["R21"][p].reshape(3, 3), t21=host["t21"][p], P3D=host["P3D"][p, :n1],
                       triangulated=host["triangulated"][p, :n1].astype(bool), n_motion=int(host["n_motion"][p]),
                       motion_R=host["motion_R"][p].reshape(8, 3, 3), motion_t=host["motion_t"][p].reshape(8, 3),
                       n_good=host["n_good"][p], cos_parallax=host["cos_parallax"][p], parallax_deg=host["parallax_deg"][p],
                       best=int(host["best"][p]), n_inliers=int(host["n_inliers"][p]))
            model.same_reconstruction(got, model_pair(hb, p), bound)
            oks += got["ok"]

    def model_all():
        with np.errstate(all="ignore"):
            return [model_pair(hb, p) for p in range(P)]

    ts = timed({"fused": fused, "earlier": earlier, "model_reconstruct": model_all}, a.batch_iters)
    d_r = tc(r)
    found = init.find_batch_device(kps, cnt, f1, f2, m12, d_r, hypotheses=False)

    def events(fn):
        ev = []
        fn()
        for _ in range(a.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                fn()
            e1.record()
            e1.synchronize()
            ev.append(e0.elapsed_time(e1) * 1e-3 / a.iters)
        return ev

    ev_all = events(lambda: init.initialize_batch_device(kps, cnt, f1, f2, m12, d_r, K4))
    ev_rec = events(lambda: init.reconstruct_batch_device(kps, cnt, f1, f2, m12, found, K4))
    h_nm, h_in = hb["n_matches"], host["n_inliers"]
    res["batch"] = {"pairs": P, "cap": cap, "n_median": float(np.median(h_nm)), "n_max": int(h_nm.max()),
                    "inliers_median": float(np.median(h_in)), "pairs_use_h": int(hb["use_h"].astype(bool).sum()),
                    "pairs_ok": int(oks), "fused": row(ts["fused"]), "fused_device_events": row(ev_all),
                    "reconstruct_only_device_events": row(ev_rec), "earlier_path": row(ts["earlier"]),
                    "of_which_model_reconstruct_1thread": row(ts["model_reconstruct"]),
                    "earlier_over_fused": round(med(ts["earlier"]) / med(ts["fused"]), 2)}
    res["results_equal_model"] = True
    res["not_measured"] = "kernel time alone (no profiler run)"
    line = json.dumps(res)
    print(line)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
