#!/usr/bin/env python3
"""Timing of the local map (orb_local_map_reference and its batch form) against a
single-threaded std::map restatement on the CPU (tests/native/local_map_baseline.cpp, -O3, the same host,
the same run).  A map of 2000 keyframes x 1000 keypoints over 100000 points; a frame of 1000 slots holds
points of five adjacent keyframes, which about 60 keyframes observe.  The results are compared with the
Python model (the single frame and the batch's first frames) and with the baseline (every frame) first;
then medians of 7: the host clock around the synchronous call for one frame, device events around the
batch of 512, the host clock around the baseline for one frame and for the 512 in a loop.  Prints one
JSON line; the raw line is kept in profiles/localmap/local_map_timing.json.

Not measured: the flattening of a live map into the tables (the caller's, once per map change, not per
frame), and the reference's mutex traffic."""
from __future__ import annotations

import ctypes
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import local_map_model as lm  # noqa: E402
import local_map_scenes as sc  # noqa: E402

N_KF, N_PT, ROW, WINDOW, SLOTS, BATCH, REPEATS = 2000, 100000, 1000, 1500, 1000, 512, 7


class Baseline:
    def __init__(self, a, n_kf, n_pt):
        self.lib = ctypes.CDLL(str(ROOT / "build" / "liblocal_map_baseline.so"))
        self.lib.local_map_baseline_create.restype = ctypes.c_void_p
        p = lambda x: ctypes.c_void_p(x.ctypes.data)  # noqa: E731
        self.w = ctypes.c_void_p(self.lib.local_map_baseline_create(
            n_kf, n_pt, p(a["kf_bad"]), p(a["kf_mp_off"]), p(a["kf_mp"]), p(a["kf_cov"]), p(a["pt_bad"]),
            p(a["pt_obs_off"]), p(a["pt_obs_kf"])))
        self.n_kf, self.n_pt = n_kf, n_pt
        self.kf, self.pt = np.zeros(n_kf, np.int32), np.zeros(n_pt, np.int32)
        self.seen, self.out = np.zeros(n_pt, np.uint8), np.zeros(6, np.int32)

    def run(self, f_mp, f_out):
        p = lambda x: ctypes.c_void_p(x.ctypes.data)  # noqa: E731
        self.lib.local_map_baseline_reference(self.w, len(f_mp), p(f_mp), p(f_out), self.n_kf, p(self.kf), self.n_pt,
                                              p(self.pt), p(self.seen), p(self.out))
        return self.out


def median_ms(samples):
    return 1e3 * float(np.median(samples))


def main():
    import torch

    import orbslam_jpminipc_amd as orb

    T = sc.random_map(11, N_KF, N_PT, ROW, p_null=0.2, p_kf_bad=0.02, p_pt_bad=0.02, window=WINDOW)
    a = T.arrays()
    mt = orb.MapTables(**a)
    dt = mt.to("cuda")
    L = orb.LocalMap(0)
    frames = np.stack([np.int32(sc.random_frame(100 + b, T, SLOTS, around=(37 * b) % N_KF)) for b in range(BATCH)])
    base = Baseline(a, N_KF, N_PT)
    f_out = np.zeros(SLOTS, np.int32)
    rec = ("n_voted", "n_local_kf", "ref_kf", "ref_votes", "n_local_pt", "n_cleared")

    # results first: the host form against the model and the baseline ...
    got = L.reference(mt, frames[0], votes=True)
    want = lm.local_map_reference(T, frames[0])
    for k in rec + ("f_mp_out", "local_kf", "local_pt", "local_pt_seen", "kf_votes"):
        assert np.asarray(got[k]).tolist() == (want[k] if isinstance(want[k], int) else list(want[k])), k
    # ... and the batch against both
    cap_kf, cap_pt = 128, 32768
    d_f, d_n = torch.from_numpy(frames).cuda(), torch.full((BATCH,), SLOTS, dtype=torch.int32, device="cuda")
    out = L.reference_batch_device(dt, d_f, d_n, cap_kf, cap_pt)
    torch.cuda.synchronize()
    h = {k: v.cpu().numpy() for k, v in out.items()}
    assert (h["info"][:, 0] == 0).all(), h["info"][:, 0]
    voted = []
    for b in range(BATCH):
        o = base.run(frames[b], f_out)
        assert h["info"][b, 1:].tolist() == o.tolist(), b
        nk, npt = int(o[1]), int(o[4])
        assert h["local_kf"][b, :nk].tolist() == base.kf[:nk].tolist(), b
        assert h["local_pt"][b, :npt].tolist() == base.pt[:npt].tolist(), b
        assert h["local_pt_seen"][b, :npt].tolist() == base.seen[:npt].tolist(), b
        assert h["f_mp_out"][b].tolist() == f_out.tolist(), b
        voted.append(int(o[0]))
        if b < 4:
            w = lm.local_map_reference(T, frames[b])
            assert h["local_pt"][b, :npt].tolist() == w["local_pt"] and h["local_kf"][b, :nk].tolist() == w["local_kf"], b

    one_gpu, one_cpu, batch_gpu, batch_cpu = [], [], [], []
    for _ in range(REPEATS):
        t = time.perf_counter()
        L.reference(mt, frames[0])
        one_gpu.append(time.perf_counter() - t)
        t = time.perf_counter()
        base.run(frames[0], f_out)
        one_cpu.append(time.perf_counter() - t)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        L.reference_batch_device(dt, d_f, d_n, cap_kf, cap_pt, out=out)
        e1.record()
        e1.synchronize()
        batch_gpu.append(e0.elapsed_time(e1) * 1e-3)
        t = time.perf_counter()
        for b in range(BATCH):
            base.run(frames[b], f_out)
        batch_cpu.append(time.perf_counter() - t)
    table_bytes = int(sum(v.nbytes for v in a.values()))
    print(json.dumps({"local_map_timing": {
        "keyframes": N_KF, "points": N_PT, "keypoints_per_keyframe": ROW, "frame_slots": SLOTS, "table_bytes": table_bytes,
        "voted_median": float(np.median(voted)), "local_kf_median": float(np.median(h["info"][:, 2])),
        "local_pt_median": float(np.median(h["info"][:, 5])),
        "one_frame": {"gpu_host_call_ms": median_ms(one_gpu), "cpu_ms": median_ms(one_cpu),
                      "cpu_over_gpu": float(np.median(one_cpu) / np.median(one_gpu))},
        "batch_512": {"gpu_events_ms": median_ms(batch_gpu), "cpu_loop_ms": median_ms(batch_cpu),
                      "cpu_over_gpu": float(np.median(batch_cpu) / np.median(batch_gpu))},
        "repeats": REPEATS}}))


if __name__ == "__main__":
    main()
