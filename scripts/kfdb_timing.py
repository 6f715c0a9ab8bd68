#!/usr/bin/env python3
"""Time the KeyFrameDatabase relocalisation query (csrc/orb_kfdb.hip) on the GPU against a
single-threaded CPU inverted file (tests/native/kfdb_baseline.cpp, -O3), in one run.

Workload: --keyframes keyframes of about --words words over a --vocab-words vocabulary, laid out
as places (keyframes of a place draw from that place's word pool, so neighbours share a few
hundred words, as keyframes of one room do); 64 queries, each near one place; ten covisible
neighbours per keyframe.

Measured: Q = 1, the host entry point (host clock around the synchronous call), and Q = 64, the
device batch entry point (device events around the enqueued work); after a warm-up, the median
over --runs repeated windows.  Before anything is timed the candidate lists of both paths are
compared with the baseline's, query by query, from the same fresh state.

Derived, not measured: "pool GB/s" is the live entry pool (12 B per entry) divided by the time
per query, i.e. the rate at which a query passes over the pool wherever the pool then sits (at
this size it fits the caches), and its share of the 8 TB/s HBM peak.

Prints one JSON line; --out also writes it to a file."""
import argparse
import ctypes
import json
import pathlib
import statistics
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def workload(rng, n_kf, n_words_kf, vocab, n_queries):
    places = max(1, n_kf // 32)
    pool_size = int(n_words_kf * 2.5)
    pools = [np.sort(rng.choice(vocab, pool_size, replace=False)) for _ in range(places)]

    def draw(p, n):
        w = np.sort(rng.choice(pools[p], n, replace=False)).astype(np.uint32)
        v = rng.random(n) + 1e-3
        return w, v / v.sum()

    kfs = [draw(k % places, int(rng.integers(n_words_kf * 3 // 4, n_words_kf * 5 // 4 + 1))) for k in range(n_kf)]
    cov = [[(k + d * places) % n_kf for d in (1, -1, 2, -2, 3, -3, 4, -4, 5, -5)] for k in range(n_kf)]
    queries = [draw(int(rng.integers(0, places)), n_words_kf) for _ in range(n_queries)]
    return kfs, cov, queries


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=2048)
    ap.add_argument("--words", type=int, default=800)
    ap.add_argument("--vocab-words", type=int, default=10**6)
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20, help="passes over the queries per timed window")
    ap.add_argument("--baseline-iters", type=int, default=2)
    ap.add_argument("--row-cap", type=int, default=0,
                    help="row capacity of the batched query layout (0: the longest query)")
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()

    import torch

    import __graft_entry__ as ge
    import orbslam_jpminipc_amd as orb
    from orbslam_jpminipc_amd._native import check, ptr

    if not torch.cuda.is_available():
        sys.exit("kfdb_timing: no GPU; a time taken elsewhere says nothing")
    ge.build()
    base = ctypes.CDLL(str(ROOT / "build" / "libkfdb_baseline.so"))
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    base.kfb_create.restype = vp
    base.kfb_create.argtypes = [i32]
    base.kfb_destroy.argtypes = [vp]
    base.kfb_add.argtypes = [vp, i32, vp, vp, i32]
    base.kfb_set_covisible.argtypes = [vp, i32, vp, i32]
    base.kfb_reloc.restype = i32
    base.kfb_reloc.argtypes = [vp, vp, vp, i32, vp, i32]

    rng = np.random.default_rng(2024)
    N, V, Q = a.keyframes, a.vocab_words, a.queries
    kfs, cov, queries = workload(rng, N, a.words, V, Q)
    entries = sum(len(w) for w, _ in kfs)
    voc = orb.ORBVocabulary.from_arrays(10, 1, 0, 0, np.zeros(V, np.int32), np.ones(V, np.uint8),
                                        np.zeros((V, 32), np.uint8), np.ones(V, np.float64))
    lib = orb.hip_lib()

    def fresh_device():
        db = orb.KeyFrameDatabase(voc, N, entries)
        for k, (w, v) in enumerate(kfs):
            db.add(k, (w, v))  # id k gets slot k
        for k in range(N):
            db.set_covisible(k, cov[k])
        return db

    def fresh_baseline():
        h = base.kfb_create(V)
        for k, (w, v) in enumerate(kfs):
            base.kfb_add(h, k, ptr(w), ptr(v), len(w))
        for k in range(N):
            nb = np.array(cov[k], np.int32)
            base.kfb_set_covisible(h, k, ptr(nb), len(nb))
        return h

    out = np.zeros(N, np.int32)
    n_out = ctypes.c_int()

    def host_query(db, q):
        w, v = q
        check(lib.orb_kfdb_detect_relocalisation_candidates(db._h, ptr(w), ptr(v), len(w), ptr(out), N,
                                                            ctypes.byref(n_out)))
        return out[: n_out.value].tolist()

    def base_query(h, q):
        w, v = q
        n = base.kfb_reloc(h, ptr(w), ptr(v), len(w), ptr(out), N)
        return out[:n].tolist()

    cap = max(a.row_cap, max(len(w) for w, _ in queries))
    bw = np.zeros((Q, cap), np.uint32)
    bv = np.zeros((Q, cap), np.float64)
    bn = np.zeros(Q, np.int32)
    for i, (w, v) in enumerate(queries):
        bw[i, : len(w)], bv[i, : len(w)], bn[i] = w, v, len(w)
    d_w, d_v, d_n = (torch.from_numpy(x).cuda() for x in (bw.view(np.int32), bv, bn))

    # ---- the same candidates, from the same fresh state --------------------------------------
    hb = fresh_baseline()
    expect = [base_query(hb, q) for q in queries]
    dev1 = fresh_device()
    got1 = [host_query(dev1, q) for q in queries]
    devq = fresh_device()
    slots, cnt = devq.detect_relocalisation_candidates_batch_device(d_w, d_v, d_n, out_cap=64)
    torch.cuda.synchronize()
    slots, cnt = slots.cpu().numpy(), cnt.cpu().numpy()
    gotq = [slots[i, : cnt[i]].tolist() for i in range(Q)]
    assert cnt.max() <= 64
    if got1 != expect or gotq != expect:
        bad = [i for i in range(Q) if got1[i] != expect[i] or gotq[i] != expect[i]]
        sys.exit(f"kfdb_timing: candidate lists differ from the baseline at queries {bad[:8]}")
    n_cand = sum(len(e) for e in expect)

    # ---- timing ------------------------------------------------------------------------------
    for q in queries:  # warm-up of every shape the windows use
        host_query(dev1, q)
    for _ in range(3):
        devq.detect_relocalisation_candidates_batch_device(d_w, d_v, d_n, out_cap=64)
    torch.cuda.synchronize()
    t_host, t_batch, t_base = [], [], []
    for _ in range(a.runs):
        t0 = time.perf_counter()
        for _ in range(a.iters):
            for q in queries:
                host_query(dev1, q)  # synchronous: returns after the device is done
        t_host.append((time.perf_counter() - t0) / (a.iters * Q))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            devq.detect_relocalisation_candidates_batch_device(d_w, d_v, d_n, out_cap=64)
        e1.record()
        e1.synchronize()
        t_batch.append(e0.elapsed_time(e1) * 1e-3 / (a.iters * Q))
        t0 = time.perf_counter()
        for _ in range(a.baseline_iters):
            for q in queries:
                base_query(hb, q)
        t_base.append((time.perf_counter() - t0) / (a.baseline_iters * Q))
    base.kfb_destroy(hb)

    pool_bytes = entries * 12
    med = statistics.median

    def row(ts):
        t = med(ts)
        return {"us_per_query": round(t * 1e6, 2), "min_us": round(min(ts) * 1e6, 2), "max_us": round(max(ts) * 1e6, 2),
                "pool_GBps": round(pool_bytes / t / 1e9, 1), "share_of_8TBps": round(pool_bytes / t / 8e12, 4)}

    res = {
        "workload": {"keyframes": N, "words_per_keyframe": a.words, "vocab_words": V, "queries": Q,
                     "pool_entries": entries, "pool_bytes": pool_bytes, "candidates_total": n_cand,
                     "batch_row_cap": cap},
        "device": torch.cuda.get_device_name(0), "runs": a.runs, "iters": a.iters,
        "candidates_equal_baseline": True,
        "gpu_host_call_q1": row(t_host),
        "gpu_device_batch_q64": row(t_batch),
        "cpu_inverted_file_1thread": {"us_per_query": round(med(t_base) * 1e6, 2),
                                      "min_us": round(min(t_base) * 1e6, 2), "max_us": round(max(t_base) * 1e6, 2)},
    }
    line = json.dumps(res)
    print(line)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
