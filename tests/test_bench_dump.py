"""bench.py --dump-outputs: `bench.dump_outputs` on host tensors shaped as the step's device
buffers (records past a frame's count filled with junk, as a reused buffer holds), read back
and compared with what went in; then the command line itself, as a CPU dry run and as a small
plain run on the GPU checked against the oracle."""
import numpy as np
import pytest
import torch

import bench
import orbslam_jpminipc_amd as orb
from orbslam_jpminipc_amd._native import KEYPOINT_DTYPE
from oracle_lib import Oracle

B, CAP = 5, 320


def _step_buffers():
    frames = orb.synth_stream(160, 120, stream=3, first=0, count=B)
    ora = Oracle(300, 1.2, 4, 1, 20)
    rng = np.random.default_rng(7)
    kps = rng.integers(0, 256, (B, CAP, 28), dtype=np.uint8)
    desc = rng.integers(0, 256, (B, CAP, 32), dtype=np.uint8)
    m12 = rng.integers(-1, CAP, (B - 1, CAP)).astype(np.int32)
    cnt = np.zeros(B, np.int32)
    ref = []
    for b in range(B):
        k, d = ora.extract(frames[b])
        cnt[b] = len(k)
        kps[b, : len(k)] = k.view(np.uint8).reshape(-1, 28)
        desc[b, : len(k)] = d
        ref.append((k, d))
    nm = rng.integers(0, 100, B - 1).astype(np.int32)
    f1 = np.arange(B - 1, dtype=np.int32)
    return ref, cnt, m12, nm, [torch.from_numpy(a) for a in (f1, kps, desc, cnt, m12, nm)]


def _load(d):
    return {p.stem: np.load(p) for p in sorted(d.iterdir())}


def test_dump_outputs_round_trip(tmp_path):
    ref, cnt, m12, nm, bufs = _step_buffers()
    assert 0 < cnt.min() and cnt.max() < CAP  # every frame has live records and junk slots
    bench.dump_outputs(str(tmp_path / "a"), *bufs)
    out = _load(tmp_path / "a")
    assert set(out) == {"counts", "nmatches", "frames", "pairs", "keypoints", "descriptors", "matches12"}
    assert all(a.dtype == np.float32 for a in out.values())
    assert sum(a.nbytes for a in out.values()) <= 64 << 20
    np.testing.assert_array_equal(out["counts"], cnt)
    np.testing.assert_array_equal(out["nmatches"], nm)
    np.testing.assert_array_equal(out["frames"], np.arange(B))  # the budget holds every frame here
    np.testing.assert_array_equal(out["pairs"], np.arange(B - 1))
    assert out["keypoints"].shape == (B, CAP, 7) and out["descriptors"].shape == (B, CAP, 32)
    for b, (k, d) in enumerate(ref):
        n = len(k)
        for j, f in enumerate(KEYPOINT_DTYPE.names):
            np.testing.assert_array_equal(out["keypoints"][b, :n, j], k[f].astype(np.float32))
        np.testing.assert_array_equal(out["descriptors"][b, :n], d)
        assert not out["keypoints"][b, n:].any() and not out["descriptors"][b, n:].any()
    for p in range(B - 1):
        np.testing.assert_array_equal(out["matches12"][p, : cnt[p]], m12[p, : cnt[p]])
        assert (out["matches12"][p, cnt[p]:] == -1).all()
    # the same arguments give the same files
    bench.dump_outputs(str(tmp_path / "b"), *bufs)
    again = _load(tmp_path / "b")
    assert all(out[k].tobytes() == again[k].tobytes() for k in out)


def test_dump_outputs_samples_within_budget(tmp_path, monkeypatch):
    """A budget that holds two frames: a fixed, sorted sample of frames and of pairs."""
    ref, cnt, m12, nm, bufs = _step_buffers()
    monkeypatch.setattr(bench, "DUMP_BYTES", 2 * CAP * 40 * 4)
    bench.dump_outputs(str(tmp_path / "a"), *bufs)
    bench.dump_outputs(str(tmp_path / "b"), *bufs)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert all(a[k].tobytes() == b[k].tobytes() for k in a)
    fr, pr = a["frames"].astype(int), a["pairs"].astype(int)
    assert len(fr) == 2 and len(pr) == 2 and fr[0] < fr[1] and pr[0] < pr[1]
    np.testing.assert_array_equal(a["counts"], cnt)  # counts and nmatches stay whole
    assert a["keypoints"].shape == (2, CAP, 7) and a["matches12"].shape == (2, CAP)
    for i, f in enumerate(fr):
        np.testing.assert_array_equal(a["descriptors"][i, : cnt[f]], ref[f][1])
    for i, p in enumerate(pr):
        np.testing.assert_array_equal(a["matches12"][i, : cnt[p]], m12[p, : cnt[p]])


def test_dry_run_dumps_last_step(tmp_path):
    """The command line: --dump-outputs DIR writes float32 arrays and the result line keeps
    ms_per_step for the --steps it was given."""
    import json
    import os
    import pathlib
    import subprocess
    import sys

    root = pathlib.Path(__file__).resolve().parent.parent
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, str(root / "bench.py"), "--gpus", "1", "--dry-run", "--steps", "3", "--warmup",
                        "0", "--dump-outputs", str(tmp_path / "out")], cwd=root, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    d = json.loads([l for l in r.stdout.decode().splitlines() if l.startswith("{")][-1])
    assert d["steps"] == 3 and d["ms_per_step"] * 3 == pytest.approx(d["rank_seconds"][0] * 1e3)
    out = _load(tmp_path / "out")
    assert all(a.dtype == np.float32 for a in out.values())
    n = int(out["counts"].sum())
    assert d["keypoints"] == 3 * n  # every step extracts the same frames
    assert out["keypoints"].shape == (n, 7) and out["descriptors"].shape == (n, 32)


@pytest.mark.gpu
def test_plain_run_on_gpu_dumps_the_step(tmp_path):
    """A plain `bench.py` run on the GPU (a small custom batch): the result line holds the headline
    figure without the --full sections, and the dumped keypoints, descriptors and vnMatches12 of
    the last timed step are the oracle's for the same frames, bit for bit."""
    import json
    import os
    import pathlib
    import subprocess
    import sys

    W, H, NF, N = 320, 240, 500, 4
    root = pathlib.Path(__file__).resolve().parent.parent
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, str(root / "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--batch", str(N), "--width", str(W), "--height", str(H), "--nfeatures", str(NF),
                        "--dump-outputs", str(tmp_path / "out")], cwd=root, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    d = json.loads([l for l in r.stdout.decode().splitlines() if l.startswith("{")][-1])
    assert d["steps"] == 2 and d["unit"] == "frames/s" and d["dtype"] == "u8" and d["higher_is_better"] is True
    assert d["value"] == pytest.approx(N / (d["ms_per_step"] * 1e-3))
    assert not {"roofline", "stages", "host_fed", "bow", "latency_b1", "cpu_baseline"} & set(d)
    out = _load(tmp_path / "out")
    assert all(a.dtype == np.float32 for a in out.values())
    np.testing.assert_array_equal(out["frames"], np.arange(N))
    np.testing.assert_array_equal(out["pairs"], np.arange(N - 1))
    frames = orb.synth_stream(W, H, stream=0, first=0, count=N)
    ora = Oracle(NF, 1.2, 8, 1, 20)
    ref = [ora.extract(f) for f in frames]
    for b, (k, dsc) in enumerate(ref):
        assert out["counts"][b] == len(k) > 0
        assert out["keypoints"][b, : len(k)].tobytes() == bench.keypoint_table(k).tobytes()
        np.testing.assert_array_equal(out["descriptors"][b, : len(k)], dsc)
    for p in range(N - 1):
        (k1, d1), (k2, d2) = ref[p], ref[p + 1]
        prev = np.ascontiguousarray(np.stack([k1["x"], k1["y"]], 1).astype(np.float32))
        n, m12 = ora.search_for_initialization(k1, d1, k2, d2, W, H, prev, 0.9, True, 100)
        assert out["nmatches"][p] == n
        np.testing.assert_array_equal(out["matches12"][p, : len(k1)], m12)
        assert (out["matches12"][p, len(k1):] == -1).all()
