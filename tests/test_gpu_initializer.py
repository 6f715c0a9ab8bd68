"""orb_initializer_check / orb_initializer_check_batch_device (csrc/orb_initializer.hip) against
the CPU model of Initializer::CheckHomography / CheckFundamental and the best-of loops
(tests/initializer_model.py): scores bitwise (as "is NaN" where the model's score is NaN), best
indices, best scores and inlier masks equal."""
import pathlib
import struct
import subprocess

import numpy as np
import pytest

import initializer_model as model
import orbslam_jpminipc_amd as orb
from orbslam_jpminipc_amd._native import KEYPOINT_DTYPE, ORB_EINVAL, ORB_ENOTSUP, OrbError
from test_initializer_model import I3, golden_as_result, golden_inputs

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parents[1]
f32 = np.float32
CHUNK = 16  # IN_CHUNK of csrc/orb_initializer.hip: matches per pipeline step (two buffers alternate)


def _kps(xy):
    k = np.zeros(len(xy), KEYPOINT_DTYPE)
    k["x"], k["y"] = xy[:, 0], xy[:, 1]
    k["size"], k["angle"], k["class_id"] = 31.0, -1.0, -1
    return k


def _skew(e):
    return np.array([[0, -e[2], e[1]], [e[2], 0, -e[0]], [-e[1], e[0], 0]], np.float64)


def synth_case(N, n_hyp, n1=None, n2=None, seed=0):
    """A pair with N matches among n1 / n2 keypoints (holes of -1, frame-2 indices shuffled):
    frame 2 = a homography of frame 1 plus pixel noise, hypotheses = that homography perturbed (and
    [e]x H for a random epipole), so that inliers, outliers and scores vary across hypotheses."""
    rng = np.random.default_rng(1000 * N + n_hyp + seed)
    n1 = n1 if n1 is not None else N + N // 2 + 3
    n2 = n2 if n2 is not None else N + 5
    x1 = (rng.random((n1, 2)) * [320, 240]).astype(f32)
    x2 = (rng.random((n2, 2)) * [320, 240]).astype(f32)
    Ht = np.array([[1.01, 0.02, 3.0], [-0.015, 0.99, -2.0], [1e-5, -2e-5, 1.0]])
    m12 = np.full(n1, -1, np.int32)
    src = np.sort(rng.choice(n1, N, replace=False))
    dst = rng.choice(n2, N, replace=False)
    m12[src] = dst
    p = np.c_[x1[src].astype(np.float64), np.ones(N)] @ Ht.T
    x2[dst] = (p[:, :2] / p[:, 2:] + rng.normal(0, 1.2, (N, 2))).astype(f32)
    H21 = np.zeros((n_hyp, 3, 3), f32)
    H12 = np.zeros_like(H21)
    F21 = np.zeros_like(H21)
    for h in range(n_hyp):
        Hh = Ht + rng.normal(0, 1, (3, 3)) * [[2e-3, 2e-3, 0.5], [2e-3, 2e-3, 0.5], [2e-6, 2e-6, 0]]
        H21[h] = Hh
        H12[h] = np.linalg.inv(Hh)
        F = _skew(np.r_[rng.normal(0, 300, 2), 1.0]) @ Hh
        F21[h] = F / np.abs(F).max()
    return _kps(x1), _kps(x2), m12, H21.reshape(n_hyp, 9), H12.reshape(n_hyp, 9), F21.reshape(n_hyp, 9)


def run_host(k1, k2, m12, H21, H12, F21, sigma=1.0):
    got = orb.Initializer(sigma).check(k1, k2, m12, H21, H12, F21)
    want = model.check(k1, k2, m12, sigma, H21, H12, F21)
    model.same_result(got, want)
    if want["RH"] is not None and not np.isnan(want["RH"]):
        assert f32(got["RH"]).tobytes() == f32(want["RH"]).tobytes()
    return got, want


def test_golden_fixture():
    k1, k2, m12, g = golden_inputs()
    got, want = run_host(k1, k2, m12, g["H21"], g["H12"], g["F21"], float(g["sigma"]))
    model.same_result(got, golden_as_result(g))
    assert got["best_h"] >= 0 and got["best_f"] >= 0


N_CASES = [0, 1, 7, 8, 63, 64, 65, 127, 128, 129, 257, 1000, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK,
           2 * CHUNK + 1]


@pytest.mark.parametrize("N", N_CASES)
def test_match_counts(N):
    got, want = run_host(*synth_case(N, 65))
    assert want["n_matches"] == N
    if N >= 8:  # the data is not degenerate: hypotheses differ, some matches are in and some out
        assert len(set(want["scores_h"].tolist())) > 1 and want["best_h"] >= 0 and want["best_f"] >= 0
    if N >= 63:
        assert 0 < want["inliers_h"].sum() < N and 0 < want["inliers_f"].sum() < N


@pytest.mark.parametrize("n_hyp", [1, 63, 64, 65, 200, 1024])
def test_hypothesis_counts(n_hyp):
    run_host(*synth_case(129, n_hyp))


@pytest.mark.parametrize("N,n1,n2", [(300, 319, 400), (300, 320, 300), (300, 321, 1000), (200, 256, 200),
                                     (200, 257, 203), (640, 641, 700), (5, 2000, 9), (8192, 8192, 8192)])
def test_keypoint_counts_and_holes(N, n1, n2):
    """n1 around the compaction strides of both kernels (320 and 256 threads), n1 != n2, sparse
    matches in a long frame, and the largest frame the entry point takes."""
    k1, k2, m12, H21, H12, F21 = synth_case(N, 65 if N < 8192 else 3, n1, n2)
    assert (m12 < 0).sum() == n1 - N
    got, want = run_host(k1, k2, m12, H21, H12, F21)
    assert want["n_matches"] == N


def test_staging_reuse_across_sizes():
    """One thread, one context: a small call, one large enough to grow the device arena and the pinned
    staging, a small one again and a pair without keypoints, each against the model; n1 != n2 and both
    below the larger, so the padding between a frame's count and the capacity is read."""
    for N, n_hyp, n1, n2 in [(40, 1, 65, 50), (100, 65, 110, 130), (1, 1, 1, 3)]:
        got, want = run_host(*synth_case(N, n_hyp, n1, n2))
        assert want["n_matches"] == N
    e, h = np.zeros(0, KEYPOINT_DTYPE), np.zeros((1, 9), f32)
    got, want = run_host(e, e, np.zeros(0, np.int32), h, h, h)
    assert want["n_matches"] == 0


def test_sigma():
    k1, k2, m12, H21, H12, F21 = synth_case(129, 65)
    a, _ = run_host(k1, k2, m12, H21, H12, F21, 0.7)
    b, _ = run_host(k1, k2, m12, H21, H12, F21, 2.5)
    assert a["scores_h"].tobytes() != b["scores_h"].tobytes()


def test_summation_order_is_visible_in_the_data():
    """The comparison above can tell a wrong add order: for most hypotheses a pairwise float32
    sum of the model's terms differs from its sequential sum."""
    k1, k2, m12, H21, H12, F21 = synth_case(257, 65)
    r = model.check(k1, k2, m12, 1.0, H21, H12, F21, terms=True)
    for t in "hf":
        differ = 0
        for h in range(65):
            v = r["terms_" + t][h].astype(f32)
            while len(v) > 1:
                if len(v) & 1:
                    v = np.concatenate([v, np.zeros(1, f32)])
                v = (v[0::2] + v[1::2]).astype(f32)
            differ += v[0].tobytes() != r["scores_" + t][h].tobytes()
        assert differ >= 10, (t, differ)


def test_identical_hypotheses_first_wins():
    k1, k2, m12, H21, H12, F21 = synth_case(129, 8)
    got, want = run_host(k1, k2, m12, H21, H12, F21)
    b = want["best_h"]
    # the winner repeated at the front, the back, and in another tile of 64
    for at in (0, 7):
        order = [b] * 2 + list(range(8)) if at == 0 else list(range(8)) + [b] * 2
        g2, w2 = run_host(k1, k2, m12, H21[order], H12[order], F21[order])
        assert w2["best_h"] == order.index(b) == g2["best_h"]
    order = [(b + 1) % 8] * 70 + [b] + [(b + 1) % 8] * 70 + [b]
    g2, w2 = run_host(k1, k2, m12, H21[order], H12[order], F21[order])
    assert g2["best_h"] == 70 == w2["best_h"]
    # equal maxima 256 and 512 apart (one thread of the 256-thread selection meets all three), and
    # a later one in a lower lane
    o = (b + 1) % 8
    for n, at in ((600, (266, 522)), (600, (10, 266, 522)), (400, (300, 390)), (1024, (1023,))):
        order = np.full(n, o)
        order[list(at)] = b
        g2, w2 = run_host(k1, k2, m12, H21[order], H12[order], F21[order])
        assert g2["best_h"] == at[0] == w2["best_h"]


def test_all_zero_scores():
    k1, k2, m12, H21, H12, F21 = synth_case(129, 65)
    k2 = k2.copy()
    k2["x"] += 5000.0  # every point far from every prediction ...
    F21 = np.stack([I3[0] * f32(h + 1) for h in range(65)])  # ... and from every line s * (u1, v1, 1)
    got, want = run_host(k1, k2, m12, H21, H12, F21)
    for t in "hf":
        assert want["best_" + t] == -1 and got["best_" + t] == -1 and got["best_score_" + t] == 0
        assert not got["inliers_" + t].any() and len(got["inliers_" + t]) == 129
        assert not got["scores_" + t].any()


@pytest.mark.parametrize("bad_first", [True, False])
@pytest.mark.parametrize("kind", ["inf", "nan"])
def test_homography_infinity_and_nan(kind, bad_first):
    k1, k2, m12, H21, H12, F21 = synth_case(129, 3)
    bad = np.array([1, 0, 0, 0, 1, 0, 0, 0, 0], f32) if kind == "inf" else np.zeros(9, f32)
    at = 0 if bad_first else 2
    H21, H12 = H21.copy(), H12.copy()
    H21[at] = H12[at] = bad
    got, want = run_host(k1, k2, m12, H21, H12, None)
    if kind == "nan":
        assert np.isnan(want["scores_h"][at]) and np.isnan(got["scores_h"][at])
    else:
        assert want["scores_h"][at] == 0
    assert want["best_h"] != at and want["best_h"] >= 0
    # the degenerate hypothesis alone: nothing wins
    got, want = run_host(k1, k2, m12, bad[None], bad[None], None)
    assert got["best_h"] == -1 and got["best_score_h"] == 0 and not got["inliers_h"].any()


@pytest.mark.parametrize("at", [0, 2])
def test_fundamental_of_zeros(at):
    k1, k2, m12, H21, H12, F21 = synth_case(129, 3)
    F21 = F21.copy()
    F21[at] = 0
    got, want = run_host(k1, k2, m12, None, None, F21)
    assert np.isnan(want["scores_f"][at]) and np.isnan(got["scores_f"][at])
    assert want["best_f"] != at and want["best_f"] >= 0
    got, want = run_host(k1, k2, m12, None, None, np.zeros((1, 9), f32))
    assert got["best_f"] == -1 and got["best_score_f"] == 0 and not got["inliers_f"].any()


def test_one_model_only():
    k1, k2, m12, H21, H12, F21 = synth_case(129, 65)
    both, _ = run_host(k1, k2, m12, H21, H12, F21)
    h, _ = run_host(k1, k2, m12, H21, H12, None)
    f, _ = run_host(k1, k2, m12, None, None, F21)
    assert "scores_f" not in h and "scores_h" not in f and h["RH"] is None and f["RH"] is None
    assert h["n_matches"] == f["n_matches"] == 129
    model.same_result(h, {k: v for k, v in both.items() if not k.endswith("_f")})
    model.same_result(f, {k: v for k, v in both.items() if not k.endswith("_h")})


def test_refusals():
    k1, k2, m12, H21, H12, F21 = synth_case(20, 4)
    init = orb.Initializer()
    for i, v in ((3, len(k2)), (0, -2), (len(m12) - 1, 1 << 30)):
        bad = m12.copy()
        bad[i] = v
        with pytest.raises(OrbError) as e:
            init.check(k1, k2, bad, H21, H12, F21)
        assert e.value.code == ORB_EINVAL and "matches12" in str(e.value)
    for n in (0, 1025):
        Z = np.tile(I3, (n, 1)).reshape(n, 9)
        with pytest.raises(OrbError) as e:
            init.check(k1, k2, m12, Z, Z, Z)
        assert e.value.code in (ORB_EINVAL, ORB_ENOTSUP) and "n_hyp" in str(e.value)
    with pytest.raises(OrbError) as e:  # neither model
        init.check(k1, k2, m12, None, None, None)
    assert e.value.code == ORB_EINVAL
    big = np.zeros(8193, KEYPOINT_DTYPE)
    with pytest.raises(OrbError) as e:
        init.check(big, k2, np.full(8193, -1, np.int32), H21, H12, F21)
    assert e.value.code == ORB_ENOTSUP
    # the call after a refusal is served
    run_host(k1, k2, m12, H21, H12, F21)


# ---- batched, on device-resident extractor and matcher output ---------------------------------

@pytest.fixture(scope="module")
def batch():
    """3 frames of 320x240 (the third flat: no keypoints), pairs (0,1), (1,2), (1,1), matched on
    the device; hypotheses per pair from synth_case (any values serve)."""
    import torch

    W, H = 320, 240
    frames = orb.synth_stream(W, H, stream=7, first=0, count=3).copy()
    frames[2] = orb.synth_special(orb.SYN_FLAT, W, H)
    ext = orb.ORBextractor(500, 1.2, 8, orb.FAST_SCORE, 20, device=0, max_batch=3)
    kps, desc, cnt = ext.extract_batch_device(torch.from_numpy(frames).cuda())
    f1 = torch.tensor([0, 1, 1], dtype=torch.int32, device="cuda")
    f2 = torch.tensor([1, 2, 1], dtype=torch.int32, device="cuda")
    m12, nm = orb.ORBmatcher(0.9, True).search_for_initialization_batch_device(kps, desc, cnt, f1, f2, W, H, 100)
    torch.cuda.synchronize()
    n_hyp = 65
    hyp = [synth_case(40 + p, n_hyp)[3:] for p in range(3)]
    H21, H12, F21 = (np.stack([h[k] for h in hyp]) for k in range(3))
    # pair (1,1) matches every keypoint with itself: the identity must win there
    H21[2, 5] = H12[2, 5] = I3[0]
    return dict(kps=kps, cnt=cnt, f1=f1, f2=f2, m12=m12, nm=nm.cpu().numpy(), H21=H21, H12=H12, F21=F21)


def _batch_vs_host_and_model(b, d_m12, host_m12):
    import torch

    P, cap = d_m12.shape
    kps = b["kps"].cpu().numpy().view(KEYPOINT_DTYPE).reshape(3, cap)
    cnt = b["cnt"].cpu().numpy()
    dev = [torch.from_numpy(b[k]).cuda() for k in ("H21", "H12", "F21")]
    out = orb.Initializer(1.0).check_batch_device(b["kps"], b["cnt"], b["f1"], b["f2"], d_m12, *dev)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    results = []
    for p, (a, c) in enumerate(zip(b["f1"].tolist(), b["f2"].tolist())):
        k1, k2 = kps[a, : cnt[a]], kps[c, : cnt[c]]
        m = host_m12[p, : cnt[a]]
        n = int(out["n_matches"][p])
        got = {"n_matches": n}
        for t in "hf":
            got.update({"scores_" + t: out["scores_" + t][p], "best_" + t: int(out["best_" + t][p]),
                        "best_score_" + t: out["best_score_" + t][p],
                        "inliers_" + t: out["inliers_" + t][p, :n].astype(bool)})
            assert not out["inliers_" + t][p, n:].any()
        host = orb.Initializer(1.0).check(k1, k2, m, b["H21"][p], b["H12"][p], b["F21"][p])
        want = model.check(k1, k2, m, 1.0, b["H21"][p], b["H12"][p], b["F21"][p])
        model.same_result(got, host)
        model.same_result(got, want)
        results.append(got)
    return results


def test_batch_equals_host_and_model(batch):
    m12 = batch["m12"].cpu().numpy()
    cnt = batch["cnt"].cpu().numpy()
    assert cnt[2] == 0 and batch["nm"][1] == 0 and batch["nm"][0] > 0 and batch["nm"][2] > 0
    res = _batch_vs_host_and_model(batch, batch["m12"], m12)
    assert [r["n_matches"] for r in res] == batch["nm"].tolist()
    assert res[1]["best_h"] == -1 and res[1]["best_f"] == -1 and not res[1]["scores_h"].any()
    assert res[2]["best_h"] == 5 and res[2]["inliers_h"].all()


def test_batch_entry_beyond_the_second_frame_counts_as_unmatched(batch):
    cnt = batch["cnt"].cpu().numpy()
    d = batch["m12"].clone()
    host = batch["m12"].cpu().numpy().copy()
    i = int(np.flatnonzero(host[0, : cnt[0]] >= 0)[1])
    d[0, i] = int(cnt[1])          # first index past frame 1's keypoints
    d[2, 0] = 1 << 30
    d[2, 1] = -7
    if cnt[0] < d.shape[1]:
        d[0, int(cnt[0])] = 0      # an index at counts[f1] is no keypoint of frame 0
    host[0, i] = host[2, 0] = host[2, 1] = -1
    res = _batch_vs_host_and_model(batch, d, host)
    assert res[0]["n_matches"] == batch["nm"][0] - 1


def test_batch_outputs_may_be_null(batch):
    """Scores not asked for (kept in scratch for the call) and a single model."""
    import ctypes

    import torch

    from orbslam_jpminipc_amd._native import check, hip_lib, ptr

    P, cap = batch["m12"].shape
    H21, H12 = (torch.from_numpy(batch[k]).cuda() for k in ("H21", "H12"))
    full = orb.Initializer(1.0).check_batch_device(batch["kps"], batch["cnt"], batch["f1"], batch["f2"], batch["m12"],
                                                   H21, H12, None)
    assert "scores_f" not in full
    best = torch.full((P,), -9, dtype=torch.int32, device="cuda")
    bs = torch.full((P,), -9.0, dtype=torch.float32, device="cuda")
    z = ctypes.c_void_p(0)
    s = torch.cuda.current_stream()
    check(hip_lib().orb_initializer_check_batch_device(
        ptr(batch["kps"]), ptr(batch["cnt"]), cap, P, ptr(batch["f1"]), ptr(batch["f2"]), ptr(batch["m12"]), 1.0,
        H21.shape[1], ptr(H21), ptr(H12), z, z, z, ptr(best), ptr(bs), z, z, z, z, z, ctypes.c_void_p(s.cuda_stream)))
    torch.cuda.synchronize()
    assert torch.equal(best, full["best_h"]) and torch.equal(bs, full["best_score_h"])


def test_native_facade(tmp_path):
    exe = ROOT / "build" / "initializer_facade"
    if not exe.exists():  # build() makes it; a tree that skipped build() compiles it here (g++, seconds)
        import __graft_entry__ as ge

        exe.parent.mkdir(exist_ok=True)
        subprocess.run(ge.INITIALIZER_FACADE_CMD(exe), check=True)
    k1, k2, m12, H21, H12, F21 = synth_case(129, 65)
    want = model.check(k1, k2, m12, 1.0, H21, H12, F21)
    path = tmp_path / "case.bin"
    path.write_bytes(struct.pack("<3i", len(k1), len(k2), 65) + k1.tobytes() + k2.tobytes() + m12.tobytes() +
                     H21.tobytes() + H12.tobytes() + F21.tobytes())
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "initializer facade OK" in r.stdout and "FAIL" not in r.stdout, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    for tag, t in (("H", "h"), ("F", "f")):
        bits = struct.unpack("<I", f32(want["best_score_" + t]).tobytes())[0]
        line = f"{tag} best={want['best_' + t]} score=0x{bits:08x} inliers={int(want['inliers_' + t].sum())} N=129"
        assert line in lines, (line, r.stdout)
