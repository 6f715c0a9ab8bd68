"""orb_initializer_compute_hypotheses / orb_initializer_ransac / orb_initializer_ransac_batch_device
(csrc/orb_initializer.hip) against the CPU model of the minimal sets, Normalize, ComputeH21 /
ComputeF21 and OpenCV 2.4's SVDecomp as read (tests/initializer_ransac_model.py), with the model of
the two checks behind it: sets and every hypothesis array bit for bit (NaN as "is NaN"), scores,
best indices, masks, RH and the chosen model equal."""
import ctypes
import pathlib
import struct
import subprocess

import numpy as np
import pytest

import initializer_model as check_model
import initializer_ransac_model as model
import orbslam_jpminipc_amd as orb
from orbslam_jpminipc_amd._native import KEYPOINT_DTYPE, ORB_EINVAL, ORB_ENOTSUP, OrbError
from test_initializer_ransac_model import (draw_for, draws, golden, golden_as_result, kps_of, replay_sets, same_find,
                                           two_view_case)

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parents[1]
f32 = np.float32
HYP = ("H21", "H12", "F21", "Hn", "Fn")


def same_hypotheses(got, want):
    assert got["n_matches"] == want["n_matches"]
    assert np.array_equal(got["sets"], want["sets"])
    for k in HYP + ("T1", "T2"):
        assert model.same_bits(got[k], want[k]), k


def run_find(k1, k2, m12, r31, sigma=1.0):
    got = orb.InitializerRansac(sigma).find(k1, k2, m12, r31)
    with np.errstate(all="ignore"):
        want = model.find(k1, k2, m12, r31, sigma)
    same_find(got, want)
    return got, want


@pytest.mark.parametrize("n_hyp", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("N", [8, 9, 100])
def test_sets_and_hypotheses_are_exact(N, n_hyp):
    """Frames hold more keypoints than matches, so Normalize sees unmatched keypoints."""
    k1, k2, m12 = two_view_case(N)
    assert len(k1) > N and len(k2) > N
    r31 = draws(n_hyp, 10 * N + n_hyp)
    got = orb.InitializerRansac().compute_hypotheses(k1, k2, m12, rand31=r31)
    want = model.hypotheses(k1, k2, m12, rand31=r31)
    same_hypotheses(got, want)
    assert want["n_matches"] == N and not np.isnan(want["H21"]).any() and want["F21"].any()
    # given sets instead of draws
    got = orb.InitializerRansac().compute_hypotheses(k1, k2, m12, sets=want["sets"])
    same_hypotheses(got, want)


def test_moved_entries_drawn_again():
    """N = 8 (every set is a permutation of all matches) and sets built to draw, two and three
    times, the position an earlier draw emptied."""
    k1, k2, m12 = two_view_case(8)
    r31 = draws(64, 3)
    r31[0] = 0
    assert replay_sets(8, r31)[1].sum() >= 32
    same_hypotheses(orb.InitializerRansac().compute_hypotheses(k1, k2, m12, rand31=r31),
                    model.hypotheses(k1, k2, m12, rand31=r31))
    k1, k2, m12 = two_view_case(100)
    r31 = draws(16, 4)
    for it in range(16):
        q = 5 * it
        r31[it, :3] = [draw_for(q, 100), draw_for(q, 99), draw_for(q, 98)]
    want = model.hypotheses(k1, k2, m12, rand31=r31)
    assert want["sets"][3, :3].tolist() == [15, 99, 98]
    same_hypotheses(orb.InitializerRansac().compute_hypotheses(k1, k2, m12, rand31=r31), want)


def test_golden_fixture():
    k1, k2, m12, g = golden()
    got, want = run_find(k1, k2, m12, g["rand31"], float(g["sigma"]))
    same_find(got, golden_as_result(g))
    assert got["best_h"] >= 0 and got["best_f"] >= 0 and not np.isnan(got["H"]).any()


@pytest.mark.parametrize("N", [7, 0])
def test_fewer_than_eight_matches(N):
    k1, k2, m12 = two_view_case(20)
    m12 = m12.copy()
    m12[np.flatnonzero(m12 >= 0)[N:]] = -1
    r31 = draws(65, 1)
    h = orb.InitializerRansac().compute_hypotheses(k1, k2, m12, rand31=r31)
    same_hypotheses(h, model.hypotheses(k1, k2, m12, rand31=r31))
    assert h["n_matches"] == N and not any(h[k].any() for k in HYP) and not h["sets"].any()
    got, want = run_find(k1, k2, m12, r31)
    assert got["best_h"] == got["best_f"] == -1 and got["best_score_h"] == 0 and got["best_score_f"] == 0
    assert not got["inliers_h"].any() and not got["inliers_f"].any() and len(got["inliers_h"]) == N
    assert np.isnan(got["RH"]) and not got["use_h"] and np.isnan(got["H"]).all() and np.isnan(got["F"]).all()


def test_rank_deficient_set_drives_the_fill_in_with_consumed_draws():
    """Two identical correspondences among 8 and draws that select all 8.  In the first four sets
    the two copies come first: the first rotation of ComputeF21's decomposition then leaves an
    exactly zero row, which is filled in from the generator before the row F is made from
    (tests/test_initializer_ransac_model.py counts the draws)."""
    k1, k2, m12 = two_view_case(8, n1=8, n2=8)
    k1, k2 = k1.copy(), k2.copy()
    k1[5] = k1[2]
    k2[m12[5]] = k2[m12[2]]
    r31 = draws(8, 9)
    r31[:4, 0], r31[:4, 1] = draw_for(2, 8), draw_for(5, 7)
    with np.errstate(all="ignore"):
        want = model.hypotheses(k1, k2, m12, rand31=r31)
        got = orb.InitializerRansac().compute_hypotheses(k1, k2, m12, rand31=r31)
    assert want["sets"][0, :2].tolist() == [2, 5] and all(sorted(s) == list(range(8)) for s in want["sets"].tolist())
    same_hypotheses(got, want)
    run_find(k1, k2, m12, r31)


def test_zero_deviation_in_x():
    k1, k2, m12 = two_view_case(30)
    k2 = k2.copy()
    k2["x"] = 100.0
    r31 = draws(65, 2)
    with np.errstate(all="ignore"):
        want = model.hypotheses(k1, k2, m12, rand31=r31)
    got = orb.InitializerRansac().compute_hypotheses(k1, k2, m12, rand31=r31)
    assert np.isinf(want["T2"][0, 0]) and np.isnan(want["H21"]).any()
    same_hypotheses(got, want)
    run_find(k1, k2, m12, r31)
    # a frame without keypoints next to one with some
    e = np.zeros(0, KEYPOINT_DTYPE)
    got, want = run_find(k1, e, np.full(len(k1), -1, np.int32), r31)
    assert got["n_matches"] == 0 and got["best_h"] == -1


def test_staging_reuse_across_sizes():
    """One thread, one context: a small call, one large enough to grow the device arena and the pinned
    staging, a small one again and a pair without keypoints, each against the model, for the whole
    RANSAC and for the hypotheses alone; n1 != n2 and both below the larger of a later call, so the
    padding between a frame's count and the capacity is read."""
    e = np.zeros(0, KEYPOINT_DTYPE)
    seq = [(*two_view_case(40, 65, 50), 1), (*two_view_case(100, 110, 130), 65), (*two_view_case(9, 12, 10), 1),
           (e, e, np.zeros(0, np.int32), 1)]
    for k1, k2, m12, n_hyp in seq:
        r31 = draws(n_hyp, len(k1))
        got, want = run_find(k1, k2, m12, r31)
        assert got["n_matches"] == int((m12 >= 0).sum()) and len(got["inliers_h"]) == got["n_matches"]
        h = orb.InitializerRansac().compute_hypotheses(k1, k2, m12, rand31=r31)
        same_hypotheses(h, model.hypotheses(k1, k2, m12, rand31=r31))


def test_find_equals_compute_hypotheses_then_check_and_the_model():
    k1, k2, m12 = two_view_case(100)
    r31 = draws(200, 8)
    init = orb.InitializerRansac(1.0)
    got, want = run_find(k1, k2, m12, r31)
    h = init.compute_hypotheses(k1, k2, m12, rand31=r31)
    c = init.check(k1, k2, m12, h["H21"], h["H12"], h["F21"])
    check_model.same_result(got, c)
    check_model.same_result(c, want)
    for k in ("H21", "H12", "F21", "sets"):
        assert model.same_bits(got[k], h[k]), k
    assert model.same_bits(f32(got["RH"]), f32(c["RH"]))
    assert got["best_h"] >= 0 and got["best_f"] >= 0 and 0 < got["inliers_h"].sum() and got["inliers_f"].sum() > 50
    assert model.same_bits(got["H"].reshape(9), h["H21"][got["best_h"]])
    assert model.same_bits(got["F"].reshape(9), h["F21"][got["best_f"]])
    # another sigma changes the scores, not the hypotheses
    g2, _ = run_find(k1, k2, m12, r31, 2.0)
    assert g2["H21"].tobytes() == got["H21"].tobytes() and g2["scores_h"].tobytes() != got["scores_h"].tobytes()


# ---- batched, on device-resident extractor and matcher output ---------------------------------

def _frames_batch(P):
    """P pairs over 2 P synthetic frames (pair p = frames 2 p, 2 p + 1, each a two_view_case);
    pair 1 (when there is one) has fewer than 8 matches."""
    import torch

    cap = 160
    kps = np.zeros((2 * P, cap), KEYPOINT_DTYPE)
    cnt = np.zeros(2 * P, np.int32)
    m12 = np.full((P, cap), -1, np.int32)
    for p in range(P):
        N = 5 if p == 1 else 40 + 3 * (p % 20)
        cnt[2 * p], cnt[2 * p + 1] = cap - 7 * (p % 5), cap - 3 * (p % 7)
        a, b, m = two_view_case(N, n1=int(cnt[2 * p]), n2=int(cnt[2 * p + 1]), seed=p)
        kps[2 * p, : len(a)], kps[2 * p + 1, : len(b)], m12[p, : len(m)] = a, b, m
    f1 = 2 * np.arange(P, dtype=np.int32)
    d = dict(kps=torch.from_numpy(kps.view(np.uint8).reshape(2 * P, cap, 28)).cuda(), cnt=torch.from_numpy(cnt).cuda(),
             f1=torch.from_numpy(f1).cuda(), f2=torch.from_numpy(f1 + 1).cuda(), m12=torch.from_numpy(m12).cuda())
    return kps, cnt, m12, d


@pytest.mark.parametrize("P", [1, 3, 50])
def test_batch_equals_host_and_model(P):
    import torch

    kps, cnt, m12, d = _frames_batch(P)
    n_hyp = 65
    r31 = np.stack([draws(n_hyp, 100 + p) for p in range(P)])
    r31[0, 3, 2] = -5  # a negative draw counts as 0 in the batch form
    init = orb.InitializerRansac(1.0)
    out = init.find_batch_device(d["kps"], d["cnt"], d["f1"], d["f2"], d["m12"], torch.from_numpy(r31).cuda())
    # a host call right behind the device call, no synchronise between them
    k1, k2 = kps[0, : cnt[0]], kps[1, : cnt[1]]
    host0 = init.find(k1, k2, m12[0, : cnt[0]], np.maximum(r31[0], 0))
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    for p in range(P):
        k1, k2 = kps[2 * p, : cnt[2 * p]], kps[2 * p + 1, : cnt[2 * p + 1]]
        n = int(out["n_matches"][p])
        got = {"n_matches": n, "sets": out["sets"][p], "H": out["best_H21"][p].reshape(3, 3),
               "F": out["best_F21"][p].reshape(3, 3), "RH": out["RH"][p], "use_h": bool(out["use_h"][p])}
        for k in ("H21", "H12", "F21"):
            got[k] = out[k][p]
        for t in "hf":
            got.update({"scores_" + t: out["scores_" + t][p], "best_" + t: int(out["best_" + t][p]),
                        "best_score_" + t: out["best_score_" + t][p],
                        "inliers_" + t: out["inliers_" + t][p, :n].astype(bool)})
            assert not out["inliers_" + t][p, n:].any()
        host = host0 if p == 0 else init.find(k1, k2, m12[p, : len(k1)], r31[p])
        with np.errstate(all="ignore"):
            want = model.find(k1, k2, m12[p, : len(k1)], np.maximum(r31[p], 0))
        same_find(got, host)
        same_find(got, want)
        if p == 1:
            assert n == 5 and got["best_h"] == -1 and not got["H21"].any() and np.isnan(got["RH"])
        else:
            assert n >= 40 and got["best_h"] >= 0 and got["best_f"] >= 0


def test_batch_outputs_may_be_null():
    import torch

    from orbslam_jpminipc_amd._native import check, hip_lib, ptr

    kps, cnt, m12, d = _frames_batch(3)
    r31 = torch.from_numpy(np.stack([draws(65, 100 + p) for p in range(3)])).cuda()
    init = orb.InitializerRansac(1.0)
    full = init.find_batch_device(d["kps"], d["cnt"], d["f1"], d["f2"], d["m12"], r31)
    lean = init.find_batch_device(d["kps"], d["cnt"], d["f1"], d["f2"], d["m12"], r31, hypotheses=False)
    assert "H21" not in lean
    for k in lean:
        assert torch.equal(lean[k].view(torch.uint8), full[k].view(torch.uint8)), k
    # only RH and the chosen model
    rh = torch.full((3,), -9.0, dtype=torch.float32, device="cuda")
    use = torch.full((3,), -9, dtype=torch.int32, device="cuda")
    z = ctypes.c_void_p(0)
    s = torch.cuda.current_stream()
    check(hip_lib().orb_initializer_ransac_batch_device(
        ptr(d["kps"]), ptr(d["cnt"]), 160, 3, ptr(d["f1"]), ptr(d["f2"]), ptr(d["m12"]), 1.0, 65, ptr(r31),
        *([z] * 15), ptr(rh), ptr(use), ctypes.c_void_p(s.cuda_stream)))  # 15 absent outputs before d_RH
    torch.cuda.synchronize()
    assert torch.equal(rh.view(torch.int32), full["RH"].view(torch.int32)) and torch.equal(use, full["use_h"])


def test_chain_from_search_for_initialization_without_a_host_copy():
    import torch

    W, H = 320, 240
    frames = orb.synth_stream(W, H, stream=7, first=0, count=3).copy()
    ext = orb.ORBextractor(500, 1.2, 8, orb.FAST_SCORE, 20, device=0, max_batch=3)
    kps, desc, cnt = ext.extract_batch_device(torch.from_numpy(frames).cuda())
    f1 = torch.tensor([0, 1], dtype=torch.int32, device="cuda")
    f2 = torch.tensor([1, 2], dtype=torch.int32, device="cuda")
    m12, nm = orb.ORBmatcher(0.9, True).search_for_initialization_batch_device(kps, desc, cnt, f1, f2, W, H, 100)
    r31 = np.stack([draws(200, 40 + p) for p in range(2)])
    init = orb.InitializerRansac(1.0)
    out = init.find_batch_device(kps, cnt, f1, f2, m12, torch.from_numpy(r31).cuda())
    torch.cuda.synchronize()
    cap = int(kps.shape[1])
    hk = kps.cpu().numpy().view(KEYPOINT_DTYPE).reshape(3, cap)
    hc, hm = cnt.cpu().numpy(), m12.cpu().numpy()
    assert out["n_matches"].cpu().tolist() == nm.cpu().tolist() and min(nm.cpu().tolist()) >= 8
    for p in range(2):
        want = model.find(hk[p, : hc[p]], hk[p + 1, : hc[p + 1]], hm[p, : hc[p]], r31[p])
        assert np.array_equal(out["sets"][p].cpu().numpy(), want["sets"])
        for k in ("H21", "H12", "F21"):
            assert model.same_bits(out[k][p].cpu().numpy(), want[k]), k
        assert int(out["best_h"][p]) == want["best_h"] and int(out["best_f"][p]) == want["best_f"]
        assert model.same_bits(out["RH"][p].cpu().numpy(), f32(want["RH"]))
        assert bool(out["use_h"][p]) == want["use_h"]


def test_refusals():
    k1, k2, m12 = two_view_case(20)
    init = orb.InitializerRansac()
    r31 = draws(4, 1)
    bad = r31.copy()
    bad[2, 5] = -1
    for call in (lambda: init.find(k1, k2, m12, bad), lambda: init.compute_hypotheses(k1, k2, m12, rand31=bad)):
        with pytest.raises(OrbError) as e:
            call()
        assert e.value.code == ORB_EINVAL and "rand31[21]" in str(e.value)
    sets = model.minimal_sets(20, r31)
    sets[1, 1] = 20
    with pytest.raises(OrbError) as e:
        init.compute_hypotheses(k1, k2, m12, sets=sets)
    assert e.value.code == ORB_EINVAL and "sets[9]" in str(e.value)
    mb = m12.copy()
    mb[3] = len(k2)
    with pytest.raises(OrbError) as e:
        init.find(k1, k2, mb, r31)
    assert e.value.code == ORB_EINVAL and "matches12[3]" in str(e.value)
    for n in (0, 1025):
        with pytest.raises(OrbError) as e:
            init.find(k1, k2, m12, np.zeros((n, 8), np.int32))
        assert e.value.code == ORB_EINVAL and "n_hyp" in str(e.value)
    big = np.zeros(8193, KEYPOINT_DTYPE)
    with pytest.raises(OrbError) as e:
        init.find(big, k2, np.full(8193, -1, np.int32), r31)
    assert e.value.code == ORB_ENOTSUP and "8192" in str(e.value)
    # the call after a refusal is served
    run_find(k1, k2, m12, r31)


def test_native_facade(tmp_path):
    exe = ROOT / "build" / "initializer_ransac_facade"
    if not exe.exists():  # build() makes it; a tree that skipped build() compiles it here (g++, seconds)
        import __graft_entry__ as ge

        exe.parent.mkdir(exist_ok=True)
        subprocess.run(ge.INITIALIZER_RANSAC_FACADE_CMD(exe), check=True)
    k1, k2, m12 = two_view_case(100)
    r31 = draws(65, 12)
    want = model.find(k1, k2, m12, r31)
    path = tmp_path / "case.bin"
    path.write_bytes(struct.pack("<3i", len(k1), len(k2), 65) + k1.tobytes() + k2.tobytes() + m12.tobytes() + r31.tobytes())
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "initializer ransac facade OK" in r.stdout and "FAIL" not in r.stdout, r.stdout + r.stderr
    lines = r.stdout.splitlines()

    def bits(x):
        return struct.unpack("<I", f32(x).tobytes())[0]

    assert f"N=100 useH={int(want['use_h'])} RH=0x{bits(want['RH']):08x}" in lines, r.stdout
    for tag, t, M in (("H", "h", want["H"]), ("F", "f", want["F"])):
        m = " ".join(f"{bits(v):08x}" for v in M.reshape(9))
        line = f"{tag} score=0x{bits(want['best_score_' + t]):08x} inliers={int(want['inliers_' + t].sum())} m={m}"
        assert line in lines, (line, r.stdout)
    s = sum((k + 1) * int(v) for k, v in enumerate(want["sets"].reshape(-1))) % (1 << 32)
    assert f"sets={s}" in lines, r.stdout
