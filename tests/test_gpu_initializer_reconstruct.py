"""orb_initializer_reconstruct / _reconstruct_batch_device / orb_initializer_initialize /
_initialize_batch_device (csrc/orb_initializer.hip) against the CPU model of ReconstructF /
ReconstructH, CheckRT, Triangulate and DecomposeE (tests/initializer_reconstruct_model.py): every
output bit for bit (NaN as "is NaN") except parallax_deg, which goes through acosf and is held to
the bound the golden generator recorded."""
import pathlib
import struct
import subprocess

import numpy as np
import pytest

import initializer_reconstruct_model as model
import initializer_reconstruct_scenes as scenes
import orbslam_jpminipc_amd as orb
from orbslam_jpminipc_amd._native import KEYPOINT_DTYPE, ORB_EINVAL, ORB_ENOTSUP, OrbError
from test_initializer_ransac_model import draws, kps_of, same_find

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parents[1]
GOLD = dict(np.load(ROOT / "tests" / "golden" / "initializer_reconstruct.npz"))
BOUND = float(GOLD["parallax_bound"])
K4 = scenes.K4
f32 = np.float32
_scene_cache = {}


def scene(name):
    """The named scene with unmatched keypoints mixed into both frames and frame 2 permuted: match
    ordinal, frame-1 index and frame-2 index all differ."""
    if name not in _scene_cache:
        _scene_cache[name] = scenes.scene(name, extra1=17, extra2=9, shuffle=True)
    return _scene_cache[name]


def run(k1, k2, m12, M21, use_h, mask, K4=K4, **kw):
    got = orb.InitializerRansac().reconstruct(kps_of(k1), kps_of(k2), m12, M21, use_h, mask, K4, **kw)
    with np.errstate(all="ignore"):
        want = model.reconstruct(k1, k2, m12, M21, use_h, mask, K4, **kw)
    model.same_reconstruction(got, want, BOUND)
    return got, want


@pytest.mark.parametrize("k", [0, 1, 49, 50, 51, 52, 63, 64, 65, 130])
@pytest.mark.parametrize("name", ["f130", "h_accept"])
def test_first_k_inliers(name, k):
    """The mask cut to the first k matches: min(50, size - 1), nGood == 0 -> parallax 0, the wave
    tail, nMinGood / minTriangulated around 50, and a mask with no set entry (k = 0)."""
    s = scene(name)
    got, want = run(s["k1"], s["k2"], s["m12"], s["M21"], s["use_h"], scenes.mask_first(s["m12"], k))
    b = int(np.argmax(want["n_good"]))
    assert got["n_inliers"] == k and want["n_good"][b] == k  # every inlier of these scenes is counted
    if k <= 49:  # F: maxGood < nMinGood = 50; H: bestGood > minTriangulated fails (at k = 50 too)
        assert not got["ok"]
    if k == 130 or (k == 50 and name == "h_accept"):
        assert got["ok"] == (k == 130)
    if k == 0:
        assert not got["n_good"].any() and not got["parallax_deg"].any() and np.isnan(got["cos_parallax"]).all()
    else:  # the selected cosine is the (min(50, k - 1) + 1)-th smallest of the winner's
        assert got["parallax_deg"][b] > 0 and not np.isnan(got["cos_parallax"][b])


def test_vp3d_is_indexed_by_the_frame1_keypoint():
    """More keypoints than matches and matches not in keypoint order: the rows of P3D / triangulated
    that are written are exactly the matched frame-1 indices, and the points are the scene's."""
    s = scene("f130")
    got, _ = run(s["k1"], s["k2"], s["m12"], s["M21"], False, scenes.mask_first(s["m12"], 130))
    matched = s["m12"] >= 0
    assert got["ok"] and len(s["k1"]) == 147 and matched.sum() == 130
    assert np.array_equal(got["triangulated"], matched) and np.array_equal(got["P3D"].any(1), matched)
    scale = np.linalg.norm(s["t"])  # t21 is a unit vector
    # depth error z^2 d / (f b): z <= 10, f = 500, b = 0.3, disparity noise d up to 4 sigma sqrt(2) = 1.7 px
    assert np.abs(got["P3D"][matched] * scale - s["X"]).max() < 100 * 1.7 / 150
    assert got["best"] == 2 and np.abs(got["R21"] - s["R"]).max() < 1e-5


def test_pure_rotation_counts_points_without_triangulating_them():
    """t = 0: every cosine is >= 0.99998, so the depth gates do not apply, the points are counted
    (vP3D written, nGood) but vbGood stays false, and the parallax rejects the pair."""
    X = scenes.volume_points(130, 5)
    k1, k2, m12 = scenes.make_pair(X, scenes.R_TRUE, np.zeros(3), noise=0.0, seed=3, extra1=5, extra2=3, shuffle=True)
    F = scenes.F_of(scenes.R_TRUE, np.array([0.3, 0.02, 0.03]))  # any t fits a pure rotation
    got, want = run(k1, k2, m12, F, False, np.ones(130, np.uint8))
    assert not got["ok"] and got["n_good"].max() == 130 and got["parallax_deg"][np.argmax(got["n_good"])] < 1.0
    b = int(np.argmax(want["n_good"]))
    assert not want["hyp_good"][b].any() and want["hyp_P3D"][b].any(1).sum() == 130
    assert not got["P3D"].any() and not got["triangulated"].any()
    # accepted with the parallax test out of the way: counted points appear in P3D, none is triangulated
    got, want = run(k1, k2, m12, F, False, np.ones(130, np.uint8), min_parallax=-1.0)
    if got["ok"]:
        assert got["P3D"].any(1).sum() == got["n_good"][got["best"]] and not got["triangulated"].any()


def test_far_points_are_counted_and_keep_vp3d_but_are_not_triangulated():
    """An accepted pair in which 12 of 130 points lie at depth 2000: their cosParallax is >= 0.99998,
    so they count in nGood and get their vP3D entry while vbTriangulated stays false for them."""
    X = scenes.volume_points(130, 230).copy()
    X[:12] *= 2000.0 / X[:12, 2:3]
    t = np.array([0.3, 0.02, 0.03])
    k1, k2, m12 = scenes.make_pair(X, scenes.R_TRUE, t, noise=0.3, seed=1, extra1=17, extra2=9, shuffle=True)
    got, _ = run(k1, k2, m12, scenes.F_of(scenes.R_TRUE, t), False, np.ones(130, np.uint8))
    far = np.flatnonzero(m12 >= 0)[:12]
    assert got["ok"] and got["n_good"][got["best"]] == 130 and got["P3D"].any(1).sum() == 130
    assert got["triangulated"].sum() == 118 and not got["triangulated"][far].any() and got["P3D"][far].all(1).all()


def test_parallax_equal_to_min_parallax_accepts_for_h_and_rejects_for_f():
    """bestParallax >= minParallax in ReconstructH, parallax > minParallax in ReconstructF: each model
    called again with min_parallax set to the very parallax it selected."""
    for name, accepts in (("h_accept", True), ("f130", False)):
        s = scene(name)
        mask = scenes.mask_first(s["m12"], 130)
        init = orb.InitializerRansac()
        first = init.reconstruct(kps_of(s["k1"]), kps_of(s["k2"]), s["m12"], s["M21"], s["use_h"], mask, K4)
        assert first["ok"]
        p = first["parallax_deg"][first["best"]]
        again = init.reconstruct(kps_of(s["k1"]), kps_of(s["k2"]), s["m12"], s["M21"], s["use_h"], mask, K4, min_parallax=p)
        above = init.reconstruct(kps_of(s["k1"]), kps_of(s["k2"]), s["m12"], s["M21"], s["use_h"], mask, K4,
                                 min_parallax=np.nextafter(p, f32(np.inf)))
        below = init.reconstruct(kps_of(s["k1"]), kps_of(s["k2"]), s["m12"], s["M21"], s["use_h"], mask, K4,
                                 min_parallax=np.nextafter(p, f32(0)))
        assert again["ok"] == accepts and not above["ok"] and below["ok"]
        rule = model.rule_h if s["use_h"] else model.rule_f
        assert again["best"] == rule(again["n_good"][:8 if s["use_h"] else 4], again["parallax_deg"][:8 if s["use_h"] else 4], 130, p)
        assert not again["ok"] or again["P3D"].tobytes() == first["P3D"].tobytes()


def _sigma_between_fused_and_unfused(args):
    """A sigma whose th2 = 4 sigma^2 separates the squared reprojection error of one match as the
    reference build computes it (three fused multiply-adds per image) from the same error without the
    fusions, the match's other error being below both: found with the model's two variants."""
    r0 = model.reconstruct(*args, sigma=100.0)
    r2 = model.reconstruct(*args, sigma=100.0, acos_variant=2)
    e0, e2 = r0["hyp_err"][r0["best"]], r2["hyp_err"][r0["best"]]
    found = []
    for key, img in zip(*np.nonzero((e0 != e2) & ~np.isnan(e0))):
        lo, hi = sorted((e0[key, img], e2[key, img]))
        if not max(e0[key, 1 - img], e2[key, 1 - img]) < lo:
            continue
        cand = f32(np.sqrt(np.float64(lo) / 4))
        for _ in range(8):
            cand = np.nextafter(cand, f32(0))
        for _ in range(17):
            if lo <= f32(4.0 * np.float64(f32(cand * cand))) < hi:
                found.append((float(lo), float(cand)))
                break
            cand = np.nextafter(cand, f32(np.inf))
    return max(found)[1] if found else None


@pytest.mark.parametrize("name", ["f130", "h_accept"])
def test_reprojection_error_is_the_fused_one(name):
    """th2 placed between the fused and the unfused squared error of one match: nGood tells which of
    the two the kernel computes."""
    s = scene(name)
    args = (s["k1"], s["k2"], s["m12"], s["M21"], s["use_h"], np.ones(130, np.uint8), K4)
    sigma = _sigma_between_fused_and_unfused(args)
    assert sigma is not None
    fused, plain = model.reconstruct(*args, sigma=sigma), model.reconstruct(*args, sigma=sigma, acos_variant=2)
    assert abs(int(fused["n_good"][fused["best"]]) - int(plain["n_good"][fused["best"]])) == 1
    got = orb.InitializerRansac(sigma).reconstruct(kps_of(s["k1"]), kps_of(s["k2"]), s["m12"], s["M21"], s["use_h"],
                                                   np.ones(130, np.uint8), K4)
    model.same_reconstruction(got, fused, BOUND)


def test_non_finite_triangulations_are_rejected_by_isfinite_alone():
    """Identical keypoints in both frames with an identity rotation (parallel rays), and three
    frame-2 keypoints that are NaN / inf: those triangulate to non-finite points and are skipped."""
    X = scenes.volume_points(130, 5)
    k1, _, m12 = scenes.make_pair(X, np.eye(3), np.zeros(3), noise=0.0, seed=3)
    k2 = k1.copy()
    k2[4], k2[70, 0], k2[129, 1] = np.nan, np.inf, -np.inf
    F = scenes.F_of(np.eye(3), np.array([1.0, 0.0, 0.0]))
    got, want = run(k1, k2, m12, F, False, np.ones(130, np.uint8))
    assert not got["ok"] and got["n_good"].max() <= 127
    assert not want["hyp_P3D"][:, [4, 70, 129]].any()


def test_gate_failure_nan_model_and_too_few_matches():
    s = scene("h_accept")
    mask = scenes.mask_first(s["m12"], 130)
    got, _ = run(s["k1"], s["k2"], s["m12"], np.eye(3, dtype=f32), True, mask)  # d1 == d2 == d3
    assert got["n_motion"] == 0 and not got["ok"] and got["best"] == -1 and not got["motion_R"].any()
    for use_h in (True, False):  # the model of a pair whose best index was -1
        got, _ = run(s["k1"], s["k2"], s["m12"], np.full((3, 3), np.nan, f32), use_h, mask)
        assert not got["ok"] and not got["n_good"].any() and not got["P3D"].any()
    m7 = s["m12"].copy()
    m7[np.flatnonzero(m7 >= 0)[7:]] = -1
    init = orb.InitializerRansac()
    got = init.initialize(kps_of(s["k1"]), kps_of(s["k2"]), m7, draws(16, 2), K4)
    with np.errstate(all="ignore"):
        want = model.initialize(s["k1"], s["k2"], m7, draws(16, 2), K4)
    model.same_reconstruction(got, want, BOUND)
    assert got["n_matches"] == 7 and got["best_h"] == -1 and not got["ok"] and got["n_inliers"] == 0


def test_staging_reuse_across_sizes():
    """One thread, one context: a small call, one large enough to grow the device arena and the pinned
    staging, a small one again and a pair without keypoints, each against the model; the frames hold
    different numbers of keypoints, so the padding between a count and the capacity is read."""
    for name in ("f60", "f130", "f60"):
        s = scene(name)
        assert len(s["k1"]) != len(s["k2"])
        got, _ = run(s["k1"], s["k2"], s["m12"], s["M21"], s["use_h"], scenes.mask_first(s["m12"], 10 ** 6))
        assert got["ok"] and len(got["P3D"]) == len(s["k1"])
    none = np.zeros((0, 2), f32)
    got, _ = run(none, none, np.zeros(0, np.int32), np.eye(3, dtype=f32), False, np.zeros(0, np.uint8))
    assert not got["ok"] and got["n_inliers"] == 0


@pytest.mark.parametrize("name", scenes.SCENE_NAMES)
def test_golden_fixture(name):
    g = {k[len(name) + 1:]: v for k, v in GOLD.items() if k.startswith(name + ".")}
    got = orb.InitializerRansac().reconstruct(kps_of(g["k1"]), kps_of(g["k2"]), g["m12"], g["M21"], bool(g["use_h"]),
                                              g["mask"], GOLD["K4"])
    want = {k: (v if v.ndim else v.item()) for k, v in g.items()}
    want["triangulated"] = g["triangulated"].astype(bool)
    model.same_reconstruction(got, want, BOUND)
    assert got["ok"] == name.startswith(("f", "h_accept"))


@pytest.mark.parametrize("name", ["f130", "h_accept", "h_ambiguous_t"])
def test_initialize_equals_find_then_reconstruct(name):
    s = scene(name)
    k1, k2, r31 = kps_of(s["k1"]), kps_of(s["k2"]), draws(64, 5)
    init = orb.InitializerRansac()
    got = init.initialize(k1, k2, s["m12"], r31, K4)
    f = init.find(k1, k2, s["m12"], r31)
    same_find(got, f)
    rec = init.reconstruct(k1, k2, s["m12"], f["H"] if f["use_h"] else f["F"], f["use_h"],
                           f["inliers_h"] if f["use_h"] else f["inliers_f"], K4)
    model.same_reconstruction(got, rec, 0.0)
    with np.errstate(all="ignore"):
        want = model.initialize(s["k1"], s["k2"], s["m12"], r31, K4)
    same_find(got, want)
    model.same_reconstruction(got, want, BOUND)
    assert got["use_h"] == (name != "f130") and got["ok"] == (name != "h_ambiguous_t")


def test_initialize_batch_equals_host_calls():
    """F-accept, H-accept, H-ambiguous, N = 7 and zero matches in one call, capacity 157."""
    import torch

    names = ["f130", "h_accept", "h_ambiguous_t", "h_accept", "f130"]
    P, cap = 5, 157
    kps = np.zeros((2 * P, cap), KEYPOINT_DTYPE)
    cnt = np.zeros(2 * P, np.int32)
    m12 = np.full((P, cap), -1, np.int32)
    for p, name in enumerate(names):
        s = scene(name)
        m = s["m12"].copy()
        if p >= 3:
            m[np.flatnonzero(m >= 0)[7 if p == 3 else 0:]] = -1
        cnt[2 * p], cnt[2 * p + 1] = len(s["k1"]), len(s["k2"])
        kps[2 * p, : cnt[2 * p]], kps[2 * p + 1, : cnt[2 * p + 1]], m12[p, : len(m)] = kps_of(s["k1"]), kps_of(s["k2"]), m
    f1 = 2 * np.arange(P, dtype=np.int32)
    r31 = np.stack([draws(64, 5 + p) for p in range(P)])
    init = orb.InitializerRansac()
    dk = torch.from_numpy(kps.view(np.uint8).reshape(2 * P, cap, 28)).cuda()
    dev = [torch.from_numpy(a).cuda() for a in (cnt, f1, f1 + 1, m12, r31)]
    out = init.initialize_batch_device(dk, dev[0], dev[1], dev[2], dev[3], dev[4], K4)
    found = init.find_batch_device(dk, dev[0], dev[1], dev[2], dev[3], dev[4], hypotheses=False)
    rec = init.reconstruct_batch_device(dk, dev[0], dev[1], dev[2], dev[3], found, K4)
    torch.cuda.synchronize()
    for k, v in rec.items():  # the two-call form equals the one-call form
        assert torch.equal(v.view(torch.uint8), out[k].view(torch.uint8)), k
    out = {k: v.cpu().numpy() for k, v in out.items()}
    oks = []
    for p in range(P):
        n1 = int(cnt[2 * p])
        host = init.initialize(kps[2 * p, :n1], kps[2 * p + 1, : cnt[2 * p + 1]], m12[p, :n1], r31[p], K4)
        got = dict(ok=bool(out["ok"][p]), R21=out["R21"][p].reshape(3, 3), t21=out["t21"][p], P3D=out["P3D"][p, :n1],
                   triangulated=out["triangulated"][p, :n1].astype(bool), n_motion=int(out["n_motion"][p]),
                   motion_R=out["motion_R"][p].reshape(8, 3, 3), motion_t=out["motion_t"][p].reshape(8, 3),
                   n_good=out["n_good"][p], cos_parallax=out["cos_parallax"][p], parallax_deg=out["parallax_deg"][p],
                   best=int(out["best"][p]), n_inliers=int(out["n_inliers"][p]))
        model.same_reconstruction(got, host, 0.0)  # bit for bit, parallax_deg included
        assert not out["P3D"][p, n1:].any() and not out["triangulated"][p, n1:].any()
        assert bool(out["use_h"][p]) == host["use_h"] and int(out["n_matches"][p]) == host["n_matches"]
        oks.append((host["use_h"], host["ok"], host["n_matches"]))
    assert oks == [(False, True, 130), (True, True, 130), (True, False, 130), (False, False, 7), (False, False, 0)]


def test_chain_from_search_for_initialization_without_a_host_copy():
    """Extraction, SearchForInitialization and the whole Initialize on the device for the committed
    320x240 stream; the answer is the model's, whether a pair initialises is printed, not required."""
    import torch

    W, H = 320, 240
    frames = orb.synth_stream(W, H, stream=7, first=0, count=3).copy()
    ext = orb.ORBextractor(500, 1.2, 8, orb.FAST_SCORE, 20, device=0, max_batch=3)
    kps, desc, cnt = ext.extract_batch_device(torch.from_numpy(frames).cuda())
    f1 = torch.tensor([0, 1], dtype=torch.int32, device="cuda")
    f2 = torch.tensor([1, 2], dtype=torch.int32, device="cuda")
    m12, nm = orb.ORBmatcher(0.9, True).search_for_initialization_batch_device(kps, desc, cnt, f1, f2, W, H, 100)
    r31 = np.stack([draws(200, 40 + p) for p in range(2)])
    K = np.array([250.0, 250.0, 160.0, 120.0], f32)
    out = orb.InitializerRansac(1.0).initialize_batch_device(kps, cnt, f1, f2, m12, torch.from_numpy(r31).cuda(), K)
    torch.cuda.synchronize()
    cap = int(kps.shape[1])
    hk = kps.cpu().numpy().view(KEYPOINT_DTYPE).reshape(3, cap)
    hc, hm = cnt.cpu().numpy(), m12.cpu().numpy()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    for p in range(2):
        n1 = int(hc[p])
        with np.errstate(all="ignore"):
            want = model.initialize(hk[p, :n1], hk[p + 1, : hc[p + 1]], hm[p, :n1], r31[p], K)
        got = dict(ok=bool(out["ok"][p]), R21=out["R21"][p].reshape(3, 3), t21=out["t21"][p], P3D=out["P3D"][p, :n1],
                   triangulated=out["triangulated"][p, :n1].astype(bool), n_motion=int(out["n_motion"][p]),
                   motion_R=out["motion_R"][p].reshape(8, 3, 3), motion_t=out["motion_t"][p].reshape(8, 3),
                   n_good=out["n_good"][p], cos_parallax=out["cos_parallax"][p], parallax_deg=out["parallax_deg"][p],
                   best=int(out["best"][p]), n_inliers=int(out["n_inliers"][p]))
        model.same_reconstruction(got, want, BOUND)
        assert bool(out["use_h"][p]) == want["use_h"] and want["n_inliers"] > 0
        print(f"pair {p}: use_h {want['use_h']} N {want['n_inliers']} n_good {want['n_good']} ok {want['ok']}")


def test_refusals():
    s = scene("f130")
    k1, k2, m12, M = kps_of(s["k1"]), kps_of(s["k2"]), s["m12"], s["M21"]
    mask = scenes.mask_first(m12, 130)
    init = orb.InitializerRansac()
    for idx, word in ((0, "fx"), (1, "fy")):
        for bad in (0.0, np.nan, np.inf):
            K = K4.copy()
            K[idx] = bad
            for call in (lambda: init.reconstruct(k1, k2, m12, M, False, mask, K),
                         lambda: init.initialize(k1, k2, m12, draws(8, 1), K)):
                with pytest.raises(OrbError) as e:
                    call()
                assert e.value.code == ORB_EINVAL and word in str(e.value)
    for sigma in (0.0, np.nan, np.inf):
        with pytest.raises(OrbError) as e:
            orb.InitializerRansac(sigma).reconstruct(k1, k2, m12, M, False, mask, K4)
        assert e.value.code == ORB_EINVAL and "sigma" in str(e.value)
    with pytest.raises(OrbError) as e:
        init.reconstruct(k1, k2, m12, M, 2, mask, K4)
    assert e.value.code == ORB_EINVAL and "use_h" in str(e.value)
    mb = mask.copy()
    mb[9] = 2
    with pytest.raises(OrbError) as e:
        init.reconstruct(k1, k2, m12, M, False, mb, K4)
    assert e.value.code == ORB_EINVAL and "inliers[9]" in str(e.value)
    big = np.zeros(8193, KEYPOINT_DTYPE)
    with pytest.raises(OrbError) as e:
        init.reconstruct(big, k2, np.full(8193, -1, np.int32), M, False, mask, K4)
    assert e.value.code == ORB_ENOTSUP and "8192" in str(e.value)
    # the call after a refusal is served
    run(s["k1"], s["k2"], m12, M, False, mask)


def test_native_facade(tmp_path):
    exe = ROOT / "build" / "initializer_reconstruct_facade"
    if not exe.exists():  # build() makes it; a tree that skipped build() compiles it here (g++, seconds)
        import __graft_entry__ as ge

        exe.parent.mkdir(exist_ok=True)
        subprocess.run(ge.INITIALIZER_RECONSTRUCT_FACADE_CMD(exe), check=True)
    s = scene("h_accept")
    k1, k2, m12 = kps_of(s["k1"]), kps_of(s["k2"]), s["m12"]
    mask = np.zeros(len(k1), np.uint8)
    mask[:130] = 1
    r31 = draws(64, 5)
    path = tmp_path / "case.bin"
    path.write_bytes(struct.pack("<4i", len(k1), len(k2), 64, 1) + K4.tobytes() + s["M21"].tobytes() + k1.tobytes() +
                     k2.tobytes() + m12.tobytes() + mask.tobytes() + r31.tobytes())
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "initializer reconstruct facade OK" in r.stdout and "FAIL" not in r.stdout, r.stdout + r.stderr

    def line(tag, w):
        if not w["ok"]:
            return f"{tag} ok=0 R=empty t=empty tri=0 p3d=0"
        hexs = lambda v: " ".join(f"{x:08x}" for x in np.ascontiguousarray(v, f32).reshape(-1).view(np.uint32))  # noqa: E731
        p = np.ascontiguousarray(w["P3D"], f32).reshape(-1).view(np.uint32).astype(np.uint64)
        ck = sum((i + 1) * int(v) for i, v in enumerate(p)) % (1 << 32)
        return f"{tag} ok=1 R={hexs(w['R21'])} t={hexs(w['t21'])} tri={int(w['triangulated'].sum())} p3d={ck}"

    with np.errstate(all="ignore"):
        rec = model.reconstruct(s["k1"], s["k2"], m12, s["M21"], True, mask[:130], K4)
        ini = model.initialize(s["k1"], s["k2"], m12, r31, K4)
    lines = r.stdout.splitlines()
    assert rec["ok"] and ini["ok"]
    assert line("reconstruct", rec) in lines and line("initialize", ini) in lines, r.stdout
