"""orb_create_new_map_points / _batch_device, orb_scene_median_depth / _batch_device and orb_compute_f12
(csrc/orb_localmap.hip) against the CPU model of CreateNewMapPoints (tests/local_mapping_model.py): every
output bit for bit, NaN as "is NaN".  The code has no libm call, so nothing here has a tolerance."""
import copy
import pathlib
import struct
import subprocess

import numpy as np
import pytest

import local_mapping_model as model
import local_mapping_scenes as scenes
import orbslam_jpminipc_amd as orb
import scenes as S
from oracle_lib import OracleMatcher
from orbslam_jpminipc_amd import mappoint
from orbslam_jpminipc_amd._native import KEYPOINT_DTYPE, ORB_EINVAL, ORB_ENOTSUP, OrbError
from orbslam_jpminipc_amd.views import FeatureVector, View

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parents[1]
f32 = np.float32
_cache = {}


def lm():
    if "lm" not in _cache:
        _cache["lm"] = orb.LocalMapping(0)
    return _cache["lm"]


def accept(m=130, n1=147, n2=139, **kw):
    key = ("accept", m, n1, n2, tuple(sorted(kw.items())))
    if key not in _cache:
        _cache[key] = scenes.accept_scene(m, n1, n2, **kw)
    return _cache[key]


def gates():
    if "gates" not in _cache:
        _cache["gates"] = scenes.gates_scene()
    return _cache["gates"]


def run(V1, V2, m12, pos2=None, has2=None):
    got = lm().triangulate(V1, V2, m12, pos2, has2)
    with np.errstate(all="ignore"):
        want = model.create(V1, V2, m12, pos2, has2)
    model.same_result(got, want)
    return got, want


def with_table(V, **tables):
    """A copy of the view with entries of its level tables replaced: sigma2={level: value}, sf={...}."""
    W = copy.copy(V)
    W.mvLevelSigma2, W.mvScaleFactors = V.mvLevelSigma2.copy(), V.mvScaleFactors.copy()
    for lvl, v in tables.get("sigma2", {}).items():
        W.mvLevelSigma2[lvl] = v
    for lvl, v in tables.get("sf", {}).items():
        W.mvScaleFactors[lvl] = v
    return W


@pytest.mark.parametrize("m,n1,n2", [(0, 147, 139), (1, 147, 139), (63, 147, 139), (64, 147, 139), (65, 147, 139),
                                     (130, 147, 139), (255, 300, 290), (256, 300, 290), (257, 300, 290)])
def test_sizes(m, n1, n2):
    """Matches per pair around the wave and the workgroup (256 lanes); the second keyframe permuted, so
    ordinal, idx1 and idx2 all differ."""
    s = accept(m, n1, n2)
    got, _ = run(s["V1"], s["V2"], s["match12"])
    assert got["n_new"] == m and (got["status"] != 0).sum() == m
    assert np.array_equal(got["new_idx1"], s["idx1"]) and np.array_equal(got["new_idx2"], s["idx2"])
    if m > 1:
        assert not np.array_equal(s["idx1"], np.arange(m)) and not np.array_equal(s["idx1"], s["idx2"])


def test_every_gate_and_the_dense_lists():
    s = gates()
    got, _ = run(s["V1"], s["V2"], s["match12"])
    c = np.bincount(got["status"], minlength=10)
    assert c[1] >= 20 and all(c[k] >= 3 for k in (2, 4, 5, 6, 7, 9))
    acc = np.flatnonzero(got["status"] == 1)
    assert np.array_equal(got["new_idx1"], acc) and np.all(np.diff(got["new_idx1"]) > 0)
    assert np.array_equal(got["new_idx2"], s["match12"][acc])
    assert np.isnan(got["cos_rays"][s["match12"] < 0]).all() and not np.isnan(got["cos_rays"][s["match12"] >= 0]).any()
    assert not got["x3d"][np.isin(got["status"], (0, 2))].any() and got["x3d"][got["status"] >= 4].any(1).all()


def test_golden_fixture():
    g = dict(np.load(ROOT / "tests" / "golden" / "local_mapping.npz"))
    for name in ("accept", "gates"):
        V = [View(g[f"{name}.kps{v}"], np.zeros((len(g[f"{name}.kps{v}"]), 32), np.uint8), (0, 640, 0, 480),
                  scenes.NLEVELS, 1.2, scenes.CALIB, g[f"{name}.pose{v}"][:9], g[f"{name}.pose{v}"][9:], g[f"{name}.Ow{v}"])
             for v in "12"]
        got = lm().triangulate(V[0], V[1], g[f"{name}.match12"], g[f"{name}.mp_pos2"], g[f"{name}.has_mp2"])
        want = {k: g[f"{name}.{k}"] for k in model.EXACT_KEYS}
        for k in ("n_new", "skipped"):
            want[k] = int(want[k])
        want["median_depth"] = float(want["median_depth"])
        model.same_result(got, want)
        assert model.same_bits(lm().compute_f12(V[0], V[1]), g[f"{name}.F12"])


@pytest.mark.parametrize("image", [1, 2])
def test_reprojection_gate_is_exact_and_strict(image):
    """sigma2 of the match's level set to the largest float with 5.991*sigma2 < e rejects the match, the
    next float up accepts it: `>` against a double product, in both images."""
    s = accept()
    V = {1: s["V1"], 2: s["V2"]}
    base = model.create(s["V1"], s["V2"], s["match12"])
    i1 = int(s["idx1"][40])
    kp = s["V1"].kps[i1] if image == 1 else s["V2"].kps[s["match12"][i1]]
    e = float(base["dbg"][i1, image - 1])
    assert base["status"][i1] == 1 and e > 0
    lo = f32(e / 5.991)
    while 5.991 * float(lo) >= e:
        lo = np.nextafter(lo, f32(0))
    while 5.991 * float(np.nextafter(lo, f32(np.inf))) < e:
        lo = np.nextafter(lo, f32(np.inf))
    hi = np.nextafter(lo, f32(np.inf))
    assert 5.991 * float(lo) < e <= 5.991 * float(hi)
    for sig, st in ((lo, 5 + image), (hi, 1)):
        W = dict(V)
        W[image] = with_table(V[image], sigma2={int(kp["octave"]): sig})
        got, _ = run(W[1], W[2], s["match12"])
        assert got["status"][i1] == st


@pytest.mark.parametrize("side", ["low", "high"])
def test_scale_ratio_gate_at_its_boundary(side):
    """The neighbour's scale factor of the match's level moved across the float at which ratioDist*ratioFactor
    < ratioOctave (low) or ratioDist > ratioOctave*ratioFactor (high) changes: rejected on one side, accepted
    on the other, as the model says."""
    s = accept()
    V1, V2 = s["V1"], s["V2"]
    base = model.create(V1, V2, s["match12"])
    i1 = int(s["idx1"][77])
    o1, o2 = int(V1.kps[i1]["octave"]), int(V2.kps[s["match12"][i1]]["octave"])
    rd, rf, a = f32(base["dbg"][i1, 2]), f32(1.5) * V1.mvScaleFactors[1], V1.mvScaleFactors[o1]
    assert base["status"][i1] == 1

    def rejected(x):
        ro = a / f32(x)
        return bool(rd * rf < ro or rd > ro * rf)

    x = f32(a / (rd * rf)) if side == "low" else f32(a * rf / rd)
    cand = [x]
    for _ in range(64):
        cand = [np.nextafter(cand[0], f32(0))] + cand + [np.nextafter(cand[-1], f32(np.inf))]
    flips = [(p, q) for p, q in zip(cand, cand[1:]) if rejected(p) != rejected(q)]
    assert flips, "no boundary within 64 floats of the estimate"
    p, q = flips[0]
    seen = []
    for x in (p, q):
        got, _ = run(V1, with_table(V2, sf={o2: x}), s["match12"])
        assert got["status"][i1] == (9 if rejected(x) else 1)
        seen.append(int(got["status"][i1]))
    assert sorted(seen) == [1, 9]


def parallax_scene(baseline):
    """130 points about 25 baselines deep, where cosParallaxRays is about 0.9998."""
    rng = np.random.default_rng(77)
    R2, t2 = scenes.pose_at(scenes.R1, -scenes.R1.T @ scenes.T1 + scenes.R1.T @ np.array([baseline, 0.0, 0.0]))
    uvz = np.stack([rng.uniform(250, 400, 130), rng.uniform(200, 300, 130), 50 * 0.5 * rng.uniform(0.99, 1.01, 130)], 1)
    X = scenes.world_of(scenes.R1, scenes.T1, uvz)
    octs = np.zeros(130, np.int64)
    return scenes.make_pair(9, 147, 139, X, octs, octs, R2, t2, 0.0)


def test_parallax_gate_at_the_floats_around_its_threshold():
    """A baseline sweep, scanned with the model, for matches whose cosParallaxRays is the largest float not
    above 0.9998 and the next one: the first passes the gate, the second ends with code 2."""
    below = f32(0.9998)
    if float(below) > 0.9998:
        below = np.nextafter(below, f32(0))
    above = np.nextafter(below, f32(1))
    assert float(below) <= 0.9998 < float(above)
    found = {}
    for j in range(200):
        s = parallax_scene(0.5 + 1e-4 * j)
        c = model.create(s["V1"], s["V2"], s["match12"])["cos_rays"]
        for name, v in (("below", below), ("above", above)):
            if name not in found and (c == v).any():
                found[name] = (s, int(np.flatnonzero(c == v)[0]))
        if len(found) == 2:
            break
    assert len(found) == 2, f"the sweep found only {sorted(found)}"
    for name, (s, i1) in found.items():
        got, _ = run(s["V1"], s["V2"], s["match12"])
        assert got["cos_rays"][i1] == (below if name == "below" else above)
        assert (got["status"][i1] == 2) == (name == "above")


def test_baseline_gate_and_median():
    s, t = accept(), accept(baseline=0.02)
    pos, has = scenes.map_points_of(s["V2"], 3)
    got, _ = run(s["V1"], s["V2"], s["match12"], pos, has)
    assert got["skipped"] == 0 and got["n_new"] == 130
    z = model.median(s["V2"], pos, has)[0]
    assert got["median_depth"] == z and f32(lm().scene_median_depth(s["V2"], pos, has)) == z
    for q in (1, 3):
        assert f32(lm().scene_median_depth(s["V2"], pos, has, q)) == model.median(s["V2"], pos, has, q)[0]
    pos[5] = np.nan  # a NaN depth sorts last
    has[5] = 1
    assert np.isnan(lm().scene_median_depth(s["V2"], pos, has, 1))
    assert f32(lm().scene_median_depth(s["V2"], pos, has, 2)) == model.median(s["V2"], pos, has, 2)[0]
    pos2, has2 = scenes.map_points_of(t["V2"], 3)
    got, _ = run(t["V1"], t["V2"], t["match12"], pos2, has2)
    assert got["skipped"] == 1 and got["n_new"] == 0 and not got["status"].any()
    for call in (lambda: lm().triangulate(s["V1"], s["V2"], s["match12"], pos, np.zeros(s["V2"].n, np.uint8)),
                 lambda: lm().scene_median_depth(s["V2"], pos, np.zeros(s["V2"].n, np.uint8))):
        with pytest.raises(OrbError) as e:
            call()
        assert e.value.code == ORB_EINVAL


def batch_inputs(views, cap):
    import torch

    B = len(views)
    kps = np.zeros((B, cap), KEYPOINT_DTYPE)
    for b, V in enumerate(views):
        kps[b, :V.n] = V.kps
    d_kps = torch.from_numpy(kps.view(np.uint8).reshape(B, cap * 28).copy()).cuda()
    d_counts = torch.tensor([V.n for V in views], dtype=torch.int32).cuda()
    d_pose = torch.from_numpy(np.stack([model.pose12(V) for V in views])).cuda()
    return d_kps, d_counts, d_pose


def test_batch_of_three_pairs_and_host_parity():
    """P = 3, cap = 256: pair 0 triangulates, pair 1 is skipped by the baseline gate, pair 2 repeats pair 0's
    keyframes with no match.  The batch form computes the camera centres itself; the host form given the
    same centres answers the same."""
    import torch

    s, t = accept(), accept(baseline=0.02)
    assert np.array_equal(s["V1"].kps, t["V1"].kps)
    views = [copy.copy(V) for V in (s["V1"], s["V2"], t["V2"])]
    for V in views:
        V.Ow = model.center(model.pose12(V))
    cap, P = 256, 3
    pairs = [(0, 1), (0, 2), (0, 1)]
    rows = [s["match12"], t["match12"], np.full(147, -1, np.int32)]
    match = np.full((P, cap), -1, np.int32)
    mp_pos, has_mp = np.zeros((3, cap, 3), f32), np.zeros((3, cap), np.uint8)
    for p, r in enumerate(rows):
        match[p, :len(r)] = r
    for b, V in enumerate(views):
        mp_pos[b, :V.n], has_mp[b, :V.n] = scenes.map_points_of(V, 3)
    d_kps, d_counts, d_pose = batch_inputs(views, cap)
    o = lm().create_new_map_points_batch_device(
        d_kps, d_counts, cap, torch.tensor([a for a, _ in pairs], dtype=torch.int32).cuda(),
        torch.tensor([b for _, b in pairs], dtype=torch.int32).cuda(), torch.from_numpy(match).cuda(), d_pose,
        scenes.SF[:scenes.NLEVELS], scenes.SIGMA2[:scenes.NLEVELS], np.array(scenes.CALIB, f32),
        torch.from_numpy(mp_pos).cuda(), torch.from_numpy(has_mp).cuda())
    torch.cuda.synchronize()
    o = {k: v.cpu().numpy() for k, v in o.items()}
    assert list(o["skipped"]) == [0, 1, 0] and list(o["n_new"]) == [130, 0, 0]
    for p, (a, b) in enumerate(pairs):
        V1, V2 = views[a], views[b]
        want = model.create(V1, V2, rows[p], mp_pos[b, :V2.n], has_mp[b, :V2.n])
        n = want["n_new"]
        got = dict(x3d=o["x3d"][p, :V1.n], status=o["status"][p, :V1.n], cos_rays=o["cos_rays"][p, :V1.n],
                   n_new=int(o["n_new"][p]), new_idx1=o["new_idx1"][p, :n], new_idx2=o["new_idx2"][p, :n],
                   skipped=int(o["skipped"][p]), median_depth=float(o["median_depth"][p]))
        model.same_result(got, want)
        assert (o["new_idx1"][p, n:] == -1).all() and (o["new_idx2"][p, n:] == -1).all()  # rows written whole
        assert not o["status"][p, V1.n:].any() and np.isnan(o["cos_rays"][p, V1.n:]).all()
        assert model.same_bits(o["F12"][p], model.compute_f12(V1, V2))
        host = lm().triangulate(V1, V2, rows[p], mp_pos[b, :V2.n], has_mp[b, :V2.n])
        model.same_result(host, want)
    # a keyframe without a MapPoint: skipped = 2 in the batch form, nothing triangulated
    o2 = lm().create_new_map_points_batch_device(
        d_kps, d_counts, cap, torch.tensor([0], dtype=torch.int32).cuda(), torch.tensor([1], dtype=torch.int32).cuda(),
        torch.from_numpy(match[:1]).cuda(), d_pose, scenes.SF[:scenes.NLEVELS], scenes.SIGMA2[:scenes.NLEVELS],
        np.array(scenes.CALIB, f32), torch.from_numpy(mp_pos).cuda(), torch.zeros((3, cap), dtype=torch.uint8).cuda())
    torch.cuda.synchronize()
    assert int(o2["skipped"][0]) == 2 and int(o2["n_new"][0]) == 0 and not o2["status"].any()
    assert np.isnan(float(o2["median_depth"][0]))
    # the median alone, one workgroup per keyframe
    d_depth, d_n = torch.zeros(3, dtype=torch.float32).cuda(), torch.zeros(3, dtype=torch.int32).cuda()
    lm().scene_median_depth_batch_device(d_counts, cap, d_pose, torch.from_numpy(mp_pos).cuda(),
                                         torch.from_numpy(has_mp).cuda(), 2, d_depth, d_n)
    torch.cuda.synchronize()
    for b, V in enumerate(views):
        z, n = model.median(V, mp_pos[b, :V.n], has_mp[b, :V.n])
        assert d_depth[b].item() == z and d_n[b].item() == n


def test_nan_pose():
    """The batch form cannot see its poses: a NaN one returns and equals the model (a NaN fails no
    comparison).  The host form refuses it, naming the argument."""
    import torch

    s = accept()
    views = [copy.copy(s["V1"]), copy.copy(s["V2"])]
    views[1].tcw = views[1].tcw.copy()
    views[1].tcw[1] = np.nan
    for V in views:
        V.Ow = model.center(model.pose12(V))
    cap = 256
    match = np.full((1, cap), -1, np.int32)
    match[0, :147] = s["match12"]
    d_kps, d_counts, d_pose = batch_inputs(views, cap)
    o = lm().create_new_map_points_batch_device(
        d_kps, d_counts, cap, torch.tensor([0], dtype=torch.int32).cuda(), torch.tensor([1], dtype=torch.int32).cuda(),
        torch.from_numpy(match).cuda(), d_pose, scenes.SF[:scenes.NLEVELS], scenes.SIGMA2[:scenes.NLEVELS],
        np.array(scenes.CALIB, f32))
    torch.cuda.synchronize()
    o = {k: v.cpu().numpy() for k, v in o.items()}
    with np.errstate(all="ignore"):
        want = model.create(views[0], views[1], s["match12"])
    n = want["n_new"]
    got = dict(x3d=o["x3d"][0, :147], status=o["status"][0, :147], cos_rays=o["cos_rays"][0, :147], n_new=int(o["n_new"][0]),
               new_idx1=o["new_idx1"][0, :n], new_idx2=o["new_idx2"][0, :n], skipped=int(o["skipped"][0]),
               median_depth=float(o["median_depth"][0]))
    model.same_result(got, want)
    with pytest.raises(OrbError) as e:
        lm().triangulate(views[0], views[1], s["match12"])
    assert e.value.code == ORB_EINVAL and "KF2 tcw" in str(e.value)
    bad = copy.copy(s["V1"])
    bad.fx = f32(np.inf)
    with pytest.raises(OrbError) as e:
        lm().triangulate(bad, s["V2"], s["match12"])
    assert e.value.code == ORB_EINVAL and "fx" in str(e.value)


def test_limits():
    s = accept()
    big = View(np.zeros(8193, KEYPOINT_DTYPE), np.zeros((8193, 32), np.uint8), (0, 640, 0, 480), 8, 1.2, scenes.CALIB,
               scenes.R1, scenes.T1)
    with pytest.raises(OrbError) as e:
        lm().triangulate(big, s["V2"], np.full(8193, -1, np.int32))
    assert e.value.code == ORB_ENOTSUP
    with pytest.raises(OrbError) as e:
        lm().triangulate(s["V1"], s["V2"], np.where(s["match12"] >= 0, 139, -1))
    assert e.value.code == ORB_EINVAL
    one = View(s["V1"].kps, s["V1"].desc, (0, 640, 0, 480), 1, 1.2, scenes.CALIB, scenes.R1, scenes.T1)
    with pytest.raises(OrbError) as e:
        lm().triangulate(one, s["V2"], s["match12"])
    assert e.value.code == ORB_ENOTSUP


def neighbourhood():
    """A current keyframe and three neighbours of about 300 keypoints over 220 common world points, built
    from tests/scenes.py; the third neighbour stands 2 cm from the current keyframe."""
    rng = np.random.default_rng(5)
    n_pts, n = 220, 300
    Rc, tc = S.rot(rng, 0.05), rng.uniform(-0.1, 0.1, 3)
    base = View(np.zeros(0, KEYPOINT_DTYPE), np.zeros((0, 32), np.uint8), (0, S.W, 0, S.H), S.NLEVELS, 1.2, S.CALIB, Rc, tc)
    P = S.backproject(base, rng.uniform(30, S.W - 30, n_pts), rng.uniform(30, S.H - 30, n_pts), rng.uniform(3, 7, n_pts))
    d0, octs = S.descriptors(rng, n_pts), rng.integers(0, 4, n_pts)
    node = np.arange(n_pts) % 40
    out = []
    centre = -Rc.T @ tc
    for shift in ((0, 0, 0), (0.5, 0.02, 0.0), (-0.45, 0.05, 0.03), (0.02, 0.0, 0.0)):
        R = Rc @ S.rot(rng, 0.03)
        t = -R @ (centre + Rc.T @ np.array(shift))
        V0 = View(np.zeros(0, KEYPOINT_DTYPE), np.zeros((0, 32), np.uint8), (0, S.W, 0, S.H), S.NLEVELS, 1.2, S.CALIB, R, t)
        pu, pv, _ = S.project(V0, P)
        k = S.keypoints(rng, n)
        idx = rng.permutation(n)[:n_pts]
        k["x"][idx], k["y"][idx] = pu + rng.normal(0, 0.4, n_pts), pv + rng.normal(0, 0.4, n_pts)
        k["octave"][idx] = octs
        k["size"] = 31 * S.SF[k["octave"]]
        k["angle"][idx] = (f32(rng.uniform(0, 360)) + rng.normal(0, 5, n_pts)).astype(f32) % 360
        dsc = S.descriptors(rng, n)
        dsc[idx] = S.perturb(rng, d0, 30)
        assign = rng.integers(0, 40, n)
        assign[idx] = node
        fv, _, _ = S.feature_vector(rng, n, node_ids=np.arange(40) * 7 + 3, assign=assign)
        V = View(k, dsc, (0, S.W, 0, S.H), S.NLEVELS, 1.2, S.CALIB, R, t)
        out.append((V, fv))
    return out


def test_create_new_map_points_neighbour_loop():
    """The reference's loop over three neighbours against the same loop over the model and the oracle's
    SearchForTriangulation.  A slot that neighbour 0 filled is not matched again by neighbour 1, although
    it would be without the update; the third neighbour is skipped by the baseline gate."""
    (cur, cur_fv), *nb = neighbourhood()
    has0 = (np.random.default_rng(1).random(cur.n) < 0.2).astype(np.uint8)
    neighbours = [(V, fv, *scenes.map_points_of(V, 10 + i)) for i, (V, fv) in enumerate(nb)]
    results, has_end = lm().create_new_map_points(cur, cur_fv, has0, neighbours)
    has1 = has0.copy()
    oracle = OracleMatcher(0.6, False)
    for i, ((V2, fv2, pos2, has2), got) in enumerate(zip(neighbours, results)):
        gate = model.create(cur, V2, np.full(cur.n, -1, np.int32), pos2, has2)
        assert got["skipped"] == gate["skipped"] == (1 if i == 2 else 0)
        if gate["skipped"]:
            assert got["match12"] is None and got["n_new"] == 0
            continue
        F12 = model.compute_f12(cur, V2)
        assert model.same_bits(got["F12"], F12)
        _, m12 = oracle.SearchForTriangulation(cur, has1, cur_fv, V2, has2, fv2, F12)
        assert np.array_equal(got["match12"], m12)
        want = model.create(cur, V2, m12)
        want["median_depth"] = gate["median_depth"]
        model.same_result(got, want)
        if i == 1:
            filled = results[0]["new_idx1"]
            assert len(filled) >= 50 and (m12[filled] == -1).all()
            _, free = oracle.SearchForTriangulation(cur, has0, cur_fv, V2, has2, fv2, F12)
            assert (free[filled] >= 0).any()  # the dependence is real
        has1[want["new_idx1"]] = 1
    assert np.array_equal(has_end, has1)
    # a neighbour without a MapPoint is reported skipped = 2 and does not stop the loop
    V2, fv2, pos2, _ = neighbours[0]
    res, _ = lm().create_new_map_points(cur, cur_fv, has0, [(V2, fv2, pos2, np.zeros(V2.n, np.uint8)), neighbours[0]])
    assert res[0]["skipped"] == 2 and np.isnan(res[0]["median_depth"]) and res[0]["n_new"] == 0
    model.same_result({k: res[1][k] for k in model.EXACT_KEYS}, {k: results[0][k] for k in model.EXACT_KEYS})


@pytest.mark.parametrize("which", ["gates", "short_baseline"])
def test_native_facade(tmp_path, which):
    """The facade binary against the Python path, without and with the baseline gate's inputs; on the
    short-baseline pair the gated call returns false and creates nothing."""
    exe = ROOT / "build" / "local_mapping_facade"
    if not exe.exists():  # build() makes it; a tree that skipped build() compiles it here (g++, seconds)
        import __graft_entry__ as ge

        exe.parent.mkdir(exist_ok=True)
        subprocess.run(ge.LOCAL_MAPPING_FACADE_CMD(exe), check=True)
    s = gates() if which == "gates" else accept(baseline=0.02)
    V1, V2 = s["V1"], s["V2"]
    pos2, has2 = scenes.map_points_of(V2, 3)
    g = dict(np.load(ROOT / "tests" / "golden" / "local_mapping.npz"))
    off, ow, pos, ref, lev = (g[f"points.{k}"] for k in ("offsets", "obs_Ow", "pos", "ref_Ow", "ref_level"))
    sf, s2 = scenes.SF[:scenes.NLEVELS], scenes.SIGMA2[:scenes.NLEVELS]
    cams = b"".join(model.K4(V).tobytes() + model.pose12(V).tobytes() + V.Ow.astype(f32).tobytes() for V in (V1, V2))
    path = tmp_path / "case.bin"
    path.write_bytes(struct.pack("<5i", V1.n, V2.n, scenes.NLEVELS, len(lev), len(ow)) + cams + sf.tobytes() + s2.tobytes() +
                     V1.kps.tobytes() + V2.kps.tobytes() + s["match12"].tobytes() + off.tobytes() + ow.tobytes() +
                     pos.tobytes() + ref.tobytes() + lev.tobytes() + pos2.tobytes() + has2.tobytes())
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "local mapping facade OK" in r.stdout and "FAIL" not in r.stdout, r.stdout + r.stderr

    def fsum(v):
        w = np.ascontiguousarray(v, f32).reshape(-1).view(np.uint32).astype(np.uint64)
        return sum((i + 1) * int(x) for i, x in enumerate(w)) % (1 << 32)

    py = lm().triangulate(V1, V2, s["match12"])
    F = lm().compute_f12(V1, V2)
    ps = sum((2 * k + 1) * int(a) + (2 * k + 2) * int(b) for k, (a, b) in enumerate(zip(py["new_idx1"], py["new_idx2"])))
    ss = sum((k + 1) * int(v) for k, v in enumerate(py["status"]))
    n, dmin, dmax = mappoint.update_normal_and_depth(off, ow, pos, ref, lev, sf)
    lines = r.stdout.splitlines()
    assert lines[0] == "f12 " + " ".join(f"{x:08x}" for x in F.reshape(-1).view(np.uint32))
    assert lines[1] == (f"create go=1 n={py['n_new']} pairs={ps % (1 << 32)} x3d={fsum(py['x3d'][py['new_idx1']])} "
                        f"status={ss % (1 << 32)}")
    gated = lm().triangulate(V1, V2, s["match12"], pos2, has2)
    assert gated["skipped"] == (0 if which == "gates" else 1)
    assert lines[2] == (f"gated go={1 - gated['skipped']} n={gated['n_new']} "
                        f"x3d={fsum(gated['x3d'][gated['new_idx1']])}")
    assert lines[3] == f"update normal={fsum(n)} dmin={fsum(dmin)} dmax={fsum(dmax)}"
