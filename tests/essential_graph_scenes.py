"""Scenes for the essential-graph tests: a camera ring that returns to its start with a
Sim3 drift accumulated along it, closed as LoopClosing::CorrectLoop would close it, and small
constructed graphs for the edges of the kernels.  A scene is the dict that
``essential_graph_model.graph_arrays`` reads, plus "scale" (the ring's radius, what point and pose
tolerances are relative to) and "seed" (the seed it took).

The margins are a condition of a scene, not a measurement: from the model's own records every
evaluation of log() stays a relative LOG_MARGIN away from both eps tests, and (exact=True) every
trial's chi2 a relative TRIAL_MARGIN away from the chi2 it is compared with.  A generator moves to the
next seed otherwise, at most 20 times; the seeds that the listed cases took are in CASE_SEEDS, which
tests/test_essential_graph_model.py checks.
"""
from __future__ import annotations

import numpy as np

import essential_graph_model as egm

MAX_SEEDS = 20


def _rodrigues(w):
    th = float(np.linalg.norm(w))
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], float)
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)


def _pose12(T):
    return np.concatenate([T[:3, :3].reshape(9), T[:3, 3]]).astype(np.float32)


def _ring_poses(n, radius, rng):
    Ts = []
    for i in range(n):
        a = 2 * np.pi * i / n
        C = radius * np.array([np.cos(a), np.sin(a), 0.1 * np.sin(3 * a)])
        Rwc = _rodrigues(np.array([0, 0, a + np.pi / 2])) @ _rodrigues(np.array([-np.pi / 2, 0, 0]))
        Rwc = Rwc @ _rodrigues(rng.normal(0, 0.02, 3))
        T = np.eye(4)
        T[:3, :3] = Rwc.T
        T[:3, 3] = -Rwc.T @ C
        Ts.append(T)
    return Ts


def _ring(n_kf, n_corrected, n_loop_to, fixed, seed, rot_deg, scale_per_lap, trans_drift, pts_per_kf, radius, covis):
    rng = np.random.default_rng(seed)
    true = _ring_poses(n_kf, radius, rng)
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    g = (1 + scale_per_lap) ** (1.0 / n_kf)
    drift = [true[0]]
    for i in range(1, n_kf):
        rel = true[i] @ np.linalg.inv(true[i - 1])
        D = np.eye(4)
        D[:3, :3] = _rodrigues(np.deg2rad(rot_deg) / n_kf * axis * (1 + 0.1 * rng.normal())) @ rel[:3, :3]
        D[:3, 3] = g ** i * rel[:3, 3] + rng.normal(0, trans_drift * radius / n_kf, 3)
        drift.append(D @ drift[i - 1])
    kf_pose = np.stack([_pose12(T) for T in drift])
    c = n_kf - 1
    s = 1 + scale_per_lap
    Scw = egm.from_pose(_pose12(true[c]))
    Scw[4:7] *= s
    Scw[7] = s
    corr, nonc = np.zeros((n_kf, 8)), np.zeros((n_kf, 8))
    corr[:, 3] = nonc[:, 3] = corr[:, 7] = nonc[:, 7] = 1
    has = np.zeros(n_kf, np.uint8)
    Swc_drift = egm.inverse(egm.from_pose(kf_pose[c]))
    for i in range(max(n_kf - n_corrected, 1), n_kf):
        nonc[i] = egm.from_pose(kf_pose[i])
        corr[i] = egm.mul(egm.mul(nonc[i], Swc_drift), Scw)  # g2oSic * g2oScw
        has[i] = 1
    edges = []
    for i in range(max(n_kf - n_corrected, 1), n_kf):  # the loop connections, first
        for j in range(min(n_loop_to, i)):
            edges.append((i, j, 0))
    for i in range(1, n_kf):  # then per keyframe: the spanning tree, the covisibility graph
        edges.append((i, i - 1, 1))
        for b in covis:
            if i - b >= 0:
                edges.append((i, i - b, 1))
    kf_fixed = np.zeros(n_kf, np.uint8)
    kf_fixed[fixed] = 1
    e = np.array(edges, np.int32).reshape(-1, 3)
    n_pt = pts_per_kf * n_kf
    ref = np.repeat(np.arange(n_kf, dtype=np.int32), pts_per_kf)
    pos = np.zeros((n_pt, 3), np.float32)
    for p in range(n_pt):
        T = drift[ref[p]]
        Xc = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(1, 4)])
        pos[p] = (T[:3, :3].T @ (Xc - T[:3, 3])).astype(np.float32)
    skip = np.zeros(n_pt, np.uint8)
    if n_pt >= 10:
        ref[rng.choice(n_pt, n_pt // 10, replace=False)] = -1
        skip[rng.choice(n_pt, n_pt // 10, replace=False)] = 1
    return {"kf_pose": kf_pose, "kf_fixed": kf_fixed, "kf_corrected": corr, "kf_has_corrected": has,
            "kf_noncorrected": nonc, "kf_has_noncorrected": has.copy(), "edge_i": e[:, 0].copy(), "edge_j": e[:, 1].copy(),
            "edge_kind": e[:, 2].astype(np.uint8), "pt_pos": pos, "pt_ref": ref, "pt_skip": skip, "scale": radius,
            "seed": seed}


def _conditioned(make, seed, n_iterations, exact):
    """The first of `seed`, `seed` + 1, ... whose model run keeps the margins; (scene, model result)."""
    for k in range(MAX_SEEDS):
        g = make(seed + k)
        res = egm.run(g, n_iterations)
        assert res["status"] == 0, res["status"]
        if egm.decisive_log(res) and (not exact or egm.decisive_trials(res)):
            return g, res
    raise AssertionError(f"no seed in [{seed}, {seed + MAX_SEEDS}) keeps the margins")


def ring(n_kf, n_corrected=3, n_loop_to=2, fixed=0, seed=0, rot_deg=3.0, scale_per_lap=0.04, trans_drift=0.02,
         pts_per_kf=0, radius=5.0, covis=(2, 3), n_iterations=20, exact=False):
    """A ring of n_kf keyframes: the chain as the spanning tree, covisibility edges to the second and third
    predecessor, corrected Sim3s (scale 1 + scale_per_lap) on the last n_corrected keyframes and loop
    connections from those to the first n_loop_to; rot_deg is the seam's rotation (above 0.5: the acos
    branch of log() runs at the seam; below 0.1: the other one)."""
    return _conditioned(lambda s: _ring(n_kf, n_corrected, n_loop_to, fixed, s, rot_deg, scale_per_lap, trans_drift,
                                        pts_per_kf, radius, covis), seed, n_iterations, exact)


def _constructed(n_kf, edges, fixed, corrected, seed, radius, sigma):
    rng = np.random.default_rng(seed)
    true = _ring_poses(n_kf, radius, rng)
    kf_pose = np.stack([_pose12(T) for T in true])
    corr, nonc = np.zeros((n_kf, 8)), np.zeros((n_kf, 8))
    corr[:, 3] = nonc[:, 3] = corr[:, 7] = nonc[:, 7] = 1
    has = np.zeros(n_kf, np.uint8)
    for i in corrected:
        nonc[i] = egm.from_pose(kf_pose[i])
        u = rng.normal(0, 1, 7) * np.array([sigma, sigma, sigma, sigma * radius, sigma * radius, sigma * radius, sigma])
        corr[i] = egm.mul(egm.exp(u), nonc[i])
        has[i] = 1
    kf_fixed = np.zeros(n_kf, np.uint8)
    kf_fixed[list(fixed)] = 1
    e = np.array(edges, np.int32).reshape(-1, 3)
    return {"kf_pose": kf_pose, "kf_fixed": kf_fixed, "kf_corrected": corr, "kf_has_corrected": has,
            "kf_noncorrected": nonc, "kf_has_noncorrected": has.copy(), "edge_i": e[:, 0].copy(), "edge_j": e[:, 1].copy(),
            "edge_kind": e[:, 2].astype(np.uint8), "pt_pos": np.zeros((0, 3), np.float32),
            "pt_ref": np.zeros(0, np.int32), "pt_skip": None, "scale": radius, "seed": seed}


def constructed(n_kf, edges, fixed=(0,), corrected=None, seed=0, radius=5.0, sigma=0.02, n_iterations=20, exact=False):
    """n_kf keyframes on a ring with the given (i, j, kind) edge rows; the keyframes in `corrected` (None:
    every second one) carry a non-corrected entry (their pose) and a corrected one (a random Sim3 of
    size sigma away), which is where the kind-1 edges' errors come from."""
    if corrected is None:
        corrected = range(1, n_kf, 2)
    corrected = list(corrected)
    return _conditioned(lambda s: _constructed(n_kf, edges, fixed, corrected, s, radius, sigma), seed, n_iterations, exact)


def chain_edges(n_kf, kind=1):
    return [(i, i - 1, kind) for i in range(1, n_kf)]


def with_points(g, n_pt, seed=0):
    """`g` with n_pt points whose references are spread over all keyframes, a tenth of them -1 and a tenth
    skipped (from 10 points on)."""
    rng = np.random.default_rng(1000 + seed)
    n_kf = len(g["kf_pose"])
    out = dict(g)
    out["pt_ref"] = (np.arange(n_pt) * 7 % n_kf).astype(np.int32)
    out["pt_pos"] = rng.uniform(-g["scale"], g["scale"], (n_pt, 3)).astype(np.float32)
    out["pt_skip"] = np.zeros(n_pt, np.uint8)
    if n_pt >= 10:
        out["pt_ref"][rng.choice(n_pt, n_pt // 10, replace=False)] = -1
        out["pt_skip"][rng.choice(n_pt, n_pt // 10, replace=False)] = 1
    return out


# The panel of the factorisation is 4 block columns and a workgroup's share of the rows below it 8 block
# rows (csrc/orb_essgraph.hip): free-vertex counts one below, at and above each, with the fixed keyframe
# on top.  name -> (generator, n_iterations, exact: the counters are compared exactly)
PANEL_BLOCKS, SHARE_BLOCKS = 4, 8


def _chain(n_free, **kw):
    return lambda: constructed(n_free + 1, chain_edges(n_free + 1), **kw)


CASES = {
    "free_1_edge_1": (lambda: constructed(2, [(1, 0, 1)], corrected=[1], seed=3), 20, False),
    "free_2_chain": (_chain(2, seed=4), 20, False),
    "chain_free_3": (_chain(PANEL_BLOCKS - 1, seed=5), 20, False),
    "chain_free_4": (_chain(PANEL_BLOCKS, seed=6), 20, False),
    "chain_free_5": (_chain(PANEL_BLOCKS + 1, seed=7), 20, False),
    "chain_free_11": (_chain(PANEL_BLOCKS + SHARE_BLOCKS - 1, seed=8), 20, False),
    "chain_free_12": (_chain(PANEL_BLOCKS + SHARE_BLOCKS, seed=9), 20, False),
    "chain_free_13": (_chain(PANEL_BLOCKS + SHARE_BLOCKS + 1, seed=10), 20, False),
    "late_row_fixed_last": (lambda: constructed(10, chain_edges(10) + [(8, 0, 1)], fixed=(9,), seed=11), 20, False),
    "several_rows": (lambda: constructed(14, chain_edges(14) + [(13, 1, 1), (12, 1, 0), (11, 2, 1), (9, 1, 1)], seed=12),
                     20, False),
    "duplicate_pairs": (lambda: constructed(6, chain_edges(6) + [(3, 1, 1), (1, 3, 1), (3, 1, 0), (2, 1, 1)], seed=14,
                                            sigma=0.01),
                        20, False),
    "isolated_two_fixed": (lambda: constructed(8, [(1, 0, 1), (2, 1, 1), (3, 2, 1), (5, 3, 1), (6, 5, 1), (7, 6, 1)],
                                               fixed=(0, 6), corrected=[1, 2, 3, 4, 5, 7], seed=14), 20, False),
    "all_corrected": (lambda: constructed(6, chain_edges(6) + [(5, 2, 1)], corrected=range(6), seed=15), 20, False),
    "none_corrected": (lambda: constructed(6, chain_edges(6) + [(5, 2, 0)], corrected=[], seed=16), 20, False),
    "ring_20": (lambda: ring(20, seed=20, pts_per_kf=3), 20, False),
    "ring_20_small_rotation": (lambda: ring(20, seed=31, rot_deg=0.05), 20, False),
    "ring_20_fixed_2": (lambda: ring(20, seed=41, fixed=2, n_loop_to=4), 20, False),
    "ring_20_unit_scale": (lambda: ring(20, seed=50, scale_per_lap=0.0), 20, False),
    "ring_20_iterations_1": (lambda: ring(20, seed=62, n_iterations=1, exact=True), 1, True),
    "ring_20_iterations_3": (lambda: ring(20, seed=63, rot_deg=1.0, n_iterations=3, exact=True), 3, True),
    "ring_64": (lambda: ring(65, seed=70, n_corrected=4, n_loop_to=3, pts_per_kf=2), 20, False),
    "ring_257": (lambda: ring(258, seed=80, n_corrected=4, n_loop_to=3), 20, False),
}
GOLDEN_CASE = "ring_20"

# the seed each case took (its generator's own seed where the margins held at once); checked by
# tests/test_essential_graph_model.py::test_case_seeds
CASE_SEEDS = {
    "free_1_edge_1": 3, "free_2_chain": 4, "chain_free_3": 5, "chain_free_4": 6, "chain_free_5": 7, "chain_free_11": 8,
    "chain_free_12": 9, "chain_free_13": 10, "late_row_fixed_last": 11, "several_rows": 12, "duplicate_pairs": 14,
    "isolated_two_fixed": 14, "all_corrected": 15, "none_corrected": 16, "ring_20": 21, "ring_20_small_rotation": 31,
    "ring_20_fixed_2": 41, "ring_20_unit_scale": 50, "ring_20_iterations_1": 62, "ring_20_iterations_3": 63,
    "ring_64": 70, "ring_257": 80,
}

_cache = {}


def case(name):
    """(scene, model result, n_iterations, exact) of a listed case; the model runs once per process."""
    if name not in _cache:
        make, n_it, exact = CASES[name]
        g, res = make()
        _cache[name] = (g, res, n_it, exact)
    return _cache[name]
