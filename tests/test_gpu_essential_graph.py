"""GPU parity of Optimizer::OptimizeEssentialGraph (csrc/orb_essgraph.hip: orb_optimize_essential_graph and
orb_sim3_correct_points) against the CPU model (tests/native/essential_graph_model.cpp).

The structure counts (active and free vertices, edges, profile bytes) are compared exactly in every case.
The iteration and trial counters and the per-trial accept flags are compared exactly where the model
says every trial was decisive (asserted for the n_iterations = 1 and 3 cases, which keep the margin by
construction).  Estimates, poses, points and the final chi2 are compared within tolerances that are 100 x
the model's own spread, and the float outputs must be the rounding of the f64 ones, bit for bit.  The
shapes are the smallest that reach each edge of the kernels: the factor's panel of 4 block columns, a
workgroup's share of 8 block rows, full-width rows, 256-point workgroups."""
import pathlib
import subprocess

import numpy as np
import pytest

import orbslam_jpminipc_amd as orb
from orbslam_jpminipc_amd.optimizer import EG_MAX_PROFILE_BYTES
import essential_graph_model as egm
import essential_graph_scenes as egs

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parents[1]
f32 = np.float32
# 100 x the model's own spread over the listed cases and the fixture, rounded down to one
# digit (1.831e-6 in a Sim3 entry, 3.058e-6 in a pose entry, 6.362e-8 of the scene's scale in a point
# coordinate, 1.333e-7 of the starting chi2 in the final chi2, between its three sum orders and between its
# -ffp-contract=off and -ffp-contract=fast -mfma builds; scripts/gen_essential_graph_golden.py --spread).
SIM3_TOL = 1.0e-4
POSE_TOL = 3.0e-4
POINT_TOL = 6.0e-6  # of the scene's scale
CHI2_TOL = 1.0e-5   # of the chi2 the run started from
_worst = {"sim3": 0.0, "pose": 0.0, "point": 0.0, "chi2": 0.0}

TABLES = ("kf_corrected", "kf_has_corrected", "kf_noncorrected", "kf_has_noncorrected", "pt_pos", "pt_ref", "pt_skip")


@pytest.fixture(scope="module")
def opt():
    return orb.Optimizer(0)


def run(opt, g, n_iterations=20, **kw):
    return opt.OptimizeEssentialGraph(g["kf_pose"], g["kf_fixed"], g["edge_i"], g["edge_j"], g["edge_kind"],
                                      **{k: g.get(k) for k in TABLES}, n_iterations=n_iterations, **kw)


def same_structure(got, want, what):
    gi, wi = got["info"], want["info"]
    assert gi["status"] == 0, what
    for k in ("n_active", "n_free", "n_edges", "profile_bytes"):
        assert gi[k] == wi[k], f"{what}: {k}"
    assert np.array_equal(got["kf_pose"], got["kf_pose_f64"].astype(f32)), f"{what}: kf_pose_out != float32(f64)"
    assert np.array_equal(got["pt_pos"], got["pt_pos_f64"].astype(f32)), f"{what}: pt_pos_out != float32(f64)"
    assert np.isfinite(got["kf_sim3"]).all() and np.isfinite(got["pt_pos_f64"]).all(), what


def same_counters(got, want, what):
    gi, wi = got["info"], want["info"]
    for k in ("iterations", "trials", "refused", "trial_accepted"):
        assert gi[k] == wi[k], f"{what}: {k}: {gi[k]} != {wi[k]}"


def same_as_model(got, want, scale, what="", exact=False):
    same_structure(got, want, what)
    before = max(want["info"]["chi2_before"], np.finfo(float).tiny)
    ds = float(np.abs(got["kf_sim3"] - want["kf_sim3"]).max(initial=0.0))
    dp = float(np.abs(got["kf_pose_f64"] - want["kf_pose_f64"]).max(initial=0.0))
    dx = float(np.abs(got["pt_pos_f64"] - want["pt_pos_f64"]).max(initial=0.0)) / scale
    dc = abs(got["info"]["chi2_after"] - want["info"]["chi2_after"]) / before
    d0 = abs(got["info"]["chi2_before"] - want["info"]["chi2_before"]) / before
    for k, v in (("sim3", ds), ("pose", dp), ("point", dx), ("chi2", max(dc, d0))):
        _worst[k] = max(_worst[k], v)
    print(f"{what}: sim3 deviation {ds:.3e}, pose {dp:.3e}, point {dx:.3e}, chi2 {dc:.3e} / start {d0:.3e}; trials "
          f"{got['info']['trials']} (model {want['info']['trials']}); worst so far " +
          ", ".join(f"{k} {v:.3e}" for k, v in _worst.items()))
    assert ds <= SIM3_TOL, f"{what}: a Sim3 entry off by {ds:.3e}"
    assert dp <= POSE_TOL, f"{what}: a pose entry off by {dp:.3e}"
    assert dx <= POINT_TOL, f"{what}: a point coordinate off by {dx:.3e} of the scale"
    assert dc <= CHI2_TOL and d0 <= CHI2_TOL, f"{what}: chi2 off by {dc:.3e} / {d0:.3e}"
    if exact or egm.decisive_trials(want):
        same_counters(got, want, what)


@pytest.mark.parametrize("name", list(egs.CASES))
def test_case(opt, name):
    g, want, n_it, exact = egs.case(name)
    if exact:
        assert egm.decisive_trials(want), name
    same_as_model(run(opt, g, n_it), want, g["scale"], name, exact)


@pytest.mark.parametrize("n_pt", [0, 1, 255, 256, 257, 5000])
def test_points(opt, n_pt):
    base, _, _, _ = egs.case("ring_20")
    g = egs.with_points(base, n_pt)
    want = egm.run(g)
    got = run(opt, g)
    same_as_model(got, want, g["scale"], f"points_{n_pt}")
    unref = g["pt_ref"] == -1
    skipped = g["pt_skip"] != 0
    assert got["pt_pos"][unref].tobytes() == g["pt_pos"][unref].tobytes()  # pt_ref == -1: bit for bit
    assert got["pt_pos"][skipped].tobytes() == g["pt_pos"][skipped].tobytes()  # skipped: not written
    if n_pt == 5000:
        assert unref.sum() >= 100 and skipped.sum() >= 100 and len(set(g["pt_ref"].tolist())) == 21


def test_sim3_correct_points_alone(opt):
    rng = np.random.default_rng(3)
    g, want, _, _ = egs.case("ring_20")
    n_pair = len(g["kf_pose"])
    frm = np.stack([egm.from_pose(p) for p in g["kf_pose"]])
    to = want["kf_sim3"]
    for n_pt in (1, 257, 1000):
        pos = rng.uniform(-5, 5, (n_pt, 3)).astype(f32)
        pair = rng.integers(-1, n_pair, n_pt).astype(np.int32)
        pair[0] = -1
        got = opt.sim3_correct_points(pos, pair, frm, to)
        w32, w64 = egm.correct_points(pos, pair, frm, to)
        assert got["pt_pos"][pair == -1].tobytes() == pos[pair == -1].tobytes()
        assert got["pt_pos_f64"][pair == -1].tobytes() == pos[pair == -1].astype(np.float64).tobytes()
        assert np.array_equal(got["pt_pos"], got["pt_pos_f64"].astype(f32))
        # no libm call on this path: + - * / only, -ffp-contract=off on both sides
        assert got["pt_pos_f64"].tobytes() == w64.tobytes() and got["pt_pos"].tobytes() == w32.tobytes()
    with pytest.raises(orb.OrbError):
        opt.sim3_correct_points(pos, np.full(n_pt, n_pair, np.int32), frm, to)
    bad = to.copy()
    bad[3, 7] = 0.0
    with pytest.raises(orb.OrbError):
        opt.sim3_correct_points(pos, pair, frm, bad)


def _refused(opt, g, code, **kw):
    with pytest.raises(orb.OrbError) as e:
        run(opt, g, **kw)
    assert e.value.code == code, (e.value.code, str(e.value))
    return str(e.value)


def test_refusals(opt):
    g, _, _, _ = egs.case("chain_free_3")
    for key, val in (("kf_fixed", np.zeros(4, np.uint8)),  # no fixed vertex
                     ("edge_j", np.int32([0, 2, 2])),       # a self-edge
                     ("edge_i", np.int32([1, 2, 4])),       # an index out of range
                     ("edge_i", np.int32([1, -1, 3])),
                     ("edge_kind", np.uint8([1, 2, 1]))):   # a bad kind
        bad = dict(g)
        bad[key] = val
        _refused(opt, bad, egm.EINVAL)
        assert egm.run(bad)["status"] == egm.EINVAL
    bad = dict(g)
    bad["kf_pose"] = g["kf_pose"].copy()
    bad["kf_pose"][2, 5] = np.nan
    assert "kf_pose" in _refused(opt, bad, egm.EINVAL)
    bad = dict(g)
    bad["kf_corrected"] = g["kf_corrected"].copy()
    bad["kf_corrected"][1, 7] = 0.0
    assert "kf_corrected" in _refused(opt, bad, egm.EINVAL)
    bad["kf_corrected"][1, 7] = 1.0
    bad["kf_noncorrected"] = g["kf_noncorrected"].copy()
    bad["kf_noncorrected"][3, 2] = np.inf
    assert "kf_noncorrected" in _refused(opt, bad, egm.EINVAL)


def test_profile_cap_refused_without_allocating(opt):
    """20000 keyframes whose every late vertex names vertex 1: a profile of about 78 GB.  The refusal
    comes from the structure alone (an allocation of that size would fail with ORB_ENOMEM instead)."""
    n = 20000
    pose = np.tile(np.concatenate([np.eye(3).reshape(9), np.zeros(3)]).astype(f32), (n, 1))
    fixed = np.zeros(n, np.uint8)
    fixed[0] = 1
    late = np.arange(2, n, dtype=np.int32)
    g = {"kf_pose": pose, "kf_fixed": fixed, "edge_i": np.concatenate([np.int32([1]), late]),
         "edge_j": np.concatenate([np.int32([0]), np.ones(n - 2, np.int32)]), "edge_kind": np.ones(n - 1, np.uint8)}
    msg = _refused(opt, g, egm.ENOTSUP)
    assert "profile" in msg
    assert (n - 2) * (n - 1) // 2 * 49 * 8 > EG_MAX_PROFILE_BYTES


def test_a_4096_keyframe_structure_fits_the_cap():
    g, res = egs.ring(4096, n_corrected=4, n_loop_to=3, seed=1, n_iterations=0)
    assert 0 < res["info"]["profile_bytes"] < EG_MAX_PROFILE_BYTES // 4


def test_null_outputs_and_zero_iterations(opt):
    g, want, _, _ = egs.case("ring_20")
    a = egm.graph_arrays(g)
    lib = opt._lib
    from orbslam_jpminipc_amd._native import check, ptr
    sim3 = np.zeros((len(a["kf_pose"]), 8))
    args = [len(a["kf_pose"]), ptr(a["kf_pose"]), ptr(a["kf_corrected"]), ptr(a["kf_has_corrected"]), None, None,
            ptr(a["kf_fixed"]), len(a["edge_i"]), ptr(a["edge_i"]), ptr(a["edge_j"]), ptr(a["edge_kind"]), len(a["pt_pos"]),
            ptr(a["pt_pos"]), ptr(a["pt_ref"]), None, 20]
    check(lib.orb_optimize_essential_graph(*args, None, None, None, None, None, None, 0))
    check(lib.orb_optimize_essential_graph(*args, ptr(sim3), None, None, None, None, None, 0))
    g2 = dict(g)
    g2["kf_noncorrected"] = g2["kf_has_noncorrected"] = g2["pt_skip"] = None
    ref = run(opt, g2)
    assert sim3.tobytes() == ref["kf_sim3"].tobytes()
    # n_iterations == 0 and n_edge == 0: the inputs after the round trip, the points through it
    for h in (run(opt, g, 0), run(opt, dict(g, edge_i=np.zeros(0, np.int32), edge_j=np.zeros(0, np.int32),
                                            edge_kind=np.zeros(0, np.uint8)))):
        m = egm.run(g, 0)
        assert h["info"]["iterations"] == 0 and h["info"]["trials"] == 0
        assert h["kf_sim3"].tobytes() == m["kf_sim3"].tobytes()
        assert h["kf_pose_f64"].tobytes() == m["kf_pose_f64"].tobytes()
        assert np.abs(h["pt_pos_f64"] - m["pt_pos_f64"]).max() <= 1e-12 * g["scale"]


def test_deterministic(opt):
    g, _, _, _ = egs.case("ring_64")
    a, b = run(opt, g), run(opt, g)
    for k in ("kf_sim3", "kf_pose", "kf_pose_f64", "pt_pos", "pt_pos_f64"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["info"] == b["info"]


def test_refused_solve(opt):
    g, _ = egs.constructed(3, [(1, 0, 1), (2, 1, 1)], corrected=[1, 2], seed=6)
    g["kf_corrected"] = g["kf_corrected"].copy()
    g["kf_corrected"][2, 4:7] = 1e160
    want, got = egm.run(g, 2), run(opt, g, 2)
    assert want["info"]["refused"] >= 1
    assert got["info"]["refused"] == want["info"]["refused"] and got["info"]["trials"] == want["info"]["trials"]
    assert got["info"]["trial_accepted"] == want["info"]["trial_accepted"]
    assert got["info"]["trial_chi2"][0] == np.finfo(np.float64).max
    assert got["kf_sim3"][1].tobytes() == np.ascontiguousarray(g["kf_corrected"][1]).tobytes()


def test_golden_fixture(opt):
    z = np.load(ROOT / "tests" / "golden" / "essential_graph_ring.npz")
    g = {k: z[k] for k in ("kf_pose", "kf_fixed", "edge_i", "edge_j", "edge_kind") + TABLES}
    got = run(opt, g, int(z["n_iterations"]))
    scale = float(z["scale"])
    assert [got["info"][k] for k in ("n_active", "n_free", "n_edges", "profile_bytes")] == z["model_counts"].tolist()
    assert np.abs(got["kf_sim3"] - z["model_kf_sim3"]).max() <= SIM3_TOL
    assert np.abs(got["kf_pose_f64"] - z["model_kf_pose_f64"]).max() <= POSE_TOL
    assert np.abs(got["pt_pos_f64"] - z["model_pt_pos_f64"]).max() <= POINT_TOL * scale
    assert abs(got["info"]["chi2_before"] - z["model_chi2"][0]) <= CHI2_TOL * z["model_chi2"][0]
    assert abs(got["info"]["chi2_after"] - z["model_chi2"][1]) <= CHI2_TOL * z["model_chi2"][0]


def _fnv(h, b):
    for x in b:
        h = ((h ^ x) * 16777619) & 0xFFFFFFFF
    return h


def test_cpp_facade(opt, tmp_path):
    g, _, _, _ = egs.case("ring_20")
    a = egm.graph_arrays(g)
    path = tmp_path / "graph.bin"
    with open(path, "wb") as f:
        f.write(np.int32([len(a["kf_pose"]), len(a["edge_i"]), len(a["pt_pos"]), 20]).tobytes())
        for k in ("kf_pose", "kf_fixed", "kf_corrected", "kf_has_corrected", "kf_noncorrected", "kf_has_noncorrected",
                  "edge_i", "edge_j", "edge_kind", "pt_pos", "pt_ref", "pt_skip"):
            f.write(a[k].tobytes())
    r = subprocess.run([str(ROOT / "build" / "essential_graph_facade"), str(path)], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "essential graph facade OK" in r.stdout, r.stdout
    got = run(opt, g)
    I = got["info"]
    lines = r.stdout.splitlines()
    assert lines[0] == (f"ESSGRAPH free={I['n_free']} iterations={I['iterations']} trials={I['trials']} "
                        f"refused={I['refused']} accepted={''.join(str(v) for v in I['trial_accepted'])}"), r.stdout
    assert lines[1] == (f"SIM3 {_fnv(2166136261, got['kf_sim3'].tobytes()):08x} POSES "
                        f"{_fnv(2166136261, got['kf_pose'].tobytes()):08x} POINTS "
                        f"{_fnv(2166136261, got['pt_pos'].tobytes()):08x}"), r.stdout
    frm = np.stack([egm.from_pose(p) for p in a["kf_pose"]])
    back = np.stack([egm.to_pose(s) for s in got["kf_sim3"]]).astype(f32)
    assert lines[2] == f"FROMPOSE {_fnv(2166136261, frm.tobytes()):08x} TOPOSE {_fnv(2166136261, back.tobytes()):08x}"
    assert back.tobytes() == got["kf_pose"].tobytes()
