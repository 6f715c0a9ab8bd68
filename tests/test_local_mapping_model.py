"""The CPU model of CreateNewMapPoints, ComputeF12, ComputeSceneMedianDepth and UpdateNormalAndDepth
(tests/native/local_mapping_model.cpp) against float64 mathematics, the Initializer's triangulation model,
and the golden fixture with its conditions.  No GPU."""
import importlib.util
import pathlib

import numpy as np
import pytest

import initializer_reconstruct_model as rec_model
import local_mapping_model as model
import local_mapping_scenes as scenes
import scenes as matcher_scenes
from orbslam_jpminipc_amd import _native

ROOT = pathlib.Path(__file__).resolve().parents[1]
GOLD_PATH = ROOT / "tests" / "golden" / "local_mapping.npz"


def generator():
    spec = importlib.util.spec_from_file_location("gen_local_mapping_golden", ROOT / "scripts" / "gen_local_mapping_golden.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_triangulated_points_are_the_scene_points():
    """Noise 0.3 px: every match is accepted and its point is the scene's.  Depth error z^2 d / (f b) with
    z <= 8, f = 520, b = 0.5 and a disparity error d up to 4 sigma sqrt(2) = 1.7 px: 64 * 1.7 / 260."""
    s = scenes.accept_scene()
    r = model.create(s["V1"], s["V2"], s["match12"])
    assert r["n_new"] == 130 and np.array_equal(r["new_idx1"], s["idx1"]) and np.array_equal(r["new_idx2"], s["idx2"])
    assert np.array_equal(r["status"] == 1, s["match12"] >= 0)
    assert np.abs(r["x3d"][s["idx1"]] - s["X"]).max() < 64 * 1.7 / 260
    unmatched = s["match12"] < 0
    assert not r["x3d"][unmatched].any() and np.isnan(r["cos_rays"][unmatched]).all()
    # the cosine is that of the true rays, to the pixel noise
    c1, c2 = s["V1"].Ow.astype(np.float64), s["V2"].Ow.astype(np.float64)
    a, b = s["X"] - c1, s["X"] - c2
    cos = (a * b).sum(1) / np.linalg.norm(a, axis=1) / np.linalg.norm(b, axis=1)
    assert np.abs(r["cos_rays"][s["idx1"]] - cos).max() < 1e-3


def test_noiseless_points_to_float_precision():
    """Without pixel noise the only error is the float32 pixel (2^-15 px at 512) and the float32 SVD: with
    the same depth formula, 64 / 260 m per px of disparity, 1e-3 px covers both with two decades to spare."""
    s = scenes.accept_scene(noise=0.0)
    r = model.create(s["V1"], s["V2"], s["match12"])
    assert r["n_new"] == 130
    assert np.abs(r["x3d"][s["idx1"]] - s["X"]).max() < 64 / 260 * 1e-3 * 10


def test_f12_annihilates_noiseless_correspondences():
    """x1^T F12 x2 = 0 on noiseless projections, relative to the size of the terms; and the matrix is the
    float64 one of tests/scenes.py to float precision."""
    s = scenes.accept_scene(noise=0.0)
    F = model.compute_f12(s["V1"], s["V2"]).astype(np.float64)
    k1, k2 = s["V1"].kps[s["idx1"]], s["V2"].kps[s["idx2"]]
    x1 = np.stack([k1["x"], k1["y"], np.ones(len(k1))], 1).astype(np.float64)
    x2 = np.stack([k2["x"], k2["y"], np.ones(len(k2))], 1).astype(np.float64)
    res = np.abs(np.einsum("ni,ij,nj->n", x1, F, x2))
    size = np.einsum("ni,ij,nj->n", np.abs(x1), np.abs(F), np.abs(x2))
    assert (res / size).max() < 1e-5  # float32 entries of F and of the pixels: a few 2^-24 per term
    F64 = matcher_scenes.fundamental12(s["V1"], s["V2"]).astype(np.float64)
    assert np.abs(F - F64).max() < 1e-5 * np.abs(F64).max()


def test_median_is_the_sorted_element():
    s = scenes.accept_scene()
    V = s["V2"]
    for seed, q in ((3, 2), (4, 2), (5, 3), (6, 1)):
        pos, has = scenes.map_points_of(V, seed)
        got, n = model.median(V, pos, has, q)
        R, t = V.Rcw.astype(np.float64), V.tcw.astype(np.float64)
        X = pos.astype(np.float64)[has != 0]
        z = ((R[2, 0] * X[:, 0] + R[2, 1] * X[:, 1] + R[2, 2] * X[:, 2]) + t[2]).astype(np.float32)
        assert n == len(z) and got == np.sort(z)[(n - 1) // q]
    got, n = model.median(V, pos, np.zeros(V.n, np.uint8))
    assert n == 0 and np.isnan(got)
    one = np.zeros(V.n, np.uint8)
    one[7] = 1
    assert model.median(V, pos, one)[1] == 1


def test_a_nan_depth_sorts_after_every_number():
    s = scenes.accept_scene()
    V = s["V2"]
    pos, _ = scenes.map_points_of(V, 3)
    has = np.zeros(V.n, np.uint8)
    has[:5] = 1
    pos[1] = np.nan
    zs = np.sort([model.median(V, pos, np.eye(V.n, dtype=np.uint8)[i])[0] for i in (0, 2, 3, 4)])
    assert model.median(V, pos, has, 2)[0] == zs[2]  # 5 depths, index 2: the third number
    assert np.isnan(model.median(V, pos, has, 1)[0])  # index 4: the NaN, last


def test_the_4x4_triangulation_is_the_initializers():
    """The same rows give the same bits as Initializer::Triangulate's model: one SVD, one reading."""
    s = scenes.gates_scene()
    V1, V2 = s["V1"], s["V2"]
    T = [np.concatenate([V.Rcw, V.tcw.reshape(3, 1)], 1).astype(np.float32) for V in (V1, V2)]
    rng = np.random.default_rng(0)
    for _ in range(50):
        xn1, xn2 = rng.uniform(-0.6, 0.6, 2).astype(np.float32), rng.uniform(-0.6, 0.6, 2).astype(np.float32)
        got = model.triangulate4(xn1, xn2, T[0], T[1])
        want = rec_model.triangulate(xn1, xn2, T[0], T[1])
        assert got is not None and model.same_bits(got, want)


def test_contraction_changes_a_reprojection_error_somewhere():
    """The fused multiply-adds are observable: the variant without them gives other squared errors."""
    s = scenes.gates_scene()
    a = model.create(s["V1"], s["V2"], s["match12"])["dbg"][:, :2]
    b = model.create(s["V1"], s["V2"], s["match12"], variant=2)["dbg"][:, :2]
    ok = ~np.isnan(a) & ~np.isnan(b)
    assert (a[ok] != b[ok]).any()


def test_baseline_gate():
    s = scenes.accept_scene(baseline=0.5)
    pos, has = scenes.map_points_of(s["V2"], 3)
    r = model.create(s["V1"], s["V2"], s["match12"], pos, has)
    assert r["skipped"] == 0 and r["n_new"] == 130 and r["median_depth"] == model.median(s["V2"], pos, has)[0]
    t = scenes.accept_scene(baseline=0.02)  # 0.02 / 5.4 < 0.01
    r = model.create(t["V1"], t["V2"], t["match12"], *scenes.map_points_of(t["V2"], 3))
    assert r["skipped"] == 1 and r["n_new"] == 0 and not r["status"].any()
    with pytest.raises(ValueError):
        model.create(s["V1"], s["V2"], s["match12"], pos, np.zeros(s["V2"].n, np.uint8))


def test_update_normal_and_depth_against_float64():
    off, ow, pos, ref, lev = generator().observations()
    n, dmin, dmax = model.update_normal_and_depth(off, ow, pos, ref, lev, scenes.SF[:scenes.NLEVELS])
    assert np.isnan(n[0]).all()  # no observation: 0 * inf
    sf = scenes.SF.astype(np.float64)
    for m in range(1, len(lev)):
        d = pos[m].astype(np.float64) - ow[off[m]:off[m + 1]].astype(np.float64)
        want = (d / np.linalg.norm(d, axis=1)[:, None]).mean(0)
        assert np.abs(n[m] - want).max() < 1e-6 * (off[m + 1] - off[m])
    dist = np.linalg.norm(pos.astype(np.float64) - ref.astype(np.float64), axis=1)
    assert np.allclose(dmin, dist / sf[1] / sf[lev], rtol=1e-6)
    assert np.allclose(dmax, dist * sf[1] * sf[scenes.NLEVELS - 1 - lev], rtol=1e-6)


def test_golden_fixture_regenerates_identically_and_meets_its_conditions():
    gen = generator()
    fresh = gen.build()
    gold = dict(np.load(GOLD_PATH))
    assert sorted(fresh) == sorted(gold)
    for k, v in fresh.items():
        g, v = gold[k], np.asarray(v)
        assert g.dtype == v.dtype and g.shape == v.shape, k
        same = model.same_bits(g, v) if v.dtype.kind == "f" else g.tobytes() == v.tobytes()
        assert same, k
    for name in ("accept", "gates"):
        assert gen.conditions(name, gold[f"{name}.status"]) is None
    c = np.bincount(gold["accept.status"], minlength=10)
    assert c[1] >= 0.9 * 130 and c[1:].sum() == 130
    c = np.bincount(gold["gates.status"], minlength=10)
    assert c[1] >= 20 and all(c[k] >= 3 for k in (2, 4, 5, 6, 7, 9)) and c[3] == 0 and c[8] == 0
    assert GOLD_PATH.stat().st_size < 1 << 20


def test_abi_declarations_match_the_binding_table_and_the_library():
    """Every new entry point: exported by the library, and its ctypes argument list is the header's
    parameter list, kind for kind (view pointer, other pointer, int, float), the 24 of the batch form
    included."""
    import ctypes
    import re

    import orbslam_jpminipc_amd as orb

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "orb_abi.h").read_text(), flags=re.S)
    lib = orb.hip_lib()
    counts = {}
    for name in ("orb_compute_f12", "orb_scene_median_depth", "orb_scene_median_depth_batch_device",
                 "orb_create_new_map_points", "orb_create_new_map_points_batch_device", "orb_update_normal_and_depth",
                 "orb_update_normal_and_depth_device"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, name
        want = []
        for p in (q.strip() for q in m.group(1).split(",")):
            if "*" in p:
                want.append(ctypes.POINTER(_native.FrameView) if "orb_frame_view_t" in p else ctypes.c_void_p)
            else:
                kind = p.split()[0]
                want.append({"int": ctypes.c_int, "float": ctypes.c_float}[kind])
        res, args = _native.HIP_SIGNATURES[name]
        assert res is ctypes.c_int and args == want, (name, len(args), len(want))
        fn = getattr(lib, name)  # AttributeError: the library does not export it
        assert fn.argtypes == want
        counts[name] = len(want)
    assert counts["orb_create_new_map_points_batch_device"] == 24 and counts["orb_create_new_map_points"] == 14
