#!/usr/bin/env python3
"""Writes tests/golden/local_mapping.npz: two small keyframe pairs (tests/local_mapping_scenes.py), a set
of map points with their observations, and the answers of the C++ model
(tests/native/local_mapping_model.cpp).

The generator refuses the fixture unless the "accept" scene yields status 1 for at least 90 % of its 130
matches, the "gates" scene holds at least 20 accepted matches and at least 3 each of the codes 2, 4, 5, 6,
7 and 9, and no scene reaches the codes 3 and 8 (`w == 0`, a zero distance: branches kept for fidelity
that no test exercises)."""
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import local_mapping_model as model  # noqa: E402
import local_mapping_scenes as scenes  # noqa: E402

OUT = ROOT / "tests" / "golden" / "local_mapping.npz"
KEYS = ("x3d", "status", "cos_rays", "n_new", "new_idx1", "new_idx2", "skipped", "median_depth")


def conditions(name, status):
    """The fixture conditions on the status row of scene `name`; a message, or None when they hold."""
    c = np.bincount(status, minlength=10)
    if c[3] or c[8]:
        return f"{name}: reaches code 3 or 8: {c}"
    if name == "accept" and (c[1:].sum() != 130 or c[1] < 0.9 * 130):
        return f"accept: {c[1]} of {c[1:].sum()} matches accepted, at least 90 % of 130 wanted"
    if name == "gates" and (c[1] < 20 or min(c[k] for k in (2, 4, 5, 6, 7, 9)) < 3):
        return f"gates: at least 20 accepted and 3 each of 2, 4, 5, 6, 7, 9 wanted: {c}"
    return None


def observations(seed=5, sizes=(0, 1, 2, 31, 7, 3)):
    """Map points with the given numbers of observations: offsets, obs_Ow, pos, ref_Ow, ref_level."""
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    M = len(sizes)
    pos = rng.uniform(-3, 3, (M, 3)).astype(np.float32) + np.float32([0, 0, 6])
    ow = rng.uniform(-1, 1, (int(off[-1]), 3)).astype(np.float32)
    ref = rng.uniform(-1, 1, (M, 3)).astype(np.float32)
    lev = rng.integers(0, scenes.NLEVELS, M).astype(np.int32)
    lev[:2] = (0, scenes.NLEVELS - 1)
    return off, ow, pos, ref, lev


def build() -> dict:
    out = {}
    for name, s in (("accept", scenes.accept_scene()), ("gates", scenes.gates_scene())):
        pos2, has2 = scenes.map_points_of(s["V2"], 3)
        r = model.create(s["V1"], s["V2"], s["match12"], pos2, has2)
        bad = conditions(name, r["status"])
        if bad:
            raise SystemExit(bad)
        if r["skipped"]:
            raise SystemExit(f"{name}: skipped by the baseline gate")
        for v, V in (("1", s["V1"]), ("2", s["V2"])):
            out[f"{name}.kps{v}"] = V.kps
            out[f"{name}.pose{v}"] = model.pose12(V)
            out[f"{name}.Ow{v}"] = V.Ow
        out[f"{name}.match12"] = s["match12"]
        out[f"{name}.mp_pos2"], out[f"{name}.has_mp2"] = pos2, has2
        out[f"{name}.F12"] = model.compute_f12(s["V1"], s["V2"])
        for k in KEYS:
            out[f"{name}.{k}"] = np.asarray(r[k])
    off, ow, pos, ref, lev = observations()
    n, dmin, dmax = model.update_normal_and_depth(off, ow, pos, ref, lev, scenes.SF[:scenes.NLEVELS])
    for k, v in (("offsets", off), ("obs_Ow", ow), ("pos", pos), ("ref_Ow", ref), ("ref_level", lev), ("normal", n),
                 ("dmin", dmin), ("dmax", dmax)):
        out[f"points.{k}"] = v
    return out


def main():
    out = build()
    for name in ("accept", "gates"):
        print(name, "codes", np.bincount(out[f"{name}.status"], minlength=10), "n_new", int(out[f"{name}.n_new"]))
    OUT.parent.mkdir(exist_ok=True)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
