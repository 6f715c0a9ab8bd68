#!/usr/bin/env python3
"""Writes tests/golden/initializer_reconstruct.npz: small synthetic pairs
(tests/initializer_reconstruct_scenes.py), the answers of the C++ model
(tests/native/initializer_reconstruct_model.cpp) and the recorded acosf bound for parallax_deg.

The bound is 4 x the largest deviation of parallax_deg among model variants that move acosf's result
by one ulp up and down, over every hypothesis of the fixture.  The generator refuses a fixture in
which a variant changes an accept / reject decision, in which a scene does not show what its name
says, or whose decisive count comparison lies within 5 % of bestGood (H) / maxGood (F) of its
boundary."""
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import initializer_reconstruct_model as model  # noqa: E402
import initializer_reconstruct_scenes as scenes  # noqa: E402

OUT = ROOT / "tests" / "golden" / "initializer_reconstruct.npz"
EXPECT = {"f60": True, "f130": True, "f300": True, "h_accept": True, "h_ambiguous_t": False,
          "h_ambiguous_plane": False}
KEYS = ("ok", "R21", "t21", "P3D", "triangulated", "n_motion", "motion_R", "motion_t", "n_good", "cos_parallax",
        "parallax_deg", "best", "n_inliers")


def margins_ok(name, r):
    g = np.sort(r["n_good"][:r["n_motion"]])[::-1].astype(np.float64)
    top, second, N = g[0], g[1], r["n_inliers"]
    if r["n_motion"] == 4:  # maxGood >= nMinGood, no second hypothesis above 0.7 maxGood
        gaps = [abs(top - max(int(0.9 * N), 50)), abs(second - 0.7 * top)]
    else:  # secondBest < 0.75 bestGood, bestGood > 0.9 N
        gaps = [abs(second - 0.75 * top), abs(top - 0.9 * N)]
    if min(gaps) < 0.05 * top:
        raise SystemExit(f"{name}: a decisive comparison is within 5 % of its boundary: gaps {gaps}, best {top}")


def main():
    out, dev = {}, 0.0
    for name in scenes.SCENE_NAMES:
        s = scenes.scene(name, extra1=17, extra2=9, shuffle=True)
        n = int((s["m12"] >= 0).sum())
        mask = np.ones(n, np.uint8)
        args = (s["k1"], s["k2"], s["m12"], s["M21"], s["use_h"], mask, scenes.K4)
        r = model.reconstruct(*args)
        if r["ok"] != EXPECT[name]:
            raise SystemExit(f"{name}: ok = {r['ok']}, the scene is meant to give {EXPECT[name]}: n_good {r['n_good']}")
        margins_ok(name, r)
        for variant in (-1, 1):
            rv = model.reconstruct(*args, acos_variant=variant)
            if rv["ok"] != r["ok"] or rv["best"] != r["best"]:
                raise SystemExit(f"{name}: the decision changes when acosf moves by one ulp")
            dev = max(dev, float(np.abs(rv["parallax_deg"].astype(np.float64) - r["parallax_deg"]).max()))
        sel = r["parallax_deg"][np.argmax(r["n_good"])]
        print(f"{name}: ok {r['ok']} best {r['best']} n_good {r['n_good'][:r['n_motion']]} parallax {sel:.3f}")
        for k, v in (("k1", s["k1"]), ("k2", s["k2"]), ("m12", s["m12"]), ("M21", s["M21"]),
                     ("use_h", np.int32(s["use_h"])), ("mask", mask)):
            out[f"{name}.{k}"] = v
        for k in KEYS:
            out[f"{name}.{k}"] = np.asarray(r[k])
    bound = 4.0 * dev
    for name in scenes.SCENE_NAMES:  # the parallax test itself must not sit inside the bound
        p = out[f"{name}.parallax_deg"][np.argmax(out[f"{name}.n_good"])]
        if abs(float(p) - 1.0) <= bound:
            raise SystemExit(f"{name}: the selected parallax {p} is within the acosf bound of min_parallax")
    out["parallax_bound"] = np.float64(bound)
    out["K4"] = scenes.K4
    OUT.parent.mkdir(exist_ok=True)
    np.savez_compressed(OUT, **out)
    print(f"largest one-ulp deviation {dev:.3e} deg, bound {bound:.3e} deg -> {OUT} ({OUT.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
