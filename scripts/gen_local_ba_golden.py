#!/usr/bin/env python3
"""Writes tests/golden/local_ba_320x240.npz from the CPU model of Optimizer::LocalBundleAdjustment
(tests/native/local_ba_model.cpp), and measures the model's own sensitivity, from which the GPU
tests' tolerances are taken.

  gen_local_ba_golden.py            write the fixture
  gen_local_ba_golden.py --spread   print the spread over every host case of the GPU tests

The fixture is a 320x240 window (6 free + 3 fixed keyframes, 180 points seen 4 times, 20 % gross
outliers, 6 points behind a camera) whose seed is chosen so that the model is decisive (every
classified chi2 at least 1e-5 from 5.991, every depth at least 1e-5 of the scene's depth from 0) and
so that each of the first three mutants - Huber weight dropped, the edges of a point that went bad in
round 1 removed from round 2, isDepthPositive dropped - changes at least 4 of its edge_erased bytes;
the script refuses to write otherwise.

The spread: per case and over all cases, the largest difference in a pose entry, a point coordinate
and a classified chi2 (relative to 5.991, or to itself where larger) between the model's edge-order sums and its pairwise /
reversed sums, and between its -ffp-contract=off build and a -ffp-contract=fast -mfma build.  The
case without a fixed keyframe is reported apart, on its final robust chi2 alone.
"""
import pathlib
import subprocess
import sys
import tempfile

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import __graft_entry__ as ge  # noqa: E402
import local_ba_model as lbm  # noqa: E402
import local_ba_scenes as sc  # noqa: E402

OUT = ROOT / "tests" / "golden" / "local_ba_320x240.npz"
MUTANTS = {1: "Huber weight dropped", 2: "edges of round-1 bad points removed", 3: "isDepthPositive dropped"}
MIN_FLAGS = 4


def variants(g, fma_lib):
    return [lbm.local_bundle_adjustment(g, **kw) for kw in ({"sum_order": 1}, {"sum_order": 2}, {"path": fma_lib})]


def final_chi2(r):
    return r["info"]["round"][1]["chi2_after"]


def spread(fma_lib, fixture) -> dict:
    tot = {"pose": 0.0, "point": 0.0, "chi2": 0.0, "flips": 0}
    for name in list(sc.HOST_CASES) + ["golden"]:
        g = fixture if name == "golden" else sc.host_case(name)
        r0, ps, xs, cs, flips = g["model"], 0.0, 0.0, 0.0, 0
        for r in variants(g, fma_lib):
            ps, xs, cs = max(ps, sc.pose_spread(r0, r)), max(xs, sc.point_spread(r0, r)), max(cs, sc.chi2_spread(r0, r))
            flips += int((r["edge_erased"] != r0["edge_erased"]).sum() + (r["pt_bad"] != r0["pt_bad"]).sum())
        print(f"  {name:28s} pose {ps:.3e}  point {xs:.3e}  chi2 {cs:.3e}  flags that differ {flips}")
        tot = {"pose": max(tot["pose"], ps), "point": max(tot["point"], xs), "chi2": max(tot["chi2"], cs),
               "flips": tot["flips"] + flips}
    g = sc.host_case(sc.GAUGE_FREE_CASE[0])
    c0 = final_chi2(g["model"])
    tot["gauge_free_chi2"] = max(abs(final_chi2(r) - c0) / c0 for r in variants(g, fma_lib))
    tot["gauge_free_pose"] = max(sc.pose_spread(g["model"], r) for r in variants(g, fma_lib))
    return tot


def fixture_case():
    for seed in range(1400, 2400, 25):
        g = sc.fixture_scene(seed)
        m = g["model"]
        changed = {v: int((lbm.local_bundle_adjustment(g, variant=v)["edge_erased"] != m["edge_erased"]).sum())
                   for v in MUTANTS}
        if all(n >= MIN_FLAGS for n in changed.values()):
            return g, changed
    return None, None


def main() -> int:
    ge.build()
    g, changed = fixture_case()
    if g is None:
        print("refusing to write: no seed makes every mutant change at least 4 edge_erased bytes", file=sys.stderr)
        return 1
    if "--spread" in sys.argv:
        with tempfile.TemporaryDirectory() as d:
            fma = pathlib.Path(d) / "liblocal_ba_model_fma.so"
            subprocess.run(ge.LOCAL_BA_MODEL_CMD(fma, ("-ffp-contract=fast", "-mfma")), check=True)
            t = spread(fma, g)
        print(f"all: pose spread {t['pose']:.3e}, point spread {t['point']:.3e}, chi2 spread {t['chi2']:.3e} relative, "
              f"{t['flips']} flags differ; scene scale {sc.RADIUS}")
        print(f"no fixed keyframe: final robust chi2 spread {t['gauge_free_chi2']:.3e} relative "
              f"(its pose spread, not compared: {t['gauge_free_pose']:.3e})")
        return 0
    m = g["model"]
    for v, n in changed.items():
        print(f"mutant {v} ({MUTANTS[v]}): {n} edge_erased bytes change")
    rounds = np.array([[r[k] for k in ("iterations", "trials", "active_edges", "active_points", "active_keyframes",
                                       "refused")] for r in m["info"]["round"]], np.int32)
    np.savez_compressed(OUT, **{k: g[k] for k in sc.GRAPH_KEYS}, seed=np.int32(g["seed"]), scale=np.float64(g["scale"]),
                        kf_pose_out=m["kf_pose"], kf_pose_out_f64=m["kf_pose_f64"], pt_pos_out=m["pt_pos"],
                        pt_pos_out_f64=m["pt_pos_f64"], edge_erased=m["edge_erased"], pt_bad=m["pt_bad"],
                        rounds=rounds, chi2_after=np.float64([r["chi2_after"] for r in m["info"]["round"]]),
                        chi2=m["chi2"], depth=m["depth"], mutant_flags=np.int32([changed[v] for v in sorted(changed)]))
    print(f"wrote {OUT} (seed {g['seed']}, {len(g['edge_pt'])} edges, {int((m['edge_erased'] > 0).sum())} erased, "
          f"{int((m['pt_bad'] > 0).sum())} bad points, {OUT.stat().st_size} bytes)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
