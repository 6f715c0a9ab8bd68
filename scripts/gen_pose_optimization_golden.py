#!/usr/bin/env python3
"""Writes tests/golden/pose_optimization_320x240.npz from the CPU model of
Optimizer::PoseOptimization (tests/native/pose_optimization_model.cpp), and measures the model's own
sensitivity, from which the GPU tests' tolerance is taken.

  gen_pose_optimization_golden.py            write the fixture
  gen_pose_optimization_golden.py --spread   print the spread over every case of the GPU tests

The fixture is a 320x240 problem (400 keypoints, 300 with a MapPoint, 30 % gross outliers, 8
levels) whose seed is chosen so that the model is decisive (every classified chi2 at least 1e-5
from its threshold) and so that each of the three mutants - Huber weight dropped, level-1 edges
left in the optimisation, outlier edges not re-evaluated before classification - changes at least
4 of its flags; the script refuses to write otherwise.

The spread: over all cases, the largest difference in a pose entry, and in a classified chi2
relative to its threshold, between the model's edge-order sum and its pairwise / reversed sums, and
between its -ffp-contract=off build and a -ffp-contract=fast -mfma build.
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
import pose_optimization_model as pom  # noqa: E402

OUT = ROOT / "tests" / "golden" / "pose_optimization_320x240.npz"
MUTANTS = {1: "Huber weight dropped", 2: "level-1 edges left in", 3: "outliers not re-evaluated"}
MIN_FLAGS = 4


def args_of(c):
    return c["p3d"], c["obs"], c["inv_sigma2"], c["has_mp"], c["K"], c["pose_in"]


def spread(cases: dict, fma_lib) -> tuple:
    ps = cs = 0.0
    flips = 0
    for name, c in cases.items():
        r0 = pom.pose_optimization(*args_of(c))
        for kw in ({"sum_order": 1}, {"sum_order": 2}, {"path": fma_lib}):
            r = pom.pose_optimization(*args_of(c), **kw)
            ps, cs = max(ps, pom.pose_spread(r0, r)), max(cs, pom.chi2_spread(r0, r))
            flips += int((r["outlier"] != r0["outlier"]).sum())
    return ps, cs, flips


def fixture_case():
    for seed in range(9000, 9400):
        c = pom.make_case(seed, 400, edges=300, outliers=0.3)
        if c["seed"] != seed:
            continue
        m = c["model"]
        changed = {v: int((pom.pose_optimization(*args_of(c), variant=v)["outlier"] != m["outlier"]).sum())
                   for v in MUTANTS}
        if all(n >= MIN_FLAGS for n in changed.values()):
            return c, changed
    return None, None


def main() -> int:
    ge.build()
    with tempfile.TemporaryDirectory() as d:
        fma = pathlib.Path(d) / "libpose_optimization_model_fma.so"
        subprocess.run(ge.POSE_OPTIMIZATION_MODEL_CMD(fma, ("-ffp-contract=fast", "-mfma")), check=True)
        c, changed = fixture_case()
        if c is None:
            print("refusing to write: no seed makes every mutant change at least 4 flags", file=sys.stderr)
            return 1
        if "--spread" in sys.argv:
            cases = pom.host_cases()
            cases["golden"] = c
            ps, cs, flips = spread(cases, fma)
            print(f"{len(cases)} cases: pose spread {ps:.3e}, chi2 spread {cs:.3e} of the threshold, "
                  f"{flips} flags differ; tolerance = 100 x = {100 * ps:.2e}")
            return 0
    m = c["model"]
    for v, n in changed.items():
        print(f"mutant {v} ({MUTANTS[v]}): {n} flags change")
    i = m["info"]
    np.savez_compressed(OUT, p3d=c["p3d"], obs=c["obs"], inv_sigma2=c["inv_sigma2"], has_mp=c["has_mp"],
                        K=np.float32(c["K"]), pose_in=c["pose_in"], seed=np.int32(c["seed"]), pose=m["pose"],
                        pose_f64=m["pose_f64"], outlier=m["outlier"], n_inliers=np.int32(m["n_inliers"]),
                        n_initial=np.int32(i.n_initial), n_bad=np.int32(i.n_bad), rounds=np.int32(i.rounds),
                        iterations=np.int32(list(i.iterations)), trials=np.int32(i.trials), lambda_=np.float64(i.lambda_), chi2=m["chi2"],
                        mutant_flags=np.int32([changed[v] for v in sorted(changed)]))
    print(f"wrote {OUT} (seed {c['seed']}, {i.n_initial} edges, {i.n_bad} outliers, {OUT.stat().st_size} bytes)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
