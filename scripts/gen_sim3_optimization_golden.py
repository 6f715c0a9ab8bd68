#!/usr/bin/env python3
"""Writes tests/golden/sim3_optimization_320x240.npz from the CPU model of Optimizer::OptimizeSim3
(tests/native/sim3_optimization_model.cpp), and measures the model's own sensitivity, from which the
GPU tests' tolerance and margin are taken.

  gen_sim3_optimization_golden.py            write the fixture
  gen_sim3_optimization_golden.py --spread   print the spread over every case of the GPU tests

The fixture is a 320x240 loop candidate (400 slots, 300 usable, 15 % gross outliers, 30 % of the
second observations 1.5 to 3 pixels off, 8 levels on both sides) whose seed is chosen so that the
model is decisive (every classified chi2 at least MARGIN from th2) and so that each of the first three mutants - e21 weighted with 1/sigma2, only the
failing edge of a pair removed, more_iterations always 5 - changes a discrete result (kept, n_inliers,
n_bad or more_iterations); the script refuses to write otherwise.

The spread: over all cases, the largest difference in a Sim3 entry (qx qy qz qw t s), and in a
classified chi2 relative to th2, between the model's edge-order sum and its pairwise / reversed sums,
and between its -ffp-contract=off build and a -ffp-contract=fast -mfma build.  SIM3_TOL of the GPU
tests is 100 x the first, MARGIN at least 10 x the second; a case in which a discrete result differs
between the orders is reported and must be replaced.
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
import sim3_optimization_model as s3m  # noqa: E402

OUT = ROOT / "tests" / "golden" / "sim3_optimization_320x240.npz"
MUTANTS = {1: "e21 weighted with 1/sigma2", 2: "only the failing edge removed", 3: "more_iterations always 5"}
K_SMALL = np.float32([260, 258, 160, 120])


def discrete(r) -> tuple:
    i = r["info"]
    return (r["kept"].tobytes(), r["n_inliers"], i.n_correspondences, i.n_bad, i.more_iterations)


def spread(cases: dict, fma_lib) -> tuple:
    ss = cs = 0.0
    undecided = []
    for name, c in cases.items():
        r0 = s3m.run_case(c)
        for kw in ({"sum_order": 1}, {"sum_order": 2}, {"path": fma_lib}):
            r = s3m.run_case(c, **kw)
            ss, cs = max(ss, s3m.sim3_spread(r0, r)), max(cs, s3m.chi2_spread(r0, r, c["th2"]))
            if discrete(r) != discrete(r0):
                undecided.append(name)
    return ss, cs, sorted(set(undecided))


def fixture_case():
    for seed in range(9000, 9400):
        usable = np.random.default_rng(seed).permutation(400) < 300
        try:
            c = s3m.make_case(seed, 400, usable=usable, outliers=0.15, moderate=0.3, K1=K_SMALL, K2=K_SMALL, tries=1)
        except AssertionError:
            continue
        base = discrete(c["model"])
        changed = {v: discrete(s3m.run_case(c, variant=v)) != base for v in MUTANTS}
        if all(changed.values()):
            return c, changed
    return None, None


def main() -> int:
    ge.build()
    with tempfile.TemporaryDirectory() as d:
        fma = pathlib.Path(d) / "libsim3_optimization_model_fma.so"
        subprocess.run(ge.SIM3_OPTIMIZATION_MODEL_CMD(fma, ("-ffp-contract=fast", "-mfma")), check=True)
        c, changed = fixture_case()
        if c is None:
            print("refusing to write: no seed makes each of the first three mutants change a discrete result",
                  file=sys.stderr)
            return 1
        if "--spread" in sys.argv:
            cases = dict(s3m.host_cases())
            cases["threshold"] = s3m.threshold_case()
            cases["golden"] = c
            ss, cs, undecided = spread(cases, fma)
            print(f"{len(cases)} cases: Sim3 spread {ss:.3e}, chi2 spread {cs:.3e} of th2; SIM3_TOL = 100 x = "
                  f"{100 * ss:.2e}, MARGIN >= 10 x = {10 * cs:.2e} (tests/sim3_optimization_model.py has "
                  f"{s3m.MARGIN:.1e}); cases whose discrete results depend on the order: {undecided or 'none'}")
            return 0 if not undecided and s3m.MARGIN >= 10 * cs else 1
    m, i = c["model"], c["model"]["info"]
    for v, ch in changed.items():
        print(f"mutant {v} ({MUTANTS[v]}): discrete result changes: {ch}")
    np.savez_compressed(OUT, x3dc1=c["x3dc1"], x3dc2=c["x3dc2"], obs1=c["obs1"], obs2=c["obs2"],
                        inv_sigma2_1=c["inv_sigma2_1"], sigma2_2=c["sigma2_2"], usable=c["usable"], K1=c["K1"],
                        K2=c["K2"], th2=np.float32(c["th2"]), sim3_in=c["sim3_in"], seed=np.int32(c["seed"]),
                        kept=m["kept"], sim3=m["sim3"], sim3_f64=m["sim3_f64"], n_inliers=np.int32(m["n_inliers"]),
                        n_correspondences=np.int32(i.n_correspondences), n_bad=np.int32(i.n_bad),
                        more_iterations=np.int32(i.more_iterations), iterations=np.int32(list(i.iterations)),
                        trials=np.int32(i.trials), lambda_=np.float64(i.lambda_), chi2=m["chi2"])
    print(f"wrote {OUT} (seed {c['seed']}, {i.n_correspondences} pairs, {i.n_bad} removed, {m['n_inliers']} inliers, "
          f"{OUT.stat().st_size} bytes)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
