#!/usr/bin/env python3
"""Measures the bounds of tests/test_epnp_stages.py: runs the stage exports of the unmodified
csrc/orb_epnp_math.h (tests/native/pnp_solver_model.cpp) against tests/epnp_reference.py over the
test's own inputs and prints the largest difference per stage, how many cases each condition left
out, and which N the cases chose.  The test's constants are 10 x the printed values.

    python scripts/measure_epnp_stage_bounds.py            # the table
    python scripts/measure_epnp_stage_bounds.py --worst    # and the case that set each maximum
"""
import argparse
import collections
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import epnp_stage_checks as sc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worst", action="store_true")
    a = ap.parse_args()
    cases = sc.general_cases()
    worst, outside, chosen = {}, collections.Counter(), collections.Counter()
    for name, p3, p2, sel in cases:
        d, h, _ = sc.differences(p3, p2, sel)
        outside.update(d.pop("outside"))
        chosen[h["N"]] += 1
        for k, v in d.items():
            if k not in worst or v > worst[k][0]:
                worst[k] = (v, name)
    groups = collections.defaultdict(lambda: (0.0, ""))
    for k, (v, name) in worst.items():
        g = k.translate(str.maketrans("", "", "123"))  # one bound for the three N
        if v >= groups[g][0]:
            groups[g] = (v, f"{k} of {name}")
    print(f"{len(cases)} cases; N chosen: {dict(chosen)}")
    for g, (v, where) in groups.items():
        print(f"{g:16s} {v:.3e}   bound {10 * v:.3e}" + (f"   ({where})" if a.worst else ""))
    for k, v in sc.jacobi_svd_differences().items():
        print(f"jacobi_svd {k:16s} {v:.3e}   bound {10 * v:.3e}")
    print("left out by a condition (at most 5 % each):")
    for k, v in sorted(outside.items()):
        print(f"  {k:10s} {v:4d}  {100.0 * v / len(cases):.1f} %")


if __name__ == "__main__":
    main()
