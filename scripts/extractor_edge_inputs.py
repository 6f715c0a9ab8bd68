#!/usr/bin/env python3
"""How often the suite's synthetic frames hold the inputs that tests/extractor_edge_frames.py
constructs, counted with the CPU oracle: IC_Angle moments that are zero or equal,
and rBRIEF samples on blur sums that are exact halves with an even integer part, by column kind.

Usage: python scripts/extractor_edge_inputs.py        (CPU only; prints one table)
"""
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import __graft_entry__  # noqa: E402

__graft_entry__.build()

import extractor_edge_frames as E  # noqa: E402
import orbslam_jpminipc_amd as orb  # noqa: E402
from oracle_lib import Oracle, lib  # noqa: E402

F32 = np.float32
# the frames of test_extract_parity_configs / test_extract_parity_odd_sizes, two of each
SAMPLE = [(640, 480, 1000, 3), (1241, 376, 2000, 3), (641, 479, 1000, 11)]


def count_frame(ora, img, tot):
    k, _ = ora.extract(img)
    _, sf, _, um = ora.level_info()
    umax = um.tolist()
    pat = E.pattern31()
    for l in range(ora.nlevels):
        kl = k[k["octave"] == l]
        if not len(kl):
            continue
        padded = ora.level_image(l)
        h, w = padded.shape[0] - 32, padded.shape[1] - 32
        xy = np.stack([np.rint(kl["x"] / sf[l]), np.rint(kl["y"] / sf[l])], 1).astype(np.int64)
        for x, y in xy:
            m10, m01 = E.ic_moments(padded, int(x), int(y), umax)
            tot["keypoints"] += 1
            tot["both zero"] += m10 == 0 and m01 == 0
            tot["one zero"] += (m10 == 0) != (m01 == 0)
            tot["|m10| = |m01|"] += abs(m10) == abs(m01)
        T = E.blur_sums(padded)
        _, _, ties = E.discriminating_ties(T)
        rad = kl["angle"].astype(F32) * F32(np.pi / float(F32(180.0)))
        a = np.array([lib().oracle_cosf(float(r)) for r in rad], F32)
        b = np.array([lib().oracle_sinf(float(r)) for r in rad], F32)
        _, X, Y = E.descriptors_level0(E.blur_plane(T), padded, xy, a, b, pat)
        inside = (X >= 0) & (X < w) & (Y >= 0) & (Y < h)
        hit = inside & ties[np.clip(Y, 0, h - 1), np.clip(X, 0, w - 1)]
        xs = (w // 4) * 4
        tot["samples"] += X.size
        tot["tie samples, tail columns"] += int((hit & (X >= xs)).sum())
        tot["tie samples, SSE2 columns"] += int((hit & (X < xs)).sum())


def main():
    tot = {k: 0 for k in ("keypoints", "samples", "both zero", "one zero", "|m10| = |m01|",
                          "tie samples, tail columns", "tie samples, SSE2 columns")}
    for W, H, nf, stream in SAMPLE:
        ora = Oracle(nf, 1.2, 8, 1, 20)
        for img in orb.synth_stream(W, H, stream=stream, first=0, count=2):
            count_frame(ora, img, tot)
    for k, v in tot.items():
        print(f"{k:32s} {int(v)}")


if __name__ == "__main__":
    main()
