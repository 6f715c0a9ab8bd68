"""The pyramid sweep's case table (tests/pyramid_cases.py) covers what it claims to: level sizes
come from the oracle's ComputePyramid, and every geometry-dependent branch of the four pyramid
builders named in DESIGN.md §5.2 is reached by some case.  No GPU: this is what keeps the table
from losing coverage silently when a case is edited."""
import numpy as np
import pytest

import pyramid_cases as pc


def test_width_sweep_takes_every_residue_at_every_level():
    sizes = [pc.level_sizes(c) for c in pc.WIDTH_SWEEP]
    assert all(len(s) == 4 for s in sizes)
    for l in range(4):
        assert {s[l][0] % 16 for s in sizes} == set(range(16)), f"level {l}"
    # the smallest level of the sweep, and no level under the extractor's 33 x 33
    assert sizes[0][3] == (37, 33)
    assert min(min(w, h) for s in sizes for w, h in s) >= 33
    # level-0 right border: the aligned v_perm branch and the general one at every other residue
    assert {c.W % 16 for c in pc.WIDTH_SWEEP} == set(range(16))
    # VResizeLinear's scalar tail: none (width a multiple of 16) and 1 .. 4 columns, at every level >= 1
    for l in range(1, 4):
        assert {pc.tail_columns(s[l][0]) for s in sizes} == {0, 1, 2, 3, 4}, f"level {l}"


def test_tail_columns_restates_the_walk():
    for dw in range(17, 200):
        t = pc.tail_columns(dw)
        assert 0 <= t <= 4 and (dw - t) % 4 == 0 and (t == 0) == (dw % 16 == 0)


def test_height_sweep_reaches_the_close_mirror_rows():
    sizes = [pc.level_sizes(c) for c in pc.HEIGHT_SWEEP]
    heights = {h for s in sizes for _, h in s}
    assert set(range(33, 51)) <= heights
    # only at h = 33 does one row (16) carry both mirror stores
    for h in range(33, 60):
        both = pc.mirror_rows(h)[2]
        assert both == ({16} if h == 33 else set()), h
    assert any(s[3][1] == 33 for s in sizes)
    # level 0 takes at least 16 consecutive heights
    h0 = sorted({s[0][1] for s in sizes})
    assert len(h0) >= 16 and h0 == list(range(h0[0], h0[0] + len(h0)))
    assert min(min(w, h) for s in sizes for w, h in s) >= 33


def test_level_count_cases():
    by_l = {c.nl: c for c in pc.LEVEL_COUNTS}
    assert set(by_l) == {2, 3, 8, 13, 14, 15, 16}
    assert pc.level_sizes(by_l[14])[-1] == (35, 34)
    assert pc.level_sizes(by_l[15])[-1] == (37, 35)
    for c in pc.LEVEL_COUNTS:
        assert len(pc.level_sizes(c)) == c.nl
        assert min(min(w, h) for w, h in pc.level_sizes(c)) >= 33
        # L > PS_THREADS / 64 - PS_LOADERS = 14 builder waves: no plan
        assert (c.expect == pc.PLAN) == (c.nl <= 14), c.name
    # nlevels == 2: level 1 is the last level, so the fused tail (levels resizeTail .. L-1 with
    # resizeTail + 1 < L) does not exist and must not be launched
    assert by_l[2] in pc.TAIL_CASES


def test_scale_factor_cases():
    assert [c.sf for c in pc.SCALE_FACTORS] == [1.05, 1.33, 1.5, 1.7, 1.9, 1.99, 2.5, 3.0]
    for c in pc.SCALE_FACTORS:
        assert c.expect in (pc.PLAN, pc.NO_PLAN, pc.REFUSED)
        if c.expect != pc.PLAN:
            assert c.why, f"{c.name}: a case without a plan states why"
        if c.expect != pc.REFUSED:
            assert len(pc.level_sizes(c)) == c.nl


def test_wide_cases_and_recorded_k0():
    for W, H, nf in [(600, 100, 400), (1000, 150, 600), (1300, 200, 800), (2040, 300, 1500)]:
        assert any((c.W, c.H, c.nf, c.sf, c.nl) == (W, H, nf, 1.2, 3) for c in pc.WIDE_SHORT)
    k0 = {c.k0 for c in pc.ALL_CASES if c.expect == pc.PLAN}
    assert k0 <= {32, 24, 16, 12, 8, 6, 4, 2} and len(k0) >= 5, sorted(k0)
    for c in pc.ALL_CASES:
        assert (c.k0 is not None) == (c.expect == pc.PLAN), c.name
        # level-0 rows per round are bounded by the loaders' K0 * ceil(W / 16) <= 1024 units
        if c.k0:
            assert c.k0 * ((c.W + 15) // 16) <= 1024, c.name


def test_alignment_cases_cover_load_unit16():
    assert [c.W for c in pc.ALIGN_WIDTHS] == list(range(64, 80))
    assert pc.ALIGN_LAYOUTS == [(0, 0), (1, 3), (4, 12), (16, 16), (15, 1)]
    aligns, seen = set(), {16: set(), 4: set(), 1: set()}
    for c in pc.ALIGN_WIDTHS:
        for off, extra in pc.ALIGN_LAYOUTS:
            stride = c.W + extra
            # (device allocations are 256-byte aligned: the base address counts as 0 here; the GPU
            # test repeats this with the real pointer)
            a, s = pc.load_classes(off, stride, c.H * stride, c.W, c.H, 2)
            aligns.add(a)
            seen[a] |= s
    assert aligns == {16, 4, 1}
    # dword-aligned rows have a width that is a multiple of 4, so their last unit needs 4, 8, 12 or
    # 16 bytes; every other count comes with byte-aligned rows
    assert {need for need, _ in seen[4]} == {4, 8, 12, 16}
    assert {need for need, _ in seen[1]} == set(range(1, 17))
    for a in (4, 1):
        assert {over for _, over in seen[a]} == {False, True}, a
    # (a 16-byte-aligned stride means a width that is a multiple of 16: whole units, one load each)
    assert seen[16] == set()
    # the partial-unit mask (1 << 8 nb) - 1 runs with nb = 1, 2 and 3
    nb = {min(max(need - 4 * q, 0), 4) for a in seen for need, _ in seen[a] for q in range(4)}
    assert {1, 2, 3} <= nb


def test_frames_are_fixed_and_shared():
    c = pc.WIDTH_SWEEP[3]
    f = pc.frames(c, 8)
    assert f.shape == (8, c.H, c.W) and f.dtype == np.uint8 and not f.flags.writeable
    assert f is pc.frames(c, 8)
    assert set(np.unique(f[1])) == {0, 255}
    assert len(np.unique(f[0])) > 200 and len(np.unique(f[7])) > 200
    assert pc.oracle_levels(c, f[0]) is pc.oracle_levels(c, f[0].copy())
    with pytest.raises(ValueError):
        f[0, 0, 0] = 1


def test_embedded_frames_sit_in_random_bytes():
    c = pc.ALIGN_WIDTHS[5]
    buf, stride = pc.embed(c, 2, 15, 1)
    v = buf[15:15 + 2 * c.H * stride].reshape(2, c.H, stride)
    assert np.array_equal(v[:, :, :c.W], pc.frames(c, 2))
    assert len(np.unique(v[:, :, c.W:])) > 50 and len(np.unique(buf[:15])) > 5


def test_subsets():
    assert len(pc.TAIL_CASES) == 16 + 9 + len(pc.LEVEL_COUNTS)
    auto = pc.auto_cases()
    assert sum(c.expect == pc.PLAN for c in auto) == 3
    assert all(c in auto for c in pc.ALL_CASES if c.expect == pc.NO_PLAN)
    names = [c.name for c in pc.ALL_CASES]
    assert len(set(names)) == len(names)
