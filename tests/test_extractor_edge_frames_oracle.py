"""The oracle on the constructed frames of tests/extractor_edge_frames.py (CPU only).

Each frame's octave-0 result is known by construction (FAST of a single pixel, the `<= 3` re-run
rule, NMS inside and across cells, IC_Angle's exact moments); the oracle is pinned to it here, and
tests/test_gpu_extractor_edge_frames.py pins the kernels to the oracle on the same frames.  The
guards make sure that each frame really holds the inputs it was built for: they are recomputed from
the oracle's own level image, so a change of the builders that loses them fails here.
"""
import ctypes

import numpy as np
import pytest

import extractor_edge_frames as E
from oracle_lib import Oracle, lib

F32 = np.float32


def _oracle_run(name):
    f = E.frame(name)
    ora = Oracle(f.nf, E.SCALE, E.NLEVELS, 1, f.th)
    k, d = ora.extract(f.img)
    return f, ora, k, d


def _oct0(k):
    return k[k["octave"] == 0]


def _as_dict(k0):
    assert (k0["x"] == np.rint(k0["x"])).all() and (k0["y"] == np.rint(k0["y"])).all()
    out = {(int(x), int(y)): float(r) for x, y, r in zip(k0["x"], k0["y"], k0["response"])}
    assert len(out) == len(k0)
    return out


def _check_expected(f, k):
    got = _as_dict(_oct0(k))
    want = {p: float(r) for p, r in f.expected.items()}
    missing = sorted(set(want) - set(got))
    extra = sorted(set(got) - set(want))
    assert not missing and not extra, (
        f"{f.name}: missing {[(p, f.describe(*p)) for p in missing[:4]]}, "
        f"unexpected {[(p, f.describe(*p)) for p in extra[:4]]}")
    wrong = [(p, got[p], want[p], f.describe(*p)) for p in want if got[p] != want[p]]
    assert not wrong, f"{f.name}: responses differ: {wrong[:4]}"


@pytest.mark.parametrize("nf,cols,rows,cw,ch", [(2000, 9, 11, 33, 20), (500, 4, 5, 73, 43), (300, 3, 3, 97, 71)])
def test_cell_grid_restatement(nf, cols, rows, cw, ch):
    g = E.cell_grid(nf)
    assert (g.cols, g.rows, g.cellW, g.cellH) == (cols, rows, cw, ch)
    ora = Oracle(nf, E.SCALE, E.NLEVELS, 1, 20)
    assert E.features_per_level(nf) == ora.level_info()[0].tolist()
    assert ora.level_info()[3].tolist() == E.umax_table()
    # a mark on the first and on the last pixel of every cell: the oracle counts two corners in every
    # cell, so the restated boundaries are the oracle's
    img = np.full((E.H, E.W), E.BG, np.uint8)
    xs = [E.EDGE] + g.x_bounds() + [E.W - E.EDGE]
    ys = [E.EDGE] + g.y_bounds() + [E.H - E.EDGE]
    for i in range(rows):
        for j in range(cols):
            img[ys[i], xs[j]] = 200           # first pixel of the cell
            img[ys[i + 1] - 1, xs[j + 1] - 1] = 200  # its last pixel
            assert g.cell_of(xs[j], ys[i]) == (i, j) == g.cell_of(xs[j + 1] - 1, ys[i + 1] - 1)
    k, _ = ora.extract(img)
    cc = ora.cell_counts(0)
    assert cc.shape == (rows, cols) and (cc == 2).all()
    # diagonal neighbours across a cell corner do not suppress each other: all survive
    assert len(_oct0(k)) == 2 * rows * cols


@pytest.mark.parametrize("th", [20, 12, 7])
def test_threshold_and_rerun_table(th):
    f, ora, k, _ = _oracle_run(f"threshold_table_{th}")
    _check_expected(f, k)
    # the table's own counts at th = 20: 5 + 6 + 4 + 3 + 4 = 22 per copy, and the arc mark of the
    # fourth cell, a corner only in the re-run
    if th == 20:
        assert len(f.expected) == 2 * 23
        assert [len(E.cell_rule(c, 20)) for c in E.table_cases(20)] == [5, 6, 4, 4, 4]
        assert [sum(E.strength(v) > 20 for v in c) for c in E.table_cases(20)] == [5, 3, 4, 0, 4]
    cc = ora.cell_counts(0)
    for kcase, contrasts in enumerate(E.table_cases(th)):
        for col in (kcase % 4, (kcase + 2) % 4):
            assert cc[kcase, col] == len(E.cell_rule(contrasts, th))


def test_saturated_strengths():
    f, _, k, _ = _oracle_run("saturated")
    _check_expected(f, k)
    r = _oct0(k)["response"]
    assert r.max() == 254 and set(r.tolist()) == {253.0, 254.0}


@pytest.mark.parametrize("kind", ["h", "v", "d"])
def test_nms_pair_sweep(kind):
    f, _, k, _ = _oracle_run(f"nms_pairs_{kind}")
    _check_expected(f, k)
    g = E.cell_grid(f.nf)
    assert f.straddling >= (g.rows - 1 if kind == "v" else g.cols - 1)
    # the three outcomes all occur
    labels = [f.labels[p] for p in f.expected]
    assert any("straddling" in s for s in labels) and any("inside" in s and "201" in s for s in labels)
    assert any("inside" in s and "200,200" in s for p, s in f.labels.items() if p not in f.expected)


def test_orientation_ties():
    f, ora, k, _ = _oracle_run("orientation_ties")
    _check_expected(f, k)
    padded = ora.level_image(0)
    umax = ora.level_info()[3].tolist()
    k0 = _oct0(k)
    seen = {}
    for kp in k0:
        p = (int(kp["x"]), int(kp["y"]))
        off, cls, nominal = f.kinds[p]
        m10, m01 = E.ic_moments(padded, p[0], p[1], umax)
        assert (m10, m01) == ((0, 0) if off is None else (4 * off[0], 4 * off[1])), (p, m10, m01)
        assert E.moment_class(m10, m01) == cls, (p, m10, m01)
        ang = float(kp["angle"])
        if cls in ("m10=m01=0", "m01=0,m10>0"):
            assert ang == 0.0, (p, cls, ang)
        else:
            assert abs(ang - nominal) <= 0.3, (p, cls, ang)  # fastAtan2's documented accuracy
        seen.setdefault((off, cls), []).append(ang)
    assert len(seen) == 9 and all(len(v) >= 4 for v in seen.values())
    # fastAtan2 is not exact at its ties: the diagonals are off 45 by the polynomial's error
    assert seen[((6, 6), "|m10|=|m01|")][0] == float(lib().oracle_fast_atan2(24.0, 24.0)) != 45.0


def _blur_setup():
    f, ora, k, d = _oracle_run("blur_ties")
    padded = ora.level_image(0)
    T = E.blur_sums(padded)
    sel = k["octave"] == 0
    k0, d0 = k[sel], d[sel]
    rad = k0["angle"].astype(F32) * F32(np.pi / float(F32(180.0)))
    a = np.array([lib().oracle_cosf(float(r)) for r in rad], F32)
    b = np.array([lib().oracle_sinf(float(r)) for r in rad], F32)
    xy = np.stack([np.rint(k0["x"]), np.rint(k0["y"])], 1).astype(np.int64)
    return f, ora, padded, T, k0, d0, xy, a, b


def test_blur_ties_guards():
    f, ora, padded, T, k0, d0, xy, a, b = _blur_setup()
    plane = E.blur_plane(T)
    ob = np.empty((E.H, E.W), np.uint8)
    assert ora.L.oracle_level_blurred(ora.h, 0, ob.ctypes.data_as(ctypes.c_void_p)) == 0
    assert np.array_equal(plane, ob), np.argwhere(plane != ob)[:5]
    pat = E.pattern31()
    desc, X, Y = E.descriptors_level0(plane, padded, xy, a, b, pat)
    bad = np.nonzero((desc != d0).any(axis=1))[0]
    assert len(bad) == 0, f"restated descriptor differs for {len(bad)} of {len(k0)} keypoints, first {k0[bad[:3]]}"
    n_simd, n_tail, ties = E.discriminating_ties(T)
    assert n_simd >= 2000, n_simd
    assert n_tail >= 100, n_tail
    inside = (X >= 0) & (X < E.W) & (Y >= 0) & (Y < E.H)
    hit = inside & ties[np.clip(Y, 0, E.H - 1), np.clip(X, 0, E.W - 1)]
    xs = (E.W // 4) * 4
    tail_hits = hit & (X >= xs)
    d_tail, _, _ = E.descriptors_level0(E.blur_plane(T, tail_rule="even"), padded, xy, a, b, pat)
    d_simd, _, _ = E.descriptors_level0(E.blur_plane(T, simd_rule="up"), padded, xy, a, b, pat)
    ch_tail = int((d_tail != d0).any(axis=1).sum())
    ch_simd = int((d_simd != d0).any(axis=1).sum())
    print(f"blur_ties: {len(k0)} octave-0 keypoints, ties simd {n_simd} tail {n_tail}, tail sample hits "
          f"{int(tail_hits.sum())} on {int(tail_hits.any(axis=1).sum())} keypoints, descriptors changed by "
          f"tail->even {ch_tail}, simd->up {ch_simd}")
    assert ch_tail >= 8, ch_tail
    assert ch_simd >= 100, ch_simd
    # keypoints changed by the tail rule are right-edge marks or their helpers
    for i in np.nonzero((d_tail != d0).any(axis=1))[0]:
        assert "right-edge" in f.describe(*xy[i]), (xy[i], f.describe(*xy[i]))


def test_mass_ties_guards():
    f, ora, k, _ = _oracle_run("mass_ties")
    k0 = _oct0(k)
    assert ora.cell_counts(0).sum() == 936
    assert set(k0["response"].tolist()) == {79.0}
    assert len(k0) == E.features_per_level(f.nf)[0] == 97
    g = E.cell_grid(f.nf)
    assert (ora.cell_counts(0) > g.per_cell).all()  # every cell's retainBest cuts too
    assert all((int(x), int(y)) in f.labels for x, y in zip(k0["x"], k0["y"]))
