"""csrc/orb_rot_hist.h, the rotation filter every matcher kernel shares, compiled for the host
(tests/native/rot_hist_host.cpp -> build/librot_hist_host.so).

rot_bin against the oracle's (oracle/orb_oracle.cpp) and against test_matcher_oracle.rot_bin;
three_maxima against test_matcher_oracle.three_maxima.  Equal ints, no tolerance.  The input set of
three_maxima is also shown to tell each `>` of the scan from `>=` and each `<` of the two float
comparisons from `<=`; the same source runs once as a program under AddressSanitizer and UBSan."""
import ctypes
import pathlib
import subprocess
import sys

import numpy as np
import pytest

from gate_tables import F32, down, up
from oracle_lib import lib as oracle
from test_matcher_oracle import rot_bin, three_maxima

ROOT = pathlib.Path(__file__).resolve().parents[1]
H = 30


@pytest.fixture(scope="module")
def L():
    lib = ctypes.CDLL(str(ROOT / "build" / "librot_hist_host.so"))
    assert lib.rot_hist_length() == H
    return lib


def native_bins(L, a1, a2):
    a1, a2 = np.ascontiguousarray(a1, np.float32), np.ascontiguousarray(a2, np.float32)
    out = np.full(len(a1), -7, np.int32)
    L.rot_hist_rot_bin(ctypes.c_void_p(a1.ctypes.data), ctypes.c_void_p(a2.ctypes.data), len(a1),
                       ctypes.c_void_p(out.ctypes.data))
    return out


def native_maxima(L, hists):
    hists = np.ascontiguousarray(hists, np.int32).reshape(-1, H)
    ind = np.full((len(hists), 3), -7, np.int32)
    L.rot_hist_three_maxima(ctypes.c_void_p(hists.ctypes.data), len(hists), ctypes.c_void_p(ind.ctypes.data))
    return ind


# ---- rot_bin ---------------------------------------------------------------------------------------
def boundary_pairs():
    """Every boundary rot = 15 + 30 k as tests/sfi_gate_tables.py's rotbin_tables builds it: the float
    below it, the boundary, the float above, and the last float of bin k where that is not `below`."""
    pairs = []
    for k in range(12):
        b = F32(15 + 30 * k)
        vals = [down(b), b, up(b)]
        v = down(b)
        for _ in range(8):
            if rot_bin(v, F32(0)) == k:
                break
            v = down(v)
        assert rot_bin(v, F32(0)) == k and rot_bin(up(v), F32(0)) == k + 1
        assert rot_bin(b, F32(0)) == k + 1
        vals.append(v)
        pairs += [(a, F32(0)) for a in vals]
    return pairs


def test_rot_bin_edges(L):
    den = F32(1e-40)
    assert np.signbit(F32(F32(-0.0) - F32(0.0)))
    assert F32(F32(0) - den) < 0 and F32(F32(F32(0) - den) + F32(360)) == 360  # negative, then exactly 360
    # Keypoint angles lie in [0, 360), so rot * (1 / 30) stays below 12.5 and the `== 30` wrap is never
    # taken by a matcher; only a difference of 885 or more reaches it, and such rows pin it here.
    pairs = boundary_pairs() + [(F32(900), F32(0)), (F32(885), F32(0)), (F32(880), F32(0)),
                                (F32(-0.0), F32(0.0)), (F32(0), den), (F32(0), F32(15))]
    got = native_bins(L, [p[0] for p in pairs], [p[1] for p in pairs])
    O = oracle()
    for (a1, a2), g in zip(pairs, got):
        assert g == rot_bin(a1, a2) == O.oracle_rot_bin(float(a1), float(a2)), (a1, a2, g)
    # the wrap (30 -> 0) and the bin before it; -0 stays in bin 0; exactly 360 -> 12; (0, 15) -> 345 -> 11.5 -> 12
    assert list(got[-6:]) == [0, 0, 29, 0, 12, 12]
    assert set(got) == set(range(13)) | {29}


def test_rot_bin_random(L):
    rng = np.random.default_rng(20261021)
    a = rng.uniform(0, 360, (100000, 2)).astype(np.float32)
    a[a >= 360] = 0  # (the float32 rounding of a double just under 360)
    got = native_bins(L, a[:, 0], a[:, 1])
    O = oracle()
    assert got.min() == 0 and got.max() == 12  # 360 / 30
    for (a1, a2), g in zip(a, got):
        assert g == rot_bin(a1, a2) == O.oracle_rot_bin(float(a1), float(a2)), (a1, a2, g)


# ---- three_maxima ----------------------------------------------------------------------------------
def hist_of(counts):
    h = [0] * H
    for b, n in counts:
        h[b] = n
    return h


def equality_rows():
    """The float-equality edge of `max < 0.1f * (float)max1`, from the product itself: for every max1 whose
    product is a whole number s, (max1, s) and (max1, s + 2, s) at equality and one short of it."""
    rows = []
    for m in range(1, 61):
        t = np.float32(0.1) * np.float32(m)
        s = int(t)
        if t != np.float32(s) or s < 1:
            continue
        rows += [[(7, m), (19, s)], [(22, s), (4, m), (13, s + 2)]]
        if s > 1:
            rows += [[(7, m), (19, s - 1)], [(22, s - 1), (4, m), (13, s + 2)]]
    assert len(rows) >= 8
    return [hist_of(r) for r in rows]


def maxima_inputs():
    hs = [hist_of([]), hist_of([(17, 1)]), hist_of([(0, 3)]), hist_of([(29, 2)])]
    # equal counts in two and in three (and four) bins: bin order decides
    hs += [hist_of([(21, 4), (6, 4)]), hist_of([(17, 4), (3, 4), (25, 4)]), hist_of([(17, 4), (3, 4), (25, 4), (9, 4)]),
           hist_of([(20, 3), (5, 6), (2, 3), (28, 2)]), hist_of([(11, 5), (6, 5), (27, 2), (14, 2)])]
    # a larger count after two smaller ones (the shift path), in each branch
    hs += [hist_of([(2, 3), (5, 4), (9, 7)]), hist_of([(2, 5), (5, 3), (9, 4)]), hist_of([(2, 5), (5, 4), (9, 2), (12, 3)]),
           [i + 1 for i in range(H)], [H - i for i in range(H)]]
    return hs + equality_rows()


def rule(h, gt=(False, False, False), le=(False, False)):
    """ComputeThreeMaxima with branch k's `>` as `>=` where gt[k], comparison k's `<` as `<=` where le[k]."""
    mx, ix = [0, 0, 0], [-1, -1, -1]
    for i, s in enumerate(h):
        for k in range(3):
            if s >= mx[k] if gt[k] else s > mx[k]:
                mx[k + 1:], ix[k + 1:] = mx[k:2], ix[k:2]
                mx[k], ix[k] = s, i
                break
    t = np.float32(0.1) * np.float32(mx[0])
    if mx[1] <= t if le[0] else mx[1] < t:
        ix[1] = ix[2] = -1
    elif mx[2] <= t if le[1] else mx[2] < t:
        ix[2] = -1
    return tuple(ix)


def test_three_maxima(L):
    made = maxima_inputs()
    hs = made + np.random.default_rng(7).integers(0, 7, (10000, H)).tolist()  # counts in [0, 6]: ties are common
    got = native_maxima(L, hs)
    want = [three_maxima([[0] * n for n in h]) for h in hs]  # (its histogram holds the entries themselves)
    assert [tuple(g) for g in got.tolist()] == want
    assert want[0] == (-1, -1, -1) and want[1] == (17, -1, -1)
    # the constructed inputs alone tell each comparison from its neighbour
    plain = [rule(h) for h in made]
    assert plain == want[:len(made)]
    for k in range(3):
        gt = tuple(j == k for j in range(3))
        assert any(rule(h, gt=gt) != w for h, w in zip(made, plain)), f"> and >= of branch {k + 1} not told apart"
    for k in range(2):
        le = tuple(j == k for j in range(2))
        assert any(rule(h, le=le) != w for h, w in zip(made, plain)), f"< and <= of max{k + 2} not told apart"


def test_sanitized_program(tmp_path):
    """The same source as a stand-alone program under AddressSanitizer and UBSan."""
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as ge

    exe = tmp_path / "rot_hist_host_san"
    subprocess.run(ge.ROT_HIST_HOST_CMD(exe, ("-DROT_HIST_HOST_MAIN", "-g", "-fsanitize=address,undefined",
                                              "-fno-sanitize-recover=all")), check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "status 0" in r.stdout and "ERROR" not in r.stderr, r.stdout + r.stderr
