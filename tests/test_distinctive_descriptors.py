"""MapPoint::ComputeDistinctiveDescriptors (reference src/MapPoint.cc:185-250): the oracle
against a numpy restatement on the CPU, and the HIP kernel against the oracle on the GPU:
at the workload's sizes, across the 64 KB of LDS a kernel gets without asking for more (36 bytes
per observation: 1820 observations fit, 1821 do not) up to the limit of 4000 observations, and
on small points built so that the expected row can be written down."""
import ctypes

import numpy as np
import pytest

import orbslam_jpminipc_amd as orb
from orbslam_jpminipc_amd._native import ORB_EINVAL, ORB_ENOTSUP, hip_lib, ptr
from orbslam_jpminipc_amd.mappoint import compute_distinctive_descriptors, compute_distinctive_descriptors_device
from oracle_lib import Oracle, _p, lib
from vocab_util import POPCNT8


def _oracle(offsets, desc, usable):
    L = lib()
    L.oracle_compute_distinctive_descriptors.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 5
    M = len(offsets) - 1
    best = np.full(M, -7, np.int32)
    out = np.zeros((M, 32), np.uint8)
    off = np.ascontiguousarray(offsets, np.int32)
    d = np.ascontiguousarray(desc, np.uint8)
    u = None if usable is None else np.ascontiguousarray(usable, np.uint8)
    assert L.oracle_compute_distinctive_descriptors(M, _p(off), _p(d), _p(u), _p(best), _p(out)) == 0
    return best, out


def _numpy(offsets, desc, usable):
    best = []
    for m in range(len(offsets) - 1):
        rows = [r for r in range(offsets[m], offsets[m + 1]) if usable is None or usable[r]]
        if not rows:
            best.append(-1)
            continue
        d, kmed = desc[rows], (len(rows) - 1) // 2
        med = np.concatenate([  # all pairs, 128 candidate rows at a time (memory)
            np.sort(POPCNT8[np.bitwise_xor(d[i:i + 128, None, :], d[None, :, :])].sum(axis=2), axis=1)[:, kmed]
            for i in range(0, len(rows), 128)])
        best.append(rows[int(np.argmin(med))])  # argmin: first minimum
    return np.array(best, np.int32)


def _case(seed, sizes, frac_bad=0.2, near=True):
    rng = np.random.default_rng(seed)
    descs = Oracle(1000, 1.2, 8, 1, 20).extract(orb.synth_stream(640, 480, stream=50 + seed, count=1)[0])[1]
    rows, offsets = [], [0]
    for n in sizes:
        base = descs[rng.integers(len(descs))]
        for _ in range(n):
            d = base.copy()
            if near:  # observations of one point: a few flipped bits (many equal medians)
                for b in rng.choice(256, size=int(rng.integers(0, 12)), replace=False):
                    d[b // 8] ^= np.uint8(1 << (b % 8))
            else:
                d = descs[rng.integers(len(descs))]
            rows.append(d)
        offsets.append(len(rows))
    desc = np.stack(rows) if rows else np.zeros((0, 32), np.uint8)
    usable = (rng.random(len(rows)) > frac_bad).astype(np.uint8)
    return np.array(offsets, np.int32), desc, usable


SIZES = [1, 2, 3, 4, 5, 10, 0, 31, 64, 65, 130, 7, 2, 1]


@pytest.mark.parametrize("seed,near", [(0, True), (1, False), (2, True)])
def test_oracle_matches_numpy(seed, near):
    off, desc, usable = _case(seed, SIZES + [300, 1000], near=near)
    for u in (usable, None):
        best, out = _oracle(off, desc, u)
        assert best.tolist() == _numpy(off, desc, u).tolist()
        for m, r in enumerate(best):
            if r >= 0:
                assert out[m].tobytes() == desc[r].tobytes()


def test_host_validation():
    with pytest.raises(orb.OrbError):
        compute_distinctive_descriptors([0, 3, 2], np.zeros((3, 32), np.uint8))  # decreasing offsets


@pytest.mark.gpu
@pytest.mark.parametrize("seed,near", [(0, True), (1, False), (3, True)])
def test_gpu_matches_oracle(seed, near):
    off, desc, usable = _case(seed, SIZES + [300, 1000], near=near)
    for u in (usable, None):
        cur = np.full((len(off) - 1, 32), 0xAB, np.uint8)
        best, out = compute_distinctive_descriptors(off, desc, u, current=cur)
        ob, oo = _oracle(off, desc, u)
        assert best.tolist() == ob.tolist()
        for m, r in enumerate(ob):
            assert out[m].tobytes() == (oo[m].tobytes() if r >= 0 else cur[m].tobytes())


@pytest.mark.gpu
def test_gpu_all_rows_bad_and_empty():
    off = np.array([0, 3, 3], np.int32)
    desc = np.arange(96, dtype=np.uint8).reshape(3, 32)
    best, out = compute_distinctive_descriptors(off, desc, np.zeros(3, np.uint8), current=np.ones((2, 32), np.uint8))
    assert best.tolist() == [-1, -1] and (out == 1).all()
    best, out = compute_distinctive_descriptors([0], np.zeros((0, 32), np.uint8))
    assert len(best) == 0


# ---- across the 64 KB line and at the limit ---------------------------------------------------
MAX_OBS = 4000  # DD_MAX_OBS
LDS_PER_OBS = 36  # a 32-byte row and its row id
# the last size that fits in 64 KB of LDS and the first that does not, the limit and the size below it
BIG_SIZES = [3, 1820, 64, 1821, 1, 3999, 0, 4000, 65]
_BIG = {}


def _big():
    """One call's worth of near-duplicate observations (many equal medians) and the oracle's answer
    with and without the usable mask, computed once and shared read-only."""
    if not _BIG:
        off, desc, usable = _case(7, BIG_SIZES, near=True)
        ref = {True: _oracle(off, desc, usable), False: _oracle(off, desc, None)}
        for a in (off, desc, usable, *ref[True], *ref[False]):
            a.setflags(write=False)
        _BIG.update(off=off, desc=desc, usable=usable, ref=ref)
    return _BIG


def test_big_case_inputs():
    c = _big()
    off, usable = c["off"], c["usable"]
    assert np.diff(off).tolist() == BIG_SIZES and max(BIG_SIZES) == MAX_OBS
    assert 1820 * LDS_PER_OBS <= 64 * 1024 < 1821 * LDS_PER_OBS
    for masked in (True, False):
        best, out = c["ref"][masked]
        for m, r in enumerate(best):
            if BIG_SIZES[m] == 0 or (masked and not usable[off[m]:off[m + 1]].any()):
                assert r == -1
            else:
                assert off[m] <= r < off[m + 1] and (not masked or usable[r])
                assert out[m].tobytes() == c["desc"][r].tobytes()
    assert c["ref"][True][0].tolist() != c["ref"][False][0].tolist()  # the mask decides somewhere


@pytest.mark.gpu
@pytest.mark.parametrize("masked", [True, False])
def test_gpu_matches_oracle_across_the_lds_line(masked):
    c = _big()
    off, desc = c["off"], c["desc"]
    cur = np.full((len(off) - 1, 32), 0xAB, np.uint8)
    best, out = compute_distinctive_descriptors(off, desc, c["usable"] if masked else None, current=cur)
    ob, oo = c["ref"][masked]
    assert best.tolist() == ob.tolist()
    for m, r in enumerate(ob):
        assert out[m].tobytes() == (oo[m].tobytes() if r >= 0 else cur[m].tobytes())


# ---- small points with the expected row written out -------------------------------------------
def _star(n, centres, c):
    """n rows: the rows in `centres` are c itself, row j elsewhere is c with bits j and j + 1 (mod
    256) flipped.  From a centre every other row is at distance 2 (median 2 with two centres);
    from another row the centres and its two neighbours are at 2, every other row at 4 (median 4,
    from a dozen rows on)."""
    assert n <= 256
    rows = np.repeat(c[None, :], n, axis=0)
    for j in range(n):
        if j not in centres:
            for b in (j % 256, (j + 1) % 256):
                rows[j, b // 8] ^= np.uint8(1 << (b % 8))
    return rows


def _big_star(n, centres, c, seed):
    """_star at the kernel's limit: row j outside `centres` is c with a pair of bits flipped, the n
    pairs distinct and drawn at random.  From a centre every other row is at distance 2; two other
    rows are at 2 only where their pairs share a bit (about n / 64 of them, far fewer than half), else
    at 4."""
    rng = np.random.default_rng(seed)
    pairs = [(p, q) for p in range(256) for q in range(p + 1, 256)]
    rows = np.repeat(c[None, :], n, axis=0)
    for j, i in enumerate(rng.choice(len(pairs), size=n, replace=False)):
        if j not in centres:
            for b in pairs[i]:
                rows[j, b // 8] ^= np.uint8(1 << (b % 8))
    return rows


def _targeted():
    """[(name, rows, usable, expected row within the point)]"""
    a = np.random.default_rng(11).integers(0, 256, 32, dtype=np.uint8)
    late = np.ones(MAX_OBS, np.uint8)
    late[10] = 0
    na = np.bitwise_not(a)
    ones = lambda n: np.ones(n, np.uint8)  # noqa: E731
    first = ones(130)
    first[0] = 0
    chunk0, chunk1 = ones(200), ones(200)
    chunk0[0:64] = 0
    chunk1[64:128] = 0
    return [
        # N = 2: kmed = 0, both medians are the distance to itself, the first row wins
        ("pair", np.stack([a, na]), ones(2), 0),
        # N = 3: row 0 sees (0, 256, 256), median 256 = the upper end of the kernel's search; rows 1, 2 see
        # (0, 0, 256), median 0, and row 1 is the first of them
        ("complement twice", np.stack([a, na, na]), ones(3), 1),
        # every median 0: the first usable row
        ("identical", np.repeat(a[None, :], 130, axis=0), ones(130), 0),
        ("identical, row 0 unusable", np.repeat(a[None, :], 130, axis=0), first, 1),
        # rows 5 and 69 tie for the least median and are the same lane's first and second round
        ("tie across rounds", _star(130, (5, 69), a), ones(130), 5),
        # a whole 64-row chunk unusable: compacted position and row id differ by 64 from there on
        ("first chunk unusable", _star(200, (10, 100), a), chunk0, 100),
        ("middle chunk unusable", _star(200, (70, 150), a), chunk1, 150),
        # the limit of 4000 observations, the only usable centre in the last round of the lane loop and
        # past the first 64 KB of LDS
        ("late row at the limit", _big_star(MAX_OBS, (10, 3990), a, 3), late, 3990),
    ]


def _targeted_call():
    cases = _targeted()
    off = np.concatenate([[0], np.cumsum([len(r) for _, r, _, _ in cases])]).astype(np.int32)
    desc = np.concatenate([r for _, r, _, _ in cases])
    usable = np.concatenate([u for _, _, u, _ in cases])
    expected = [int(off[m]) + e for m, (_, _, _, e) in enumerate(cases)]
    return off, desc, usable, expected


def test_targeted_points_oracle():
    off, desc, usable, expected = _targeted_call()
    best, out = _oracle(off, desc, usable)
    assert best.tolist() == expected
    assert _numpy(off[:8], desc, usable).tolist() == expected[:7]  # the small points (all pairs in numpy)
    assert out.tobytes() == desc[expected].tobytes()
    # without the masks the earlier centre / the first row wins: the masks are what the cases test
    unmasked = _oracle(off, desc, None)[0] - off[:-1]
    assert unmasked.tolist() == [0, 1, 0, 0, 5, 10, 70, 10]


@pytest.mark.gpu
def test_gpu_targeted_points():
    off, desc, usable, expected = _targeted_call()
    best, out = compute_distinctive_descriptors(off, desc, usable)
    assert best.tolist() == expected
    assert out.tobytes() == desc[expected].tobytes()
    best, out = compute_distinctive_descriptors(off, desc, None)
    assert (best - off[:-1]).tolist() == [0, 1, 0, 0, 5, 10, 70, 10]
    for m, (_, rows, u, e) in enumerate(_targeted()):  # and each point as a call of its own
        best, out = compute_distinctive_descriptors([0, len(rows)], rows, u)
        assert best.tolist() == [e] and out[0].tobytes() == rows[e].tobytes(), m


# ---- refusals and the device entry point --------------------------------------------------------
@pytest.mark.gpu
def test_gpu_refuses_more_than_the_limit():
    rng = np.random.default_rng(5)
    off = np.array([0, 5, 5 + MAX_OBS + 1], np.int32)
    desc = rng.integers(0, 256, (off[-1], 32), dtype=np.uint8)
    best = np.full(2, -7, np.int32)
    cur = np.full((2, 32), 0xAB, np.uint8)
    L = hip_lib()
    assert L.orb_compute_distinctive_descriptors(2, ptr(off), ptr(desc), None, ptr(best), ptr(cur), 0) == ORB_ENOTSUP
    assert b"4000" in L.orb_last_error()
    assert best.tolist() == [-7, -7] and (cur == 0xAB).all()  # nothing written, not even the first point
    with pytest.raises(orb.OrbError) as e:
        compute_distinctive_descriptors(off, desc)
    assert e.value.code == ORB_ENOTSUP
    off = np.array([0, 5, 5 + 300], np.int32)  # the next call works
    best, out = compute_distinctive_descriptors(off, desc[:305])
    ob, oo = _oracle(off, desc[:305], None)
    assert best.tolist() == ob.tolist() and out.tobytes() == oo.tobytes()


@pytest.mark.gpu
def test_gpu_device_entry_point():
    import torch

    c = _big()
    off, desc, usable = c["off"], c["desc"], c["usable"]
    M, R = len(off) - 1, len(desc)
    d_off, d_desc, d_use = (torch.from_numpy(np.array(a)).cuda() for a in (off, desc, usable))

    def fresh():
        return (torch.full((M,), -7, dtype=torch.int32, device="cuda"),
                torch.full((M, 32), 0xAB, dtype=torch.uint8, device="cuda"))

    for masked in (True, False):
        best, out = fresh()
        ret = compute_distinctive_descriptors_device(d_off, d_desc, d_use if masked else None, MAX_OBS, best, out)
        torch.cuda.synchronize()
        assert ret[0] is best and ret[1] is out
        hb, ho = compute_distinctive_descriptors(off, desc, usable if masked else None,
                                                 current=np.full((M, 32), 0xAB, np.uint8))
        assert best.cpu().numpy().tobytes() == hb.tobytes() and out.cpu().numpy().tobytes() == ho.tobytes()
        assert hb.tolist() == c["ref"][masked][0].tolist()
    # M = 0: nothing to do
    empty_i, empty_d = torch.empty((0,), dtype=torch.int32, device="cuda"), torch.empty((0, 32), dtype=torch.uint8,
                                                                                        device="cuda")
    compute_distinctive_descriptors_device(d_off[:1], empty_d, None, 0, empty_i, empty_d)
    # descriptors 8 bytes off a 16-byte boundary
    flat = torch.zeros(R * 32 + 16, dtype=torch.uint8, device="cuda")
    shifted = flat[8:8 + R * 32].view(R, 32)
    assert shifted.data_ptr() % 16 == 8
    best, out = fresh()
    with pytest.raises(orb.OrbError) as e:
        compute_distinctive_descriptors_device(d_off, shifted, None, MAX_OBS, best, out)
    assert e.value.code == ORB_EINVAL
    # one observation more than the kernel holds (refused from max_obs alone, before any launch)
    with pytest.raises(orb.OrbError) as e:
        compute_distinctive_descriptors_device(d_off, d_desc, None, MAX_OBS + 1, best, out)
    assert e.value.code == ORB_ENOTSUP
    torch.cuda.synchronize()
    assert (best == -7).all() and (out == 0xAB).all()
