"""GPU parity of k_match_init's geometric and rotation gates (csrc/orb_sfi.hip) exactly on their
thresholds: the tables of tests/sfi_gate_tables.py, one F1 query per row on / next to a float
comparison of the reference, on a grid or window edge, on a bin boundary or on a non-finite input.

Every row is held to the decision its reference line dictates (stated by the table, confirmed for
the oracle by tests/test_sfi_gate_tables_oracle.py) and to the oracle, bit for bit: vnMatches12,
nmatches and the updated vbPrevMatched, on the first call and on the second call that reads the
vbPrevMatched the first wrote.  Every body of the kernel sees every table:
  * the host call (one pair, 1024 threads, the fixed-point phase 2) with F2 padded to at most 256,
    to 257 .. 512 and to more than 512 octave-0 keypoints (the ranking's 4 / 2 / 1 lanes per key),
    the rows behind a lead of filler queries so that they straddle query 256;
  * the host call with more than 1024 octave-0 keypoints in both frames, the rows straddling query
    1024: the large-capacity body (both-coordinate cell test, global scratch);
  * a batch of 2 pairs (1024 threads, batch addressing), with and without d_prev_xy;
  * a batch of 256 pairs of capacity <= 512 (512 threads, the 8-wave speculated pass, nmax = 256),
    the tables spread over the pairs, some pairs with more than 256 octave-0 keypoints in F2 or F1
    (the in-workgroup large-capacity redo at 512 threads).
A failure names the row (table / rectangle / window, gate, direction, side) and the path.
"""
import numpy as np
import pytest

import orbslam_jpminipc_amd as orb
import sfi_gate_tables as S
from oracle_lib import search_for_initialization
from orbslam_jpminipc_amd._native import FrameBounds

pytestmark = pytest.mark.gpu

NNRATIO = 0.9
TABLES = S.all_tables()


def oracle_calls(T, b, calls=2):
    """[(n, m12, prev after)] of the oracle's first and second call."""
    prev = b["prev"].copy()
    out = []
    for _ in range(calls):
        n, m = search_for_initialization(b["k1"], b["d1"], b["k2"], b["d2"], 0, 0, prev, NNRATIO, T.ori, T.window,
                                         bounds=T.bounds)
        out.append((n, m, prev.copy()))
    return out


def verdict(bad, T, b, path, call, got_n, got_m, got_prev, ref):
    """Append one line per differing row; the table's dictated entries bind the first call."""
    l1, l2 = b["lead1"], b["lead2"]
    rn, rm, rp = ref
    loc = lambda v: int(v) - l2 if v >= 0 else -1  # noqa: E731
    for i, r in enumerate(T.rows):
        g, o = got_m[l1 + i], rm[l1 + i]
        if g != o or (call == 0 and g != b["m12"][l1 + i]):
            bad.append(f"{path}, call {call + 1}: {r}: GPU {loc(g)}, oracle {loc(o)}, dictated {r.expect if call == 0 else '-'}")
    if not np.array_equal(got_m, rm):
        bad.append(f"{path}, call {call + 1}: {T}: vnMatches12 differs from the oracle at {np.flatnonzero(got_m != rm)[:8]}")
    if call == 0 and not np.array_equal(got_m, b["m12"]):
        bad.append(f"{path}, call 1: {T}: vnMatches12 differs from the table at {np.flatnonzero(got_m != b['m12'])[:8]}")
    if got_n != rn or (call == 0 and got_n != b["n"]):
        bad.append(f"{path}, call {call + 1}: {T}: nmatches GPU {got_n}, oracle {rn}")
    if got_prev is not None and got_prev.tobytes() != rp.tobytes():
        bad.append(f"{path}, call {call + 1}: {T}: vbPrevMatched differs from the oracle")


def report(bad):
    assert not bad, "%d difference(s):\n%s" % (len(bad), "\n".join(bad[:60]))


def leads(T, mode):
    nq = len(T.q)
    return {"n2c<=256": (0, 0), "n2c 257..512": (max(0, 256 - nq // 2), 290), "n2c>512": (max(0, 256 - nq // 2), 600),
            "large capacity": (1024 - nq // 2, S.MAX_LEAD2)}[mode]


@pytest.mark.parametrize("mode", ["n2c<=256", "n2c 257..512", "n2c>512", "large capacity"])
def test_host_call(mode):
    bad = []
    for T in TABLES:
        b = T.build(*leads(T, mode))
        n2c = len(b["k2"]) - sum(1 for e in T.q for c in e.cands if c[3] != 0 or not T.G.in_grid(c[0], c[1]))
        lo, hi = {"n2c<=256": (1, 256), "n2c 257..512": (257, 512), "n2c>512": (513, 1024), "large capacity": (1025, 8192)}[mode]
        assert lo <= n2c <= hi, (T, n2c)
        assert (len(b["k1"]) > 1024) == (mode == "large capacity")
        F1, F2 = orb.Frame(b["k1"], b["d1"], 0, 0), orb.Frame(b["k2"], b["d2"], 0, 0)
        for F in (F1, F2):
            F.mnMinX, F.mnMaxX, F.mnMinY, F.mnMaxY = T.bounds
        m = orb.ORBmatcher(NNRATIO, T.ori)
        prev = b["prev"].copy()
        for call, ref in enumerate(oracle_calls(T, b)):
            m12 = []
            n = m.SearchForInitialization(F1, F2, prev, m12, T.window)
            verdict(bad, T, b, f"host call ({mode})", call, n, np.array(m12, np.int32), prev, ref)
    report(bad)


def frames_to_device(builds, cap):
    """Device tensors (kps, desc, counts) of the frames [F1, F2] of every build, and prev (len, cap, 2)."""
    import torch

    nb = len(builds)
    kps = np.zeros((2 * nb, cap, 28), np.uint8)
    desc = np.zeros((2 * nb, cap, 32), np.uint8)
    cnt = np.zeros(2 * nb, np.int32)
    prev = np.zeros((nb, cap, 2), np.float32)
    for j, b in enumerate(builds):
        for f, (k, d) in ((2 * j, (b["k1"], b["d1"])), (2 * j + 1, (b["k2"], b["d2"]))):
            assert len(k) <= cap
            kps[f, : len(k)] = np.frombuffer(np.ascontiguousarray(k).tobytes(), np.uint8).reshape(len(k), 28)
            desc[f, : len(k)] = d
            cnt[f] = len(k)
        prev[j, : len(b["k1"])] = b["prev"]
    t = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    return t(kps), t(desc), t(cnt), prev


@pytest.mark.parametrize("with_prev", [True, False], ids=["prev", "no_prev"])
def test_batch_of_two_pairs(with_prev):
    """Pair 0: the table as built; pair 1: the same table behind 9 filler queries and 5 filler
    keypoints.  Without d_prev_xy the windows sit on the F1 keypoints themselves (which the tables
    place on their vbPrevMatched entries) and nothing is written back."""
    import torch

    bad = []
    for T in TABLES:
        builds = [T.build(0, 0), T.build(9, 5)]
        cap = max(max(len(b["k1"]), len(b["k2"])) for b in builds)
        kps, desc, cnt, prev = frames_to_device(builds, cap)
        d_prev = torch.from_numpy(prev).cuda() if with_prev else None
        f1 = torch.tensor([0, 2], dtype=torch.int32, device="cuda")
        refs = [oracle_calls(T, b) for b in builds]
        for call in range(2 if with_prev else 1):
            m12, nm = orb.ORBmatcher(NNRATIO, T.ori).search_for_initialization_batch_device(
                kps, desc, cnt, f1, f1 + 1, 0, 0, T.window, d_prev_xy=d_prev, bounds=FrameBounds(*T.bounds))
            torch.cuda.synchronize()
            m12, nm = m12.cpu().numpy(), nm.cpu().numpy()
            pg = d_prev.cpu().numpy() if with_prev else None
            for p, b in enumerate(builds):
                n1 = len(b["k1"])
                verdict(bad, T, b, f"batch of 2, pair {p}, {'with' if with_prev else 'without'} d_prev_xy", call, int(nm[p]),
                        m12[p, :n1], pg[p, :n1] if with_prev else None, refs[p][call])
    report(bad)


GROUPS = sorted({(t.rect, t.window, t.ori) for t in TABLES})


@pytest.mark.parametrize("rect,window,ori", GROUPS, ids=[f"{r}-w{w}-{'ori' if o else 'noori'}" for r, w, o in GROUPS])
def test_batch_of_256_pairs(rect, window, ori):
    """256 pairs, capacity <= 512: every table of the group as built (the LDS body at nmax = 256),
    with 300 filler keypoints in F2 and with 300 filler queries in F1 (more than 256 octave-0
    keypoints: redone by the large-capacity body inside the 512-thread workgroup)."""
    import torch

    P = 256
    group = [t for t in TABLES if (t.rect, t.window, t.ori) == (rect, window, ori)]
    builds = [(T, T.build(l1, l2)) for T in group for l1, l2 in ((0, 0), (0, 300), (300, 3))]
    cap = max(max(len(b["k1"]), len(b["k2"])) for _, b in builds)
    assert 256 < cap <= 512
    kps, desc, cnt, prev1 = frames_to_device([b for _, b in builds], cap)
    which = np.arange(P) % len(builds)
    d_prev = torch.from_numpy(np.ascontiguousarray(prev1[which])).cuda()
    f1 = torch.from_numpy((2 * which).astype(np.int32)).cuda()
    refs = [oracle_calls(T, b) for T, b in builds]
    bad = []
    for call in range(2):
        m12, nm = orb.ORBmatcher(NNRATIO, ori).search_for_initialization_batch_device(
            kps, desc, cnt, f1, f1 + 1, 0, 0, window, d_prev_xy=d_prev, bounds=FrameBounds(*S.RECTS[rect]))
        torch.cuda.synchronize()
        m12, nm, pg = m12.cpu().numpy(), nm.cpu().numpy(), d_prev.cpu().numpy()
        for p in range(P):
            T, b = builds[which[p]]
            n1 = len(b["k1"])
            verdict(bad, T, b, f"batch of 256, pair {p} (leads {b['lead1']}, {b['lead2']})", call, int(nm[p]), m12[p, :n1],
                    pg[p, :n1], refs[which[p]][call])
    report(bad)
