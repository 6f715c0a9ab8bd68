"""GPU parity of the local map (csrc/orb_localmapref.hip: orb_local_map_reference,
orb_keyframe_update_connections and their batch forms) against the plain-Python model
(tests/local_map_model.py).

Everything is integer: every output is compared for equality, with nothing left out (the frame's row,
both lists, seen, the vote table and every field of the record).  The shapes are the smallest at which
each mechanism can go wrong (a wave, the workgroup, a packed counter's halves, the limit of 80, the row
block, the chunk), not a map's own size."""
import numpy as np
import pytest

import orbslam_jpminipc_amd as orb
from orbslam_jpminipc_amd import _native
from orbslam_jpminipc_amd.local_map import frame_scratch_bytes, keyframe_scratch_bytes
import local_map_model as lm
import local_map_scenes as sc
from local_map_model import Tables

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A
REC = ("n_voted", "n_local_kf", "ref_kf", "ref_votes", "n_local_pt", "n_cleared")
LISTS = ("f_mp_out", "local_kf", "local_pt", "local_pt_seen", "kf_votes")
CONN = ("conn_kf", "conn_w", "ord_kf", "ord_w")


@pytest.fixture(scope="module")
def L():
    h = orb.LocalMap(0)
    yield h
    h.set_scratch_cap(0)


def tables(T: Tables) -> orb.MapTables:
    return orb.MapTables(**T.arrays())


def same_reference(got, want, what=""):
    assert got["status"] == 0, what
    for k in REC:
        assert got[k] == want[k], f"{what}: {k} {got[k]} != {want[k]}"
    # the vote table first: a wrong count then fails here, a wrong order below
    for k in ("kf_votes", "f_mp_out", "local_kf", "local_pt", "local_pt_seen"):
        if k in got:
            assert np.asarray(got[k]).tolist() == list(want[k]), f"{what}: {k} differs"


def check_frames(L, T, frames, what=""):
    mt = tables(T)
    for i, fr in enumerate(frames):
        same_reference(L.reference(mt, fr, votes=True), lm.local_map_reference(T, fr), f"{what} frame {i}")


def same_connections(got, want, what=""):
    assert got["status"] == 0 and got["unchanged"] == want["unchanged"], what
    assert got["n_conn"] == len(want["conn_kf"]) and got["n_ord"] == len(want["ord_kf"]), what
    for k in CONN:
        assert np.asarray(got[k]).tolist() == list(want[k]), f"{what}: {k} differs"


# ---- call 1: the scan's wave and workgroup edges --------------------------------------------------

@pytest.mark.parametrize("n_kf", [1, 2, 63, 64, 65, 257, 513, 1025])
def test_keyframe_counts_at_wave_and_workgroup_edges(L, n_kf):
    # a frame that votes for most keyframes: one point of every keyframe's row
    T = sc.random_map(100 + n_kf, n_kf, 4 * n_kf + 8, 6, p_kf_bad=0.15)
    wide = [next((p for p in row if p >= 0), -1) for row in T.kf_mp]
    frames = [wide, sc.random_frame(1, T, 40), sc.random_frame(2, T, 7, around=n_kf - 1)]
    want = lm.local_map_reference(T, wide)
    assert n_kf < 64 or want["n_voted"] > 0.5 * n_kf  # the voted list really crosses the edges
    check_frames(L, T, frames, f"n_kf={n_kf}")


def test_packed_counter_halves_at_their_largest_counts(L):
    T, frame = sc.packed_counter_extremes()
    want = lm.local_map_reference(T, frame)
    assert [want["kf_votes"][k] for k in (65533, 65534, 65535)] == [1, 8192, 8191] and want["ref_kf"] == 65534
    same_reference(L.reference(tables(T), frame, votes=True), want)


@pytest.mark.parametrize("n_voted", [79, 80, 81, 82])
def test_limit_of_80_with_eligible_neighbours(L, n_voted):
    T, frame = sc.voted_chain(n_voted)
    want = lm.local_map_reference(T, frame)
    assert want["n_local_kf"] == (81 if n_voted <= 80 else n_voted)
    same_reference(L.reference(tables(T), frame, votes=True), want)
    # one voted keyframe bad: the list before the neighbour step is one shorter than the vote
    T, frame = sc.voted_chain(n_voted, bad_voted=(3,))
    same_reference(L.reference(tables(T), frame, votes=True), lm.local_map_reference(T, frame), "one voted bad")


def test_neighbour_loop_visits_the_voted_list_only(L):
    # keyframe 0's neighbour is 1, whose neighbour is 2: a loop over the growing list would append 2 as well
    T = sc.consistent([[0], [], []], 1, kf_cov=[[1], [2], []])
    got = L.reference(tables(T), [0], votes=True)
    assert got["local_kf"].tolist() == [0, 1]
    same_reference(got, lm.local_map_reference(T, [0]))


def test_neighbour_rows_empty_all_bad_all_present(L):
    T, frame = sc.neighbour_rows()
    want = lm.local_map_reference(T, frame)
    assert want["local_kf"] == [0, 1, 2, 3, 4, 10]  # and a local keyframe (10) with zero keypoints
    same_reference(L.reference(tables(T), frame, votes=True), want)


def test_tie_bad_keyframe_and_bad_frame_point(L):
    T = sc.consistent([[], [0, 1], [], [0, 1]], 2)
    same_reference(L.reference(tables(T), [0, 1], votes=True), lm.local_map_reference(T, [0, 1]), "tie")
    T = sc.consistent([[0, 1, 2], [0], [1]], 3, kf_bad=[1, 0, 0])
    same_reference(L.reference(tables(T), [0, 1, 2], votes=True), lm.local_map_reference(T, [0, 1, 2]), "bad kf")
    # point 1 is bad and would be the only vote for keyframe 1; it is also held twice
    T = Tables([0, 0], [[0], [1]], [[], []], [0, 1], [[0], [1]])
    got = L.reference(tables(T), [0, 1, -1, 1], votes=True)
    assert got["kf_votes"].tolist() == [1, 0] and got["f_mp_out"].tolist() == [0, -1, -1, -1] and got["n_cleared"] == 2
    same_reference(got, lm.local_map_reference(T, [0, 1, -1, 1]), "bad frame point")


def test_seen_and_frame_points_stay_local(L):
    T = sc.consistent([[0, 1, 2, 3]], 4, pt_bad=[0, 0, 1, 0])
    got = L.reference(tables(T), [3, -1, 0, 2], votes=True)
    assert got["local_pt"].tolist() == [0, 1, 3] and got["local_pt_seen"].tolist() == [1, 0, 1]
    same_reference(got, lm.local_map_reference(T, [3, -1, 0, 2]))


@pytest.mark.parametrize("row_len", [1, 255, 256, 257])
def test_one_local_row_at_the_row_block_edges(L, row_len):
    T, frame = sc.shared_rows(1, row_len, max(2, row_len // 3))
    want = lm.local_map_reference(T, frame)
    assert want["n_local_kf"] == 1
    same_reference(L.reference(tables(T), frame, votes=True), want)


def test_twenty_thousand_entries_with_heavy_sharing(L):
    T, frame = sc.shared_rows(110, 183, 1500)  # 20130 entries over 1500 points, more rows than row blocks
    want = lm.local_map_reference(T, frame)
    assert want["n_local_kf"] == 110 and 1300 < want["n_local_pt"] <= 1500
    same_reference(L.reference(tables(T), frame, votes=True), want)


def test_first_occurrence_in_the_last_keypoint_of_the_last_keyframe(L):
    T, frame = sc.last_is_first()
    want = lm.local_map_reference(T, frame)
    assert want["local_pt"][-1] == 7
    same_reference(L.reference(tables(T), frame, votes=True), want)


def test_empty_frame_and_all_bad_frame(L):
    T = sc.random_map(9, 20, 60, 12, p_pt_bad=0.3)
    bad = [p for p in range(T.n_pt) if T.pt_bad[p]]
    assert len(bad) >= 3
    for fr in ([], [-1, -1, -1], bad, bad + [-1] + bad):
        got = L.reference(tables(T), fr, votes=True)
        assert got["ref_kf"] == -1 and got["n_local_kf"] == 0 and got["n_local_pt"] == 0
        assert len(got["local_kf"]) == 0 and len(got["local_pt"]) == 0
        same_reference(got, lm.local_map_reference(T, fr))


def test_null_vote_table_and_repeatable_bytes(L):
    T = sc.random_map(4, 65, 300, 20)
    fr = sc.random_frame(5, T, 50)
    mt = tables(T)
    a, b, c = L.reference(mt, fr, votes=True), L.reference(mt, fr, votes=True), L.reference(mt, fr, votes=False)
    assert "kf_votes" not in c
    for k in LISTS:
        assert a[k].tobytes() == b[k].tobytes(), k
        if k != "kf_votes":
            assert a[k].tobytes() == c[k].tobytes(), k
    same_reference(c, lm.local_map_reference(T, fr), "NULL kf_votes")


# ---- call 1: refusals -----------------------------------------------------------------------------

def poisoned(n, cap_kf, cap_pt):
    return dict(f_mp_out=np.full(max(n, 1), POISON, np.int32), local_kf=np.full(max(cap_kf, 1), POISON, np.int32),
                local_pt=np.full(max(cap_pt, 1), POISON, np.int32), local_pt_seen=np.full(max(cap_pt, 1), 0x5A, np.uint8))


def test_capacity_too_small_reports_counts_and_writes_nothing(L):
    T = sc.random_map(4, 65, 300, 20)
    fr = sc.random_frame(5, T, 50)
    want = lm.local_map_reference(T, fr)
    nk, npt = want["n_local_kf"], want["n_local_pt"]
    assert nk > 2 and npt > 2
    for cap_kf, cap_pt in ((nk - 1, npt), (nk, npt - 1), (0, 0)):
        out = poisoned(len(fr), cap_kf, cap_pt)
        with pytest.raises(orb.OrbError) as e:
            L.reference(tables(T), fr, cap_kf=cap_kf, cap_pt=cap_pt, out=out)
        assert e.value.code == _native.ORB_ERANGE
        assert e.value.info["status"] == _native.ORB_ERANGE
        for k in REC:
            assert e.value.info[k] == want[k], k
        assert all((v == (0x5A if v.dtype == np.uint8 else POISON)).all() for v in out.values())
    # exactly enough: written to the count, poison after it
    out = poisoned(len(fr), nk + 2, npt + 2)
    got = L.reference(tables(T), fr, cap_kf=nk + 2, cap_pt=npt + 2, out=out)
    same_reference(got, want)
    assert (out["local_kf"][nk:] == POISON).all() and (out["local_pt"][npt:] == POISON).all()
    assert (out["local_pt_seen"][npt:] == 0x5A).all()


def _broken(T, **change):
    a = T.arrays()
    for k, f in change.items():
        a[k] = f(a[k].copy())
    return orb.MapTables(**a)


def _set(i, v):
    def f(a):
        a.reshape(-1)[i] = v
        return a
    return f


def test_bad_tables_are_einval(L):
    T = sc.random_map(4, 20, 90, 12, p_null=0.1)
    fr = sc.random_frame(5, T, 30)
    a = T.arrays()
    long_row = int(np.argmax(np.diff(a["pt_obs_off"])))
    lo = int(a["pt_obs_off"][long_row])
    assert a["pt_obs_off"][long_row + 1] - lo >= 2
    cases = {
        "kf_mp point index too large": dict(kf_mp=_set(3, T.n_pt)),
        "kf_mp below -1": dict(kf_mp=_set(3, -2)),
        "kf_cov keyframe index too large": dict(kf_cov=_set(7, T.n_kf)),
        "kf_cov below -1": dict(kf_cov=_set(7, -3)),
        "pt_obs_kf too large": dict(pt_obs_kf=_set(len(a["pt_obs_kf"]) - 1, T.n_kf)),
        "pt_obs_kf negative": dict(pt_obs_kf=_set(0, -1)),
        "observation row with a duplicate": dict(pt_obs_kf=_set(lo + 1, int(a["pt_obs_kf"][lo]))),
        "observation row descending": dict(pt_obs_kf=lambda v: _swap(v, lo)),
        "kf_mp_off not monotone": dict(kf_mp_off=_set(5, int(a["kf_mp_off"][6]) + 1)),
        "kf_mp_off leaves the array": dict(kf_mp_off=_set(T.n_kf, len(a["kf_mp"]) + 1)),
        "kf_mp_off negative": dict(kf_mp_off=_set(0, -1)),
        "pt_obs_off not monotone": dict(pt_obs_off=_set(5, int(a["pt_obs_off"][6]) + 1)),
        "pt_obs_off leaves the array": dict(pt_obs_off=_set(T.n_pt, len(a["pt_obs_kf"]) + 1)),
    }
    for what, change in cases.items():
        with pytest.raises(orb.OrbError) as e:
            L.reference(_broken(T, **change), fr)
        assert e.value.code == _native.ORB_EINVAL, what
        with pytest.raises(orb.OrbError) as e:
            L.update_connections(_broken(T, **change), [0, 1])
        assert e.value.code == _native.ORB_EINVAL, what
    for bad_fr in ([0, T.n_pt], [-2, 0]):
        with pytest.raises(orb.OrbError) as e:
            L.reference(tables(T), bad_fr)
        assert e.value.code == _native.ORB_EINVAL
    for bad_k in ([T.n_kf], [0, -1]):
        with pytest.raises(orb.OrbError) as e:
            L.update_connections(tables(T), bad_k)
        assert e.value.code == _native.ORB_EINVAL
    # the untouched tables pass
    same_reference(L.reference(tables(T), fr, votes=True), lm.local_map_reference(T, fr))


def _swap(v, lo):
    v[lo], v[lo + 1] = v[lo + 1], v[lo]
    return v


def test_sizes_above_the_limits_are_enotsup(L):
    import torch

    T = sc.random_map(4, 20, 90, 12)
    mt = tables(T)
    with pytest.raises(orb.OrbError) as e:  # a frame of more than 8192 slots
        L.reference(mt, [-1] * 8193)
    assert e.value.code == _native.ORB_ENOTSUP
    same_reference(L.reference(mt, [-1] * 8192, votes=True), lm.local_map_reference(T, [-1] * 8192), "8192 slots")
    # a keyframe row of 8193 entries (8192 passes)
    for n, ok in ((8192, True), (8193, False)):
        Tl = Tables([0], [[0] * n], [[]], [0], [[0]])
        if ok:
            same_reference(L.reference(tables(Tl), [0], votes=True), lm.local_map_reference(Tl, [0]), "row of 8192")
            same_connections(L.update_connections(tables(Tl), [0])[0], lm.update_connections(Tl, 0))
        else:
            for call in (lambda: L.reference(tables(Tl), [0]), lambda: L.update_connections(tables(Tl), [0])):
                with pytest.raises(orb.OrbError) as e:
                    call()
                assert e.value.code == _native.ORB_ENOTSUP
    # more than 65536 keyframes
    n = 65537
    big = orb.MapTables(np.zeros(n, np.uint8), np.zeros(n + 1, np.int32), np.zeros(0, np.int32),
                        np.full((n, 10), -1, np.int32), np.zeros(1, np.uint8), np.zeros(2, np.int32), np.zeros(0, np.int32))
    for call in (lambda: L.reference(big, [0]), lambda: L.update_connections(big, [0])):
        with pytest.raises(orb.OrbError) as e:
            call()
        assert e.value.code == _native.ORB_ENOTSUP
    # more than 65535 frames / keyframes in a batch, and a frame row above 8192, from the sizes alone
    dt = mt.to("cuda")
    z = torch.zeros((65536, 1), dtype=torch.int32, device="cuda")
    with pytest.raises(orb.OrbError) as e:
        L.reference_batch_device(dt, z, z[:, 0].contiguous(), 4, 4)
    assert e.value.code == _native.ORB_ENOTSUP
    with pytest.raises(orb.OrbError) as e:
        L.update_connections_batch_device(dt, z[:, 0].contiguous(), 4, 4)
    assert e.value.code == _native.ORB_ENOTSUP
    z = torch.zeros((1, 8193), dtype=torch.int32, device="cuda")
    with pytest.raises(orb.OrbError) as e:
        L.reference_batch_device(dt, z, torch.zeros(1, dtype=torch.int32, device="cuda"), 4, 4)
    assert e.value.code == _native.ORB_ENOTSUP


def test_scratch_cap_below_one_frame_is_enotsup(L):
    T = sc.random_map(4, 64, 300, 20)
    fr = sc.random_frame(5, T, 50)
    mt = tables(T)
    try:
        for votes in (False, True):
            need = frame_scratch_bytes(T.n_kf, T.n_pt, votes)
            L.set_scratch_cap(need - 1)
            with pytest.raises(orb.OrbError) as e:
                L.reference(mt, fr, votes=votes)
            assert e.value.code == _native.ORB_ENOTSUP
            L.set_scratch_cap(need)
            same_reference(L.reference(mt, fr, votes=votes), lm.local_map_reference(T, fr))
        need = keyframe_scratch_bytes(T.n_kf)
        L.set_scratch_cap(need - 1)
        with pytest.raises(orb.OrbError) as e:
            L.update_connections(mt, [0])
        assert e.value.code == _native.ORB_ENOTSUP
        L.set_scratch_cap(need)
        same_connections(L.update_connections(mt, [3])[0], lm.update_connections(T, 3))
    finally:
        L.set_scratch_cap(0)


# ---- call 1: the batch form -----------------------------------------------------------------------

def test_batch_equals_host_form_byte_for_byte_in_two_chunks(L):
    import torch

    T = sc.random_map(4, 64, 300, 20)
    mt = tables(T)
    dt = mt.to("cuda")
    cap, cap_kf, cap_pt = 60, 64, 300
    rng = np.random.default_rng(3)
    frames = [sc.random_frame(10, T, 50), sc.random_frame(11, T, 60, around=3), [], sc.random_frame(12, T, 1),
              sc.random_frame(13, T, 33, around=40)]
    f_mp = rng.integers(-5, T.n_pt + 5, (5, cap)).astype(np.int32)  # garbage past each count, out of range too
    for b, fr in enumerate(frames):
        f_mp[b, :len(fr)] = fr
    counts = np.array([len(fr) for fr in frames], np.int32)

    def run():
        out = dict(f_mp_out=torch.full((5, cap), POISON, dtype=torch.int32, device="cuda"),
                   local_kf=torch.full((5, cap_kf), POISON, dtype=torch.int32, device="cuda"),
                   local_pt=torch.full((5, cap_pt), POISON, dtype=torch.int32, device="cuda"),
                   local_pt_seen=torch.full((5, cap_pt), 0x5A, dtype=torch.uint8, device="cuda"),
                   kf_votes=torch.full((5, T.n_kf), POISON, dtype=torch.int32, device="cuda"))
        o = L.reference_batch_device(dt, torch.from_numpy(f_mp).cuda(), torch.from_numpy(counts).cuda(), cap_kf, cap_pt,
                                     votes=True, out=out)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in o.items()}

    try:
        whole = run()
        L.set_scratch_cap(3 * frame_scratch_bytes(T.n_kf, T.n_pt, True))  # chunks of 3 and 2 frames
        chunked = run()
        again = run()
    finally:
        L.set_scratch_cap(0)
    for k in whole:
        assert whole[k].tobytes() == chunked[k].tobytes() == again[k].tobytes(), k
    for b, fr in enumerate(frames):
        out = poisoned(cap, cap_kf, cap_pt)
        h = L.reference(mt, fr, cap_kf=cap_kf, cap_pt=cap_pt, votes=True, out=out)
        same_reference(h, lm.local_map_reference(T, fr), f"frame {b}")
        assert [int(v) for v in whole["info"][b]] == [0] + [h[k] for k in REC]
        for k in ("f_mp_out", "local_kf", "local_pt", "local_pt_seen"):
            assert whole[k][b].tobytes() == out[k].tobytes(), (b, k)  # the poison past the counts included
        assert whole["kf_votes"][b].tobytes() == h["kf_votes"].tobytes()


def test_batch_reports_each_frame_status(L):
    import torch

    T = sc.random_map(4, 64, 300, 20)
    dt = tables(T).to("cuda")
    good = sc.random_frame(10, T, 20)
    want = lm.local_map_reference(T, good)
    f_mp = np.full((4, 24), -1, np.int32)
    f_mp[0, :20] = good
    f_mp[1, :20] = good
    f_mp[1, 7] = T.n_pt  # out of range
    f_mp[2, :20] = good
    f_mp[3, :20] = good
    counts = torch.tensor([20, 20, 25, 20], dtype=torch.int32, device="cuda")  # frame 2: a count above cap
    cap_pt = want["n_local_pt"]
    o = L.reference_batch_device(dt, torch.from_numpy(f_mp).cuda(), counts, want["n_local_kf"], cap_pt)
    torch.cuda.synchronize()
    info = o["info"].cpu().numpy()
    assert info[:, 0].tolist() == [0, _native.ORB_EINVAL, _native.ORB_EINVAL, 0]
    assert info[1, 1:].tolist() == [0, 0, -1, 0, 0, 0]
    for b in (0, 3):
        assert o["local_pt"][b].cpu().numpy().tolist() == want["local_pt"]
    # one slot less for the points: every frame reports -34 with the counts, the call itself is OK
    o = L.reference_batch_device(dt, torch.from_numpy(f_mp).cuda(), counts, want["n_local_kf"], cap_pt - 1)
    torch.cuda.synchronize()
    info = o["info"].cpu().numpy()
    assert info[0].tolist() == [_native.ORB_ERANGE] + [want[k] for k in REC]
    assert int(o["local_pt"].abs().sum()) == 0 and int(o["f_mp_out"].abs().sum()) == 0  # nothing written
    # broken tables refuse every frame
    a = T.arrays()
    a["kf_mp"][3] = T.n_pt
    o = L.reference_batch_device(orb.MapTables(**a).to("cuda"), torch.from_numpy(f_mp).cuda(), counts, 8, 8)
    torch.cuda.synchronize()
    assert o["info"][:, 0].cpu().numpy().tolist() == [_native.ORB_EINVAL] * 4


# ---- call 2 ---------------------------------------------------------------------------------------

def test_update_connections_hand_cases(L):
    T = sc.connections_scene()
    mt = tables(T)
    got = L.update_connections(mt, [0])  # K = 1
    assert got[0]["ord_kf"].tolist() == [5, 4, 3, 2] and got[0]["ord_w"].tolist() == [20, 16, 16, 15]
    same_connections(got[0], lm.update_connections(T, 0))
    ks = [6, 9, 0, 7, 5, 1, 0]  # K = 7: the fallback's tie, the empty counter, a bad keyframe's own, a repeat
    got = L.update_connections(mt, ks)
    assert got[0]["ord_kf"].tolist() == [7] and got[1]["unchanged"] == 1
    for g, k in zip(got, ks):
        same_connections(g, lm.update_connections(T, k), f"keyframe {k}")


@pytest.mark.parametrize("n_kf", [1, 2, 63, 64, 65, 257, 600])
def test_update_connections_random_maps(L, n_kf):
    # rows of 40 from a window of 60 points: neighbours share tens of points, so weights straddle 15
    T = sc.random_map(7 + n_kf, n_kf, 12 * n_kf + 60, 40, p_null=0.1, p_kf_bad=0.2, window=60)
    ks = sorted(set([0, n_kf - 1, n_kf // 2, min(n_kf - 1, 64)]))
    want = [lm.update_connections(T, k) for k in ks]
    assert n_kf < 63 or any(w["ord_w"][0] >= 15 for w in want if w["ord_w"])
    for g, w, k in zip(L.update_connections(tables(T), ks), want, ks):
        same_connections(g, w, f"keyframe {k}")


def test_update_connections_many_ordered_entries(L):
    # keyframe 0 shares 15 + (k % 3) points with each of 299 others: a sort over more keys than threads in
    # a wave, with many equal weights
    n_kf = 300
    kf_mp = [[] for _ in range(n_kf)]
    nxt = 0
    for k in range(1, n_kf):
        for _ in range(15 + k % 3):
            kf_mp[0].append(nxt), kf_mp[k].append(nxt)
            nxt += 1
    T = sc.consistent(kf_mp, nxt)
    want = lm.update_connections(T, 0)
    assert len(want["ord_kf"]) == 299 and want["ord_kf"][:2] == [299, 296]
    same_connections(L.update_connections(tables(T), [0])[0], want)


def test_update_connections_capacity(L):
    T = sc.connections_scene()
    mt = tables(T)
    with pytest.raises(orb.OrbError) as e:
        L.update_connections(mt, [6, 0], cap_conn=4, cap_ord=4)  # keyframe 0 has 5 connections
    assert e.value.code == _native.ORB_ERANGE
    assert [r["status"] for r in e.value.info] == [0, _native.ORB_ERANGE]
    assert (e.value.info[1]["n_conn"], e.value.info[1]["n_ord"]) == (5, 4)
    with pytest.raises(orb.OrbError) as e:
        L.update_connections(mt, [0], cap_conn=5, cap_ord=3)
    assert e.value.code == _native.ORB_ERANGE and e.value.info[0]["n_ord"] == 4
    same_connections(L.update_connections(mt, [0], cap_conn=5, cap_ord=4)[0], lm.update_connections(T, 0))


def test_update_connections_batch_equals_host_form_in_two_chunks(L):
    import torch

    T = sc.connections_scene()
    mt = tables(T)
    dt = mt.to("cuda")
    ks = [0, 9, 6, 7, 3]  # 9: unchanged
    cap = 6

    def run():
        out = {k: torch.full((len(ks), cap), POISON, dtype=torch.int32, device="cuda") for k in CONN}
        o = L.update_connections_batch_device(dt, torch.tensor(ks, dtype=torch.int32, device="cuda"), cap, cap, out=out)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in o.items()}

    try:
        whole = run()
        L.set_scratch_cap(3 * keyframe_scratch_bytes(T.n_kf))
        chunked = run()
    finally:
        L.set_scratch_cap(0)
    for k in whole:
        assert whole[k].tobytes() == chunked[k].tobytes(), k
    host = L.update_connections(mt, ks, cap_conn=cap, cap_ord=cap)
    for q, k in enumerate(ks):
        w = lm.update_connections(T, k)
        same_connections(host[q], w, f"keyframe {k}")
        assert whole["info"][q].tolist() == [0, len(w["conn_kf"]), len(w["ord_kf"]), w["unchanged"]]
        for name in CONN:
            n = len(w[name])
            assert whole[name][q, :n].tolist() == list(w[name]) and (whole[name][q, n:] == POISON).all(), (k, name)
    assert whole["info"][1].tolist() == [0, 0, 0, 1]


# ---- the order is what the matcher consumes -------------------------------------------------------

def test_local_points_feed_the_frustum_and_the_projection_matcher(L):
    import scenes as S
    from orbslam_jpminipc_amd.views import MapPointSet

    rng = np.random.default_rng(23)
    F = S.view(rng, 220, clusters=6, spread=20)
    mps, src = S.map_points_on(rng, F, 200, bad_frac=0.0)
    n_pt = mps.n
    # 6 keyframes hold random thirds of the map in random order; the frame already holds a few points
    kf_mp = [[int(p) for p in rng.permutation(n_pt)[:70]] for _ in range(6)]
    T = sc.consistent(kf_mp, n_pt, pt_bad=(rng.random(n_pt) < 0.05).astype(int), kf_cov=[[(k + 1) % 6] for k in range(6)])
    f_mp = np.full(F.n, -1, np.int32)
    for p in rng.permutation(n_pt)[:25]:
        f_mp[src[p]] = p
    got = L.reference(tables(T), f_mp)
    want = lm.local_map_reference(T, f_mp)
    m = orb.ORBmatcher(0.8, True)

    def track(local_pt, seen, f_out):
        lp = np.asarray(local_pt, np.int64)
        sub = MapPointSet(mps.pos[lp], mps.normal[lp], mps.dmin[lp], mps.dmax[lp], mps.desc[lp])
        iv, px, py, lv, vc = m.isInFrustum(F, sub, 0.5)
        usable = iv & (1 - np.asarray(seen, np.uint8))
        taken = (np.asarray(f_out) >= 0).astype(np.uint8)
        n, match = m.SearchByProjection_Local(F, taken, usable, px, py, lv, vc, sub.desc, 3.0)
        return n, lp[match[match >= 0]].tolist(), match

    n_g, pts_g, match_g = track(got["local_pt"], got["local_pt_seen"], got["f_mp_out"])
    n_w, pts_w, match_w = track(want["local_pt"], want["local_pt_seen"], want["f_mp_out"])
    assert n_w > 0 and sum(want["local_pt_seen"]) > 5
    assert n_g == n_w and match_g.tolist() == match_w.tolist() and pts_g == pts_w
