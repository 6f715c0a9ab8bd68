"""The local-map yardstick proved by hand (tests/local_map_model.py): every expected
value below is written out from the reference's lines on tables small enough to read, never computed by
the code under test.  No GPU."""
import numpy as np

import local_map_model as lm
import local_map_scenes as sc
from local_map_model import Tables


def test_tie_for_the_maximum_goes_to_the_lowest_index():
    # points 0, 1 seen by keyframes 1 and 3; `>` at line 840 keeps the first of the equal counts
    T = sc.consistent([[], [0, 1], [], [0, 1]], 2)
    r = lm.local_map_reference(T, [0, 1])
    assert r["kf_votes"] == [0, 2, 0, 2]
    assert (r["ref_kf"], r["ref_votes"]) == (1, 2)
    assert r["local_kf"] == [1, 3] and r["n_voted"] == 2


def test_voted_bad_keyframe_is_skipped_and_cannot_be_the_reference():
    # keyframe 0 has the most votes but is bad: not in the list, not pKFmax; its vote count stays in the counter
    T = sc.consistent([[0, 1, 2], [0], [1]], 3, kf_bad=[1, 0, 0])
    r = lm.local_map_reference(T, [0, 1, 2])
    assert r["kf_votes"] == [3, 1, 1]
    assert r["local_kf"] == [1, 2] and (r["ref_kf"], r["ref_votes"]) == (1, 1)
    # the bad keyframe's points are not local points: only rows 1 and 2 are walked
    assert r["local_pt"] == [0, 1]
    # all voted keyframes bad: no reference
    T = sc.consistent([[0]], 1, kf_bad=[1])
    r = lm.local_map_reference(T, [0])
    assert r["ref_kf"] == -1 and r["local_kf"] == [] and r["local_pt"] == [] and r["n_voted"] == 0


def test_neighbour_rows_bad_present_then_eligible():
    T, frame = sc.neighbour_rows()
    r = lm.local_map_reference(T, frame)
    # visits: 0 (empty row), 1 (8, 9 bad), 2 (0, 1, 3 in the list), 3 (8 bad, 2 present, 10 eligible: 11 not
    # reached), 4 (-1 ends the row before 11)
    assert r["local_kf"] == [0, 1, 2, 3, 4, 10]
    assert r["n_voted"] == 5 and r["n_local_kf"] == 6


def test_list_stops_at_81():
    # 79 voted: size() > 80 is tested before each visit; the sizes it sees are 79, 80 and 81, so two
    # visits append (keyframe 0's neighbour 79, keyframe 1's neighbour 80) and the third breaks
    T, frame = sc.voted_chain(79)
    r = lm.local_map_reference(T, frame)
    assert r["local_kf"] == list(range(79)) + [79, 80] and r["n_local_kf"] == 81
    # 80 voted: one visit appends (80 -> 81), the next sees 81 > 80
    T, frame = sc.voted_chain(80)
    r = lm.local_map_reference(T, frame)
    assert r["local_kf"] == list(range(80)) + [80] and r["n_local_kf"] == 81
    # 1 voted: the loop visits the voted list only (itEndKF fixed): exactly one neighbour, not a chain
    T = sc.consistent([[0], [], []], 1, kf_cov=[[1], [2], []])
    assert lm.local_map_reference(T, [0])["local_kf"] == [0, 1]


def test_nothing_appended_when_81_are_voted():
    for n in (81, 82):
        T, frame = sc.voted_chain(n)
        r = lm.local_map_reference(T, frame)
        assert r["local_kf"] == list(range(n)) and r["n_voted"] == n


def test_shared_point_kept_at_its_first_occurrence():
    T = sc.consistent([[5, 1, 5, 2], [2, 3, 1]], 6)
    r = lm.local_map_reference(T, [1])
    assert r["local_kf"] == [0, 1]
    assert r["local_pt"] == [5, 1, 2, 3]
    T, frame = sc.last_is_first()
    r = lm.local_map_reference(T, frame)
    assert r["local_kf"] == [0, 1, 2] and r["local_pt"] == [0, 1, 2, 3, 7]


def test_bad_frame_point_is_cleared_and_does_not_vote():
    # point 1 is bad: keyframe 1 (seen only through it) gets no vote, the slot comes back NULL
    T = Tables([0, 0], [[0], [1]], [[], []], [0, 1], [[0], [1]])
    r = lm.local_map_reference(T, [0, 1, -1, 1])
    assert r["f_mp_out"] == [0, -1, -1, -1] and r["n_cleared"] == 2
    assert r["kf_votes"] == [1, 0] and r["local_kf"] == [0]
    # a frame whose points are all bad, and an empty frame
    r = lm.local_map_reference(T, [1, 1])
    assert r["f_mp_out"] == [-1, -1] and r["local_kf"] == [] and r["local_pt"] == [] and r["ref_kf"] == -1
    r = lm.local_map_reference(T, [])
    assert r["local_kf"] == [] and r["local_pt"] == [] and r["ref_kf"] == -1 and r["n_cleared"] == 0


def test_seen_marks_the_points_the_frame_holds():
    # the frame's own points are not excluded from the local points (step 4); they are flagged
    T = sc.consistent([[0, 1, 2, 3]], 4, pt_bad=[0, 0, 1, 0])
    r = lm.local_map_reference(T, [3, -1, 0, 2])
    assert r["local_pt"] == [0, 1, 3]
    assert r["local_pt_seen"] == [1, 0, 1]
    assert r["f_mp_out"] == [3, -1, 0, -1]


def test_update_connections_threshold_order_and_bad_keyframe():
    T = sc.connections_scene()
    r = lm.update_connections(T, 0)
    # itself excluded; the bad keyframe 5 counts; 14 is below the threshold but stays in the counter
    assert r["conn_kf"] == [1, 2, 3, 4, 5] and r["conn_w"] == [14, 15, 16, 16, 20]
    # weight descending, and 4 before 3 among the equal weights (sort ascending, then push_front)
    assert r["ord_kf"] == [5, 4, 3, 2] and r["ord_w"] == [20, 16, 16, 15]
    assert r["unchanged"] == 0


def test_update_connections_fallback_takes_the_first_maximum():
    T = sc.connections_scene()
    r = lm.update_connections(T, 6)
    assert r["conn_kf"] == [7, 8] and r["conn_w"] == [3, 3]
    assert r["ord_kf"] == [7] and r["ord_w"] == [3]
    # seen from the other side: keyframe 7 is connected to 6 only
    r = lm.update_connections(T, 7)
    assert r["conn_kf"] == [6] and r["ord_kf"] == [6] and r["ord_w"] == [3]


def test_update_connections_empty_counter():
    T = sc.connections_scene()
    r = lm.update_connections(T, 9)  # one bad point, one NULL
    assert r == dict(conn_kf=[], conn_w=[], ord_kf=[], ord_w=[], unchanged=1)
    # a keyframe alone with its points: only itself observes them
    T = sc.consistent([[0, 1]], 2)
    assert lm.update_connections(T, 0)["unchanged"] == 1


def test_tables_flatten_as_the_abi_takes_them():
    T = sc.consistent([[0, -1], [], [1, 0]], 2, kf_cov=[[2], [], [0, 1]])
    a = T.arrays()
    assert a["kf_mp_off"].tolist() == [0, 2, 2, 4] and a["kf_mp"].tolist() == [0, -1, 1, 0]
    assert a["pt_obs_off"].tolist() == [0, 2, 3] and a["pt_obs_kf"].tolist() == [0, 2, 2]
    assert a["kf_cov"][0].tolist() == [2] + [-1] * 9 and a["kf_cov"][2].tolist() == [0, 1] + [-1] * 8
    assert a["kf_bad"].dtype == np.uint8 and a["kf_mp"].dtype == np.int32


def test_generator_is_consistent_and_seeded():
    T = sc.random_map(3, 20, 60, 12)
    for k, row in enumerate(T.kf_mp):
        for p in row:
            assert p == -1 or k in T.pt_obs[p]
    for p, row in enumerate(T.pt_obs):
        assert row == sorted(set(row)) and all(p in T.kf_mp[k] for k in row)
    assert sc.random_map(3, 20, 60, 12).arrays()["kf_mp"].tolist() == T.arrays()["kf_mp"].tolist()
    f = sc.random_frame(1, T, 30, around=4)
    assert len(f) == 30 and any(p >= 0 for p in f)
