"""The KeyFrameDatabase model (tests/kfdb_model.py) on cases whose answer is known by
construction (tests/kfdb_cases.py).  No GPU: this proves the checker that
tests/test_gpu_kfdb.py holds the kernels against."""
import numpy as np
import pytest

import kfdb_cases as C
from kfdb_model import ModelDatabase, bow_items, l1_score, l1_terms

U = C.U


def test_l1_score_of_nonnegative_grid_values_is_the_sum_of_minima():
    rng = np.random.default_rng(5)
    for _ in range(50):
        w1 = np.sort(rng.choice(400, rng.integers(0, 120), replace=False))
        w2 = np.sort(rng.choice(400, rng.integers(0, 120), replace=False))
        v1 = rng.integers(1, 64, len(w1)) * U
        v2 = rng.integers(1, 64, len(w2)) * U
        a, b = dict(zip(w1.tolist(), v1.tolist())), dict(zip(w2.tolist(), v2.tolist()))
        expect = sum(min(a[w], b[w]) for w in a if w in b)
        assert l1_score(bow_items(a), bow_items(b)) == expect
        assert l1_score(bow_items((w1, v1)), bow_items((w2, v2))) == expect
        assert len(l1_terms(bow_items(a), bow_items(b))) == len(set(a) & set(b))


def test_l1_score_walks_in_ascending_word_order():
    # terms -8, -2^-51, -2^-51: half an ulp of 8 each.  Left to right each is lost to round-to-even;
    # right to left they first add up to a whole ulp
    c = [(0, 2.0 ** 2), (1, 2.0 ** -52), (2, 2.0 ** -52)]
    d = [(0, 2.0 ** 3), (1, 2.0 ** -51), (2, 2.0 ** -51)]
    assert l1_terms(c, d) == [-8.0, -(2.0 ** -51), -(2.0 ** -51)]
    assert l1_score(c, d) == 4.0 and l1_score(c, d, reverse=True) == 4.0 + 2.0 ** -51


@pytest.mark.parametrize("M", range(1, 41))
def test_min_common_boundary(M):
    C.case_min_common(ModelDatabase(), M)


@pytest.mark.parametrize("name", list(C.CASES))
def test_case(name):
    C.CASES[name](ModelDatabase())


def test_truncated_float_product():
    # (int)(maxCommonWords * 0.8f): a float product, truncated (in double 5 * 0.8 is 4 as well, but
    # e.g. 0.8f * 15 = 12.000000178... and 0.8 * 15 = 12 agree only after truncation)
    assert [C.min_common(m) for m in (1, 2, 4, 5, 6, 10, 15, 40)] == [0, 1, 3, 4, 4, 8, 12, 32]


def test_len_erase_clear():
    db = ModelDatabase()
    db.add(1, {0: U})
    db.add(2, {0: U})
    db.erase(7)
    db.erase(1)
    assert len(db) == 1 and db.DetectRelocalisationCandidates({0: U}) == [2]
    db.clear()
    assert len(db) == 0 and db.DetectRelocalisationCandidates({0: U}) == []
