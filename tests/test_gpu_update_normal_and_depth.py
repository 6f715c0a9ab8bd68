"""orb_update_normal_and_depth / _device (csrc/orb_mappoint.hip) against the CPU model of
MapPoint::UpdateNormalAndDepth (tests/local_mapping_model.py): bit for bit, NaN as "is NaN"."""
import numpy as np
import pytest

import local_mapping_model as model
import local_mapping_scenes as scenes
from orbslam_jpminipc_amd import mappoint
from orbslam_jpminipc_amd._native import ORB_EINVAL, ORB_ENOTSUP, OrbError

pytestmark = pytest.mark.gpu

f32 = np.float32
SF = scenes.SF[:scenes.NLEVELS]


def points(seed, sizes, levels=None):
    rng = np.random.default_rng(seed)
    M = len(sizes)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    pos = (rng.uniform(-3, 3, (M, 3)) + [0, 0, 6]).astype(f32)
    ow = rng.uniform(-1, 1, (int(off[-1]), 3)).astype(f32)
    ref = rng.uniform(-1, 1, (M, 3)).astype(f32)
    lev = rng.integers(0, scenes.NLEVELS, M).astype(np.int32) if levels is None else np.asarray(levels, np.int32)
    return off, ow, pos, ref, lev


def same(got, want):
    for g, w, name in zip(got, want, ("normal", "dmin", "dmax")):
        assert model.same_bits(g, w), name


def test_observation_counts_and_levels():
    """0, 1, 2, 31 and 4000 observations; the reference level at both ends of the table and outside it
    (clamped).  No observation: a NaN normal, the depths still set."""
    args = points(1, [0, 1, 2, 31, 4000, 5, 5], [3, 0, scenes.NLEVELS - 1, 2, 5, -4, 99])
    got = mappoint.update_normal_and_depth(*args, SF)
    same(got, model.update_normal_and_depth(*args, SF))
    assert np.isnan(got[0][0]).all() and not np.isnan(got[0][1:]).any() and (got[1] > 0).all() and (got[2] > got[1]).all()
    assert np.abs(np.linalg.norm(got[0][1], axis=-1) - 1) < 1e-6  # one observation: a unit vector
    clamped = points(1, [0, 1, 2, 31, 4000, 5, 5], [3, 0, scenes.NLEVELS - 1, 2, 5, 0, scenes.NLEVELS - 1])
    same(got, model.update_normal_and_depth(*clamped, SF))


@pytest.mark.parametrize("M", [1, 63, 64, 65])
def test_point_counts(M):
    rng = np.random.default_rng(M)
    args = points(M, rng.integers(0, 9, M))
    same(mappoint.update_normal_and_depth(*args, SF), model.update_normal_and_depth(*args, SF))


def test_the_sum_depends_on_the_observation_order():
    """The caller's order is part of the input: reversing 31 observations changes the float sum."""
    off, ow, pos, ref, lev = points(3, [31] * 20)
    rev = ow.reshape(20, 31, 3)[:, ::-1].reshape(-1, 3).copy()
    a = mappoint.update_normal_and_depth(off, ow, pos, ref, lev, SF)
    b = mappoint.update_normal_and_depth(off, rev, pos, ref, lev, SF)
    same(b, model.update_normal_and_depth(off, rev, pos, ref, lev, SF))
    assert (a[0] != b[0]).any() and np.abs(a[0] - b[0]).max() < 1e-6


def test_device_form():
    import torch

    off, ow, pos, ref, lev = points(4, [0, 3, 17, 1, 64])
    d = [torch.from_numpy(x).cuda() for x in (off, ow, pos, ref, lev)]
    n, lo, hi = (torch.zeros((5, 3), dtype=torch.float32).cuda(), torch.zeros(5, dtype=torch.float32).cuda(),
                 torch.zeros(5, dtype=torch.float32).cuda())
    mappoint.update_normal_and_depth_device(*d, SF, 64, n, lo, hi)
    torch.cuda.synchronize()
    same([x.cpu().numpy() for x in (n, lo, hi)], model.update_normal_and_depth(off, ow, pos, ref, lev, SF))


def test_limits():
    args = points(5, [4001])
    with pytest.raises(OrbError) as e:
        mappoint.update_normal_and_depth(*args, SF)
    assert e.value.code == ORB_ENOTSUP
    args = points(5, [3])
    with pytest.raises(OrbError) as e:
        mappoint.update_normal_and_depth(*args, SF[:1])
    assert e.value.code == ORB_ENOTSUP
    with pytest.raises(OrbError) as e:
        mappoint.update_normal_and_depth(np.array([1, 3], np.int32), *args[1:], SF)
    assert e.value.code == ORB_EINVAL
