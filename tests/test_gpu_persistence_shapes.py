"""The device record packer (csrc/orb_persist.hip) beyond one frame per thread.

k_record_offsets is a 1024-thread scan in which every thread owns ceil(B / 1024) frames; the
extractor-fed test in tests/test_persistence.py has B = 6.  Here B runs across 1024 and 2048
(threads that own one, two and three frames, threads that own none, a last thread that owns
fewer), with empty frames, full frames and a run of empty frames across the middle of the batch,
on synthetic records of capacity 5: offsets against numpy's cumulative sums, streams against the
host writers (which tests/test_persistence.py pins to the golden streams), every byte past the
end of the streams left as the caller filled it, and the entry point's refusals."""
import numpy as np
import pytest

import orbslam_jpminipc_amd as orb
from orbslam_jpminipc_amd import persistence as P
from orbslam_jpminipc_amd._native import ORB_EINVAL, ORB_ERANGE, ORB_OK, hip_lib, ptr

CAP = 5
FILL = 0xA5
BATCHES = [1, 2, 1023, 1024, 1025, 2048, 2049, 2500]
PATTERNS = ["random", "empty", "full_with_empty_run"]


def make_counts(B, pattern):
    if pattern == "random":
        return np.random.default_rng(B).integers(0, CAP + 1, B).astype(np.int32)
    if pattern == "empty":
        return np.zeros(B, np.int32)
    c = np.full(B, CAP, np.int32)  # every frame full, but a run of (up to) 40 empty frames across B / 2
    run = min(40, B // 2)
    c[B // 2 - run // 2: B // 2 - run // 2 + run] = 0
    return c


def make_batch(B, pattern):
    """(keypoint bytes (B, CAP, 28), descriptor bytes (B, CAP, 32), counts (B,)): random bytes in every
    slot, those past the count included."""
    rng = np.random.default_rng(1000 + B)
    return (rng.integers(0, 256, (B, CAP, 28), dtype=np.uint8), rng.integers(0, 256, (B, CAP, 32), dtype=np.uint8),
            make_counts(B, pattern))


def expected(kps, desc, counts):
    """(key offsets, descriptor offsets, keypoint stream, descriptor stream) of the batch: numpy
    cumulative sums of the record sizes, and the host writers' records one after another."""
    n = counts.astype(np.int64)
    ko = np.concatenate([[0], np.cumsum(10 + 28 * n)])
    do = np.concatenate([[0], np.cumsum(6 + 32 * n)])
    keys = b"".join(P.write_keypoint_record(kps[b, :c].reshape(-1).view(orb.KEYPOINT_DTYPE))
                    for b, c in enumerate(counts))
    des = b"".join(P.write_descriptor_record(desc[b, :c]) for b, c in enumerate(counts))
    return ko, do, keys, des


# ---- CPU: the inputs and the reference side ----------------------------------------------------
@pytest.mark.parametrize("B", [1, 2, 1025, 2500])
def test_inputs_and_reference_streams(B):
    for pattern in PATTERNS:
        kps, desc, counts = make_batch(B, pattern)
        assert counts.min() >= 0 and counts.max() <= CAP
        ko, do, keys, des = expected(kps, desc, counts)
        assert len(keys) == ko[B] and len(des) == do[B]
        recs = P.read_keypoint_stream(keys)
        assert [len(k) for k, ok in recs] == counts.tolist() and all(ok for _, ok in recs)
        drecs = P.read_descriptor_stream(des)
        assert [len(d) for d, ok in drecs] == counts.tolist() and all(ok for _, ok in drecs)
        for b in (0, B // 2, B - 1):
            assert recs[b][0].tobytes() == kps[b, :counts[b]].tobytes()
            assert drecs[b][0].tobytes() == desc[b, :counts[b]].tobytes()
            assert keys[ko[b]:ko[b] + 2] == b"\xeb\x90" and des[do[b]:do[b] + 2] == b"\xeb\x90"
    assert make_counts(B, "empty").sum() == 0
    c = make_counts(B, "full_with_empty_run")
    assert set(c.tolist()) <= {0, CAP} and (c == 0).sum() == min(40, B // 2)
    if B >= 2:
        assert c[B // 2] == 0 and c[B // 2 - 1] == (0 if B >= 4 else CAP) and c[0] == CAP
    if B == 2500:
        assert len(set(make_counts(B, "random").tolist())) == CAP + 1


# ---- GPU ------------------------------------------------------------------------------------------
def _pack(kps, desc, counts, slack=64):
    """Pack into 0xA5-filled buffers `slack` bytes longer than B full records; everything back on
    the host."""
    import torch

    B = len(counts)
    kcap, dcap = B * P.keypoint_record_bytes(CAP), B * P.descriptor_record_bytes(CAP)
    keys = torch.full((kcap + slack,), FILL, dtype=torch.uint8, device="cuda")
    des = torch.full((dcap + slack,), FILL, dtype=torch.uint8, device="cuda")
    k, d, ko, do = P.pack_keyframe_records_device(torch.from_numpy(kps).cuda(), torch.from_numpy(desc).cuda(),
                                                  torch.from_numpy(counts).cuda(), keys=keys, des=des)
    torch.cuda.synchronize()
    assert k is keys and d is des
    return keys.cpu().numpy(), des.cpu().numpy(), ko.cpu().numpy(), do.cpu().numpy()


def _check(kps, desc, counts):
    B = len(counts)
    keys, des, ko, do = _pack(kps, desc, counts)
    want_ko, want_do, want_keys, want_des = expected(kps, desc, counts)
    assert ko.shape == (B + 1,) and do.shape == (B + 1,)
    assert ko.tolist() == want_ko.tolist() and do.tolist() == want_do.tolist()
    assert keys[:ko[B]].tobytes() == want_keys
    assert des[:do[B]].tobytes() == want_des
    assert (keys[ko[B]:] == FILL).all() and (des[do[B]:] == FILL).all()  # nothing past the end of the streams


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("B", BATCHES)
def test_packer_shapes(B, pattern):
    _check(*make_batch(B, pattern))


@pytest.mark.gpu
def test_packer_refusals():
    import ctypes

    import torch

    B = 7
    kps, desc, counts = make_batch(B, "random")
    kcap, dcap = B * P.keypoint_record_bytes(CAP), B * P.descriptor_record_bytes(CAP)
    assert kcap % 2 == 0 and dcap % 2 == 0
    d_kps, d_desc, d_cnt = torch.from_numpy(kps).cuda(), torch.from_numpy(desc).cuda(), torch.from_numpy(counts).cuda()
    keys = torch.full((kcap + 2,), FILL, dtype=torch.uint8, device="cuda")
    des = torch.full((dcap + 2,), FILL, dtype=torch.uint8, device="cuda")
    ko = torch.full((B + 1,), -1, dtype=torch.int64, device="cuda")
    do = torch.full((B + 1,), -1, dtype=torch.int64, device="cuda")
    L = hip_lib()
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(n, keys_ptr, keys_cap, des_ptr, des_cap):
        return L.orb_pack_keyframe_records_device(ptr(d_kps), ptr(d_desc), ptr(d_cnt), CAP, n, keys_ptr, keys_cap,
                                                  des_ptr, des_cap, ptr(ko), ptr(do), s)

    assert call(B, ptr(keys), kcap - 1, ptr(des), dcap) == ORB_ERANGE  # one byte short of B full records
    assert call(B, ptr(keys), kcap, ptr(des), dcap - 1) == ORB_ERANGE
    odd = lambda t: ctypes.c_void_p(t.data_ptr() + 1)  # noqa: E731
    assert call(B, odd(keys), kcap, ptr(des), dcap) == ORB_EINVAL  # the body moves in 16-bit units
    assert call(B, ptr(keys), kcap, odd(des), dcap) == ORB_EINVAL
    assert call(0, ptr(keys), kcap, ptr(des), dcap) == ORB_OK  # B = 0: nothing to do
    torch.cuda.synchronize()
    for t in (keys, des):
        assert (t == FILL).all()
    assert (ko == -1).all() and (do == -1).all()
    with pytest.raises(orb.OrbError) as e:  # the wrapper reports the same refusal
        P.pack_keyframe_records_device(d_kps, d_desc, d_cnt, keys=keys[:kcap - 2], des=des)
    assert e.value.code == ORB_ERANGE
    # an exact-size call afterwards packs correctly
    assert call(B, ptr(keys), kcap, ptr(des), dcap) == ORB_OK
    torch.cuda.synchronize()
    want_ko, want_do, want_keys, want_des = expected(kps, desc, counts)
    assert ko.cpu().numpy().tolist() == want_ko.tolist() and do.cpu().numpy().tolist() == want_do.tolist()
    keys, des = keys.cpu().numpy(), des.cpu().numpy()
    assert keys[:want_ko[B]].tobytes() == want_keys and des[:want_do[B]].tobytes() == want_des
    assert (keys[want_ko[B]:] == FILL).all() and (des[want_do[B]:] == FILL).all()
