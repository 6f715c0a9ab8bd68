"""The overlapped front-end pipeline (csrc/orb_pipeline.hip) equals the serial path:
extract_batch_device + search_for_initialization_batch_device on one stream, bit for bit.

Further down, one pipeline is reused across steps of different density and batch size and every step
is compared with the CPU oracle (extraction per frame, SearchForInitialization per consecutive pair),
on the default stream, on a caller stream with a single synchronisation, and with a camera."""
import numpy as np
import pytest

import orbslam_jpminipc_amd as orb
from orbslam_jpminipc_amd.pipeline import FrontEndPipeline

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B,S", [(9, 4), (3, 8), (8, 1), (17, 3)])
def test_pipeline_equals_serial_path(B, S):
    import torch

    W, H = 640, 480
    frames = torch.from_numpy(orb.synth_stream(W, H, stream=60 + B, first=0, count=B)).cuda()
    pipe = FrontEndPipeline(1000, 1.2, 8, 1, 20, device=0, max_batch=B, n_streams=S)
    cap = pipe.max_keypoints
    k = torch.zeros((B, cap, 28), dtype=torch.uint8, device="cuda")
    d = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
    c = torch.zeros((B,), dtype=torch.int32, device="cuda")
    m12 = torch.full((max(B - 1, 1), cap), -7, dtype=torch.int32, device="cuda")
    nm = torch.full((max(B - 1, 1),), -7, dtype=torch.int32, device="cuda")
    pipe.run(frames, k, d, c, m12, nm)
    torch.cuda.synchronize()
    ext = orb.ORBextractor(1000, 1.2, 8, orb.FAST_SCORE, 20, device=0, max_batch=B)
    k2, d2, c2 = ext.extract_batch_device(frames)
    f1 = torch.arange(0, B - 1, dtype=torch.int32, device="cuda")
    m2, n2 = orb.ORBmatcher(0.9, True).search_for_initialization_batch_device(k2, d2, c2, f1, f1 + 1, W, H, 100)
    torch.cuda.synchronize()
    assert torch.equal(c, c2)
    for b in range(B):
        n = int(c[b])
        assert torch.equal(k[b, :n], k2[b, :n]) and torch.equal(d[b, :n], d2[b, :n])
    assert torch.equal(nm[:B - 1], n2)
    for p in range(B - 1):
        n = int(c[p])
        assert torch.equal(m12[p, :n], m2[p, :n])


# ---- one pipeline reused across steps, every step against the oracle --------------------------
# The frames are the ladder of tests/call_history.py (323 x 243, 1000 features, 4 levels).  A class has
# eight frames, so the ninth frame of a batch of nine is the class's frame 0 again.
import call_history as C  # noqa: E402
from oracle_lib import compute_image_bounds, search_for_initialization, undistort_keypoints  # noqa: E402

MB, FILL, MFILL = 9, 0xA5, -7
MIXED9 = [("flat", 0), ("noise", 1), ("lowtex", 2), ("stream", 3), ("flat", 4), ("noise", 5), ("lowtex", 6),
          ("stream", 7), ("flat", 0)]
_pairs = {}


def _nine(cls):
    return C.batch(cls) + [(cls, 0)]


def _expected_frame(item, cam):
    ko, do = C.expected(*item)
    return (ko if cam is None else undistort_keypoints(ko, *cam)), do


def _expected_pair(a, b, cam):
    """The oracle's SearchForInitialization(a, b), window 100, ratio 0.9 (on mvKeysUn inside the camera's
    bounds when there is a camera), computed once."""
    key = (a, b, cam)
    if key not in _pairs:
        (k1, d1), (k2, d2) = _expected_frame(a, cam), _expected_frame(b, cam)
        prev = np.ascontiguousarray(np.stack([k1["x"], k1["y"]], 1).astype(np.float32)).reshape(-1, 2)
        bounds = None if cam is None else compute_image_bounds(C.W, C.H, *cam)
        _pairs[key] = search_for_initialization(k1, d1, k2, d2, C.W, C.H, prev, 0.9, True, 100, bounds=bounds)
    return _pairs[key]


class _Outputs:
    """Output tensors for nine frames and eight pairs, prefilled: rows 0xA5, counts 0, matches -7."""

    def __init__(self, cap, undistorted=False):
        import torch

        self.k = torch.full((MB, cap, 28), FILL, dtype=torch.uint8, device="cuda")
        self.kun = torch.full((MB, cap, 28), FILL, dtype=torch.uint8, device="cuda") if undistorted else None
        self.d = torch.full((MB, cap, 32), FILL, dtype=torch.uint8, device="cuda")
        self.c = torch.zeros((MB,), dtype=torch.int32, device="cuda")
        self.m12 = torch.full((MB - 1, cap), MFILL, dtype=torch.int32, device="cuda")
        self.nm = torch.full((MB - 1,), MFILL, dtype=torch.int32, device="cuda")

    def tensors(self):
        return [t for t in (self.k, self.kun, self.d, self.c, self.m12, self.nm) if t is not None]


def _check_step(step, items, host, cam=None):
    """host: the output tensors as numpy arrays, in _Outputs.tensors() order."""
    if cam is None:
        k, d, c, m12, nm = host
        kun = None
    else:
        k, kun, d, c, m12, nm = host
    B = len(items)
    for b, item in enumerate(items):
        ko, do = C.expected(*item)
        n = int(c[b])
        assert n == len(ko), f"{step}, frame {b} {item}: {n} keypoints, oracle {len(ko)}"
        assert k[b, :n].tobytes() == ko.tobytes(), f"{step}, frame {b} {item}: keypoints differ"
        assert d[b, :n].tobytes() == do.tobytes(), f"{step}, frame {b} {item}: descriptors differ"
        if kun is not None:
            assert kun[b, :n].tobytes() == _expected_frame(item, cam)[0].tobytes(), f"{step}, frame {b}: mvKeysUn differ"
    for p in range(B - 1):
        no, m12o = _expected_pair(items[p], items[p + 1], cam)
        assert nm[p] == no, f"{step}, pair {p} {items[p]} {items[p + 1]}: {nm[p]} matches, oracle {no}"
        assert np.array_equal(m12[p, :c[p]], m12o), f"{step}, pair {p} {items[p]} {items[p + 1]}: matches differ"
        if "flat" in (items[p][0], items[p + 1][0]):
            assert no == 0 and (m12o == -1).all()
    assert (c[B:] == 0).all() and (k[B:] == FILL).all() and (d[B:] == FILL).all(), f"{step}: frames past the batch written"
    assert kun is None or (kun[B:] == FILL).all(), f"{step}: mvKeysUn past the batch written"
    assert (nm[max(B - 1, 0):] == MFILL).all() and (m12[max(B - 1, 0):] == MFILL).all(), f"{step}: pairs past the batch written"


STEPS = [("1 B = 9 noise", _nine("noise")), ("2 B = 9 lowtex", _nine("lowtex")),
         ("3 B = 5", [("stream", 0), ("stream", 1), ("lowtex", 3), ("noise", 2), ("noise", 3)]),
         ("4 B = 2", [("lowtex", 4), ("lowtex", 5)]), ("5 B = 1", [("stream", 2)]), ("6 B = 9 mixed", MIXED9)]


def test_one_pipeline_across_batch_sizes_equals_the_oracle():
    """max_batch 9 on 4 streams (chunk handles of 3 frames): dense, sparse, then fewer frames than chunks
    can fill, fewer frames than streams, one frame without match buffers, and a mixed batch whose flat
    frames sit at both ends and in the middle.  A chunk handle that a smaller step leaves out keeps the
    state of the step before."""
    import torch

    pipe = FrontEndPipeline(C.NF, C.SCALE, C.NLEVELS, orb.FAST_SCORE, C.TH, device=0, max_batch=MB, n_streams=4)
    assert pipe.n_streams == 4
    for step, items in STEPS:
        B = len(items)
        o = _Outputs(pipe.max_keypoints)
        frames = torch.from_numpy(C.images(items)).cuda()
        pipe.run(frames, o.k, o.d, o.c, o.m12 if B > 1 else None, o.nm if B > 1 else None)
        torch.cuda.synchronize()
        _check_step(step, items, [t.cpu().numpy() for t in o.tensors()])
    pipe.close()


def test_pipeline_is_ordered_after_the_callers_earlier_work():
    """The header's promise, "after earlier work on the caller's stream and before later work on it", on
    one non-default caller stream: the device input still holds the noise frames of the step before, the
    lowtex frames are copied over them from pinned memory without blocking, run(stream=caller) follows,
    the outputs are copied to pinned memory on the caller stream, and the stream is synchronised once.
    Chunk streams that did not wait for the copy would usually extract noise frames; a match that did not
    wait for the chunks, or a download that did not wait for the match, would read the prefill.

    This can only catch such a race when it happens, it cannot prove there is none: a missing wait may
    still lose the race to the copy and pass."""
    import torch

    pipe = FrontEndPipeline(C.NF, C.SCALE, C.NLEVELS, orb.FAST_SCORE, C.TH, device=0, max_batch=MB, n_streams=4)
    noise, lowtex = _nine("noise"), _nine("lowtex")
    pinned_in = torch.from_numpy(C.images(lowtex)).pin_memory()
    d_in = torch.from_numpy(C.images(noise)).cuda()
    first, second = _Outputs(pipe.max_keypoints), _Outputs(pipe.max_keypoints)
    pinned_out = [torch.empty(t.shape, dtype=t.dtype).pin_memory() for t in second.tensors()]
    torch.cuda.synchronize()
    caller = torch.cuda.Stream()
    with torch.cuda.stream(caller):
        pipe.run(d_in, first.k, first.d, first.c, first.m12, first.nm, stream=caller)
        d_in.copy_(pinned_in, non_blocking=True)
        pipe.run(d_in, second.k, second.d, second.c, second.m12, second.nm, stream=caller)
        for dst, src in zip(pinned_out, second.tensors()):
            dst.copy_(src, non_blocking=True)
    caller.synchronize()
    _check_step("lowtex after noise, one synchronisation", lowtex, [t.numpy() for t in pinned_out])
    torch.cuda.synchronize()
    _check_step("the noise step before it", noise, [t.cpu().numpy() for t in first.tensors()])
    pipe.close()


def test_one_undistorting_pipeline_across_batch_sizes():
    """run_undistorted with the strong pincushion camera of test_gpu_undistort.py, B = 9 then B = 4 on one
    pipeline: mvKeysUn and the matches inside the camera's bounds against the oracle."""
    import torch
    from test_gpu_undistort import CAMS

    cam = CAMS[4]
    pipe = FrontEndPipeline(C.NF, C.SCALE, C.NLEVELS, orb.FAST_SCORE, C.TH, device=0, max_batch=MB, n_streams=4)
    for step, items in [("1 B = 9 noise, undistorted", _nine("noise")), ("2 B = 4 mixed, undistorted", MIXED9[:4])]:
        o = _Outputs(pipe.max_keypoints, undistorted=True)
        frames = torch.from_numpy(C.images(items)).cuda()
        pipe.run_undistorted(frames, cam[0], cam[1], o.k, o.kun, o.d, o.c, o.m12, o.nm)
        torch.cuda.synchronize()
        _check_step(step, items, [t.cpu().numpy() for t in o.tensors()], cam)
    pipe.close()
