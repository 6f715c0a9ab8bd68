"""One ORBextractor handle driven through a history of calls, every call bit for bit against the oracle.

The product is a long-lived handle over a changing video; the handle keeps cell counters, candidate
lists, per-level tables, a self-resetting completion counter and Harris scratch between calls
("State that outlives a call").  Each sequence here makes stale state from real earlier
calls on the ladder of tests/call_history.py: a dense call, then a sparser one, an empty one, a
smaller batch, another entry point, another frame size, another pyramid builder.  A reset that is
missing on one path then shows as a wrong count or a keypoint of the earlier, denser frame.

After every step, for every frame b of the step: counts[b], kps[b, :n] and desc[b, :n] are the
oracle's bytes (rows at and past n are not part of the ABI and not asserted); for a step of fewer
than 8 frames, counts[B:] and every row of the frames >= B still hold the prefill (0xA5 rows, zero
counts).  A failure names the step, the frame, the first level whose cell counts differ and the
first differing keypoint.
"""
import ctypes

import numpy as np
import pytest

import call_history as C
import orbslam_jpminipc_amd as orb

pytestmark = pytest.mark.gpu

MB = 8
SCORES = pytest.mark.parametrize("score", [orb.FAST_SCORE, orb.HARRIS_SCORE], ids=["fast", "harris"])
FILL = 0xA5
_dev = {}


def _device_images(items, w=C.W, h=C.H):
    """The frames of a step on the device, uploaded once."""
    import torch

    key = (tuple(items), w, h)
    if key not in _dev:
        _dev[key] = torch.from_numpy(C.images(items, w, h)).cuda()
    return _dev[key]


class Handle:
    """One extractor handle and the checks of a step."""

    def __init__(self, score):
        self.score = score
        self.ext = orb.ORBextractor(C.NF, C.SCALE, C.NLEVELS, score, C.TH, device=0, max_batch=MB)
        self.cap = self.ext.max_keypoints
        self.lib = orb.hip_lib()

    def outputs(self):
        """Output tensors for 8 frames: rows 0xA5, counts 0."""
        import torch

        k = torch.full((MB, self.cap, 28), FILL, dtype=torch.uint8, device="cuda")
        d = torch.full((MB, self.cap, 32), FILL, dtype=torch.uint8, device="cuda")
        c = torch.zeros((MB,), dtype=torch.int32, device="cuda")
        return k, d, c

    def device_step(self, step, items, w=C.W, h=C.H, stream=None):
        """extract_batch_device of the items into fresh prefilled outputs, synchronised and checked."""
        import torch

        out = self.outputs()
        self.ext.extract_batch_device(_device_images(items, w, h), *out, stream=stream)
        torch.cuda.synchronize()
        self.check(step, items, out, w, h)

    def check(self, step, items, out, w=C.W, h=C.H, live=True):
        """`live`: the step is the handle's last launch, so its cell counters can be read back."""
        k, d, c = (t.cpu().numpy() for t in out)
        B = len(items)
        for b, (cls, i) in enumerate(items):
            ko, do = C.expected(cls, i, self.score, w, h)
            n = int(c[b])
            if not 0 <= n <= self.cap:
                pytest.fail(f"{step}, frame {b} ({cls} {i}): count {n} outside [0, {self.cap}], oracle {len(ko)}")
            self.same(step, b, (cls, i), orb.keypoints_from_bytes(k[b], n), d[b, :n], ko, do, w, h, live)
        assert (c[B:] == 0).all(), f"{step}: counts of the frames past the batch of {B} were written: {c.tolist()}"
        assert (k[B:] == FILL).all() and (d[B:] == FILL).all(), f"{step}: rows of the frames past the batch were written"

    def same(self, step, b, item, kg, dg, ko, do, w=C.W, h=C.H, live=True):
        cls, i = item
        head = f"{step}, frame {b} ({cls} {i}, {w} x {h}, {'FAST' if self.score == orb.FAST_SCORE else 'HARRIS'}_SCORE)"
        m = min(len(kg), len(ko))
        raw = [np.ascontiguousarray(x[:m]).view(np.uint8).reshape(m, 28) for x in (kg, ko)]
        bad = np.nonzero((raw[0] != raw[1]).any(axis=1))[0]
        if len(kg) != len(ko) or len(bad):
            lines = [f"{head}: gpu {len(kg)} keypoints, oracle {len(ko)}"]
            if live:
                lines.append(self.first_level(b, item, w, h))
            if len(bad):
                j = int(bad[0])
                fields = [f for f in kg.dtype.names if kg[j][f].tobytes() != ko[j][f].tobytes()]
                lines.append(f"first differing keypoint {j} (fields {fields}):\n  gpu    {kg[j]}\n  oracle {ko[j]}")
            elif len(kg) != len(ko):
                longer, who = (kg, "gpu") if len(kg) > len(ko) else (ko, "oracle")
                lines.append(f"first extra keypoint ({who}): {longer[m]}")
            pytest.fail("\n".join(lines))
        if m == 0:
            return
        rows = np.nonzero((np.asarray(dg) != do).any(axis=1))[0]
        if len(rows):
            pytest.fail(f"{head}: descriptors differ in {len(rows)} of {m} rows, first {rows[:5].tolist()}: {ko[rows[0]]}")

    def first_level(self, b, item, w, h):
        """The first level whose per-cell corner counts differ from the oracle's (test_gpu_parity._diagnose)."""
        for l in range(C.NLEVELS):
            cnt = np.zeros(4096, np.int32)
            n = self.lib.orb_debug_cell_counts(self.ext._h, b, l, cnt.ctypes.data_as(ctypes.c_void_p), 4096)
            oc = C.cell_counts(*item, w, h)[l].reshape(-1)
            if n != oc.size or not np.array_equal(cnt[:n], oc):
                return f"level {l} cell counts differ: gpu {cnt[:max(n, 0)].tolist()} oracle {oc.tolist()}"
        return "cell counts equal at every level"

    def host_step(self, step, item, w=C.W, h=C.H):
        """The single-image host call."""
        kg, dg = self.ext(C.frame(*item, w, h))
        ko, do = C.expected(*item, self.score, w, h)
        assert (dg is None) == (len(kg) == 0)
        self.same(step, 0, item, kg, dg if dg is not None else np.zeros((0, 32), np.uint8), ko, do, w, h)

    def host_batch_step(self, step, items, w=C.W, h=C.H):
        outs = self.ext.extract_batch(C.images(items, w, h))
        for b, item in enumerate(items):
            kg, dg = outs[b]
            ko, do = C.expected(*item, self.score, w, h)
            self.same(step, b, item, kg, dg if dg is not None else np.zeros((0, 32), np.uint8), ko, do, w, h)

    def pyramid_path(self, mode):
        assert self.lib.orb_debug_set_pyramid_path(self.ext._h, mode) == 0

    def corner_list(self, cap):
        assert self.lib.orb_debug_set_fast_corner_list(self.ext._h, cap) == 0


@SCORES
def test_content_sequence(score):
    """noise -> stream -> lowtex -> flat -> mixed -> noise, 8 frames each: every cell counter, candidate
    list and level table falls from over its quota to a few entries to none, then rises again, and in
    the mixed step each frame slot holds another class than in the steps around it."""
    h = Handle(score)
    for step, items in [("1 noise x 8", C.batch("noise")), ("2 stream x 8", C.batch("stream")),
                        ("3 lowtex x 8", C.batch("lowtex")), ("4 flat x 8", C.batch("flat")), ("5 mixed", C.MIXED),
                        ("6 noise x 8", C.batch("noise"))]:
        h.device_step(step, items)


@SCORES
def test_batch_size_and_entry_point_sequence(score):
    """A full dense device batch, then smaller batches and the host entry points (which stage through the
    handle's own buffers and stream), then a full batch again: slots 3 .. 7 keep the dense call's state
    while slots 0 .. 2 are rewritten, and the frames past a batch are not touched."""
    h = Handle(score)
    h.device_step("1 noise x 8 (device batch)", C.batch("noise"))
    h.device_step("2 B = 3 (lowtex, flat, stream)", [("lowtex", 0), ("flat", 0), ("stream", 0)])
    h.device_step("3 B = 1 flat", [("flat", 1)])
    h.host_step("4 host call, lowtex", ("lowtex", 1))
    h.host_batch_step("5 host batch, stream x 8", C.batch("stream"))
    h.device_step("6 B = 8 mixed", C.MIXED)


@SCORES
def test_geometry_sequence(score):
    """Frame sizes alternate on one handle: every change rebuilds the plan and all buffers, and the
    return to 323 x 243 must not meet anything of the first visit."""
    h = Handle(score)
    h.device_step("1 323 x 243 noise", C.batch("noise"))
    h.device_step("2 161 x 121 lowtex", C.batch("lowtex"), 161, 121)
    h.device_step("3 323 x 243 lowtex", C.batch("lowtex"))
    h.device_step("4 96 x 57 stream", C.batch("stream"), 96, 57)
    h.device_step("5 323 x 243 flat", C.batch("flat"))
    h.device_step("6 323 x 243 noise", C.batch("noise"))


@SCORES
def test_pyramid_path_sequence(score):
    """The per-level builders (mode 1: the cell counters are zeroed by a memset) and k_pyr_stream (mode 2:
    it zeroes them on its way) alternate between dense and sparse steps, so each of the two has to
    clear what a dense call under the other one left."""
    h = Handle(score)
    steps = [(1, "noise"), (2, "lowtex"), (1, "noise"), (2, "flat"), (2, "noise"), (1, "lowtex"), (1, "flat"),
             (0, "noise")]
    for n, (mode, cls) in enumerate(steps):
        h.pyramid_path(mode)
        h.device_step(f"{n + 1} pyramid path {mode}, {cls} x 8", C.batch(cls))
        assert h.lib.orb_debug_pyramid_plan(h.ext._h, None, None, None) == 1, "323 x 243 has no k_pyr_stream plan"


@SCORES
@pytest.mark.parametrize("mode", [2, 1], ids=["streaming", "per-level"])
def test_phase_split_after_a_dense_call(score, mode):
    """A dense whole call, then a sparse call as set_phases(1) and set_phases(2): the phase-2-only launch
    zeroes the cell counters itself, whichever builder ran in phase 1 (k_pyr_stream leaves them alone when
    detection does not follow in the same launch)."""
    import torch

    h = Handle(score)
    h.pyramid_path(mode)
    for n, (dense, sparse) in enumerate([(C.batch("noise"), C.batch("lowtex")), (C.MIXED, C.batch("flat")),
                                         (C.batch("noise"), [("lowtex", 3), ("flat", 3), ("stream", 3)])]):
        h.device_step(f"{2 * n + 1} whole call, dense", dense)
        out = h.outputs()
        h.ext.set_phases(1)
        h.ext.extract_batch_device(_device_images(sparse), *out)
        h.ext.set_phases(2)
        try:
            h.ext.extract_batch_device(_device_images(sparse), *out)
        finally:
            h.ext.set_phases(3)
        torch.cuda.synchronize()
        h.check(f"{2 * n + 2} phases 1 then 2, sparse", sparse, out)


@SCORES
def test_corner_list_sequence(score):
    """k_fast's corner list at 256, 8 and 256 entries across noise -> lowtex -> noise: with 8 entries every
    wave of the noise frame and some of the lowtex frame go through the plane-scan fallback."""
    h = Handle(score)
    for n, (cap, cls) in enumerate([(256, "noise"), (8, "lowtex"), (256, "noise"), (8, "noise"), (256, "lowtex"),
                                    (8, "flat")]):
        h.corner_list(cap)
        h.device_step(f"{n + 1} corner list {cap}, {cls} x 8", C.batch(cls))


@SCORES
def test_back_to_back_without_host_synchronisation(score):
    """noise, lowtex, flat and mixed enqueued back to back on one non-default stream into four output
    sets, one synchronisation at the end: the benchmark's usage.  The self-resetting completion counter and
    the cell counters are reset on the device, in stream order, with no host in between."""
    import torch

    h = Handle(score)
    steps = [("1 noise x 8", C.batch("noise")), ("2 lowtex x 8", C.batch("lowtex")), ("3 flat x 8", C.batch("flat")),
             ("4 mixed", C.MIXED)]
    imgs = [_device_images(items) for _, items in steps]
    outs = [h.outputs() for _ in steps]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    for d_imgs, out in zip(imgs, outs):
        h.ext.extract_batch_device(d_imgs, *out, stream=s)
    s.synchronize()
    for n, ((step, items), out) in enumerate(zip(steps, outs)):
        h.check(step + " (no synchronisation between the steps)", items, out, live=n == len(steps) - 1)
