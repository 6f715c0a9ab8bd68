"""TEST INFRASTRUCTURE: synthetic [B][cap] keypoint batches for k_undistort (csrc/orb_frame.hip)
off the extractor's shapes: capacities that are no multiple of the kernel's 256-thread block,
counts of 0, 1, cap - 1 and cap, coordinates outside the image and on exact half-integers, and a
sentinel record in every slot past the count.  tests/test_undistort_oracle.py checks on the CPU
that the batches are what they claim; tests/test_gpu_undistort.py runs the kernel on them."""
import numpy as np

from oracle_lib import KEYPOINT_DTYPE

W, H = 640, 480
IN_SENTINEL = 0xC3  # every byte of an input slot past the frame's count
OUT_SENTINEL = 0x3C  # every byte of the output buffer before the call

# (B, cap, counts): the counts mix 0, 1, cap - 1 and cap over the cases of one capacity
CASES = [
    (1, 1, [1]),
    (1, 1, [0]),
    (3, 255, [255, 0, 254]),
    (3, 255, [1, 255, 0]),
    (3, 257, [1, 257, 256]),
    (3, 257, [257, 0, 1]),
    (2, 1000, [999, 1000]),
    (2, 1000, [0, 1]),
]


def make_batch(B, cap, counts, seed=0):
    """(B, cap) KEYPOINT_DTYPE records.  Below the count: x in [-300, W + 300), y in [-300, H + 300),
    every third point snapped to half-integers, the other five fields random; from the count on:
    IN_SENTINEL bytes."""
    rng = np.random.default_rng(seed + 7 * B + cap)
    k = np.zeros((B, cap), KEYPOINT_DTYPE)
    k["x"] = rng.uniform(-300, W + 300, (B, cap))
    k["y"] = rng.uniform(-300, H + 300, (B, cap))
    snap = (np.arange(B * cap).reshape(B, cap) % 3) == 0
    k["x"][snap] = np.floor(k["x"][snap]) + 0.5
    k["y"][snap] = np.floor(k["y"][snap]) + 0.5
    k["size"] = 31.0 * 1.2 ** rng.integers(0, 8, (B, cap))
    k["angle"] = rng.uniform(0, 360, (B, cap))
    k["response"] = rng.integers(7, 200, (B, cap))
    k["octave"] = rng.integers(0, 8, (B, cap))
    k["class_id"] = rng.integers(-1, 1000, (B, cap))
    raw = k.view(np.uint8).reshape(B, cap, 28)
    for b, n in enumerate(counts):
        raw[b, n:] = IN_SENTINEL
    return k
