"""Frames for the BoW tests (tests/test_gpu_bow_resident.py, tests/test_gpu_bow_trees.py): image bounds, keypoint records
around given angles, and near-duplicate descriptors."""
import numpy as np

from visual_sgraphs_amd import orb

B = (0.0, 0.0, 640.0, 480.0)


def keypoints(angle, rng):
    n = len(angle)
    k = np.zeros(n, orb.KP_DTYPE)
    k["x"], k["y"] = rng.uniform(0, 639, n), rng.uniform(0, 479, n)
    k["size"], k["response"], k["octave"] = 31.0, 1.0, rng.integers(0, 8, n)
    k["angle"] = angle
    return k


def near_dups(desc, rng, max_flips):
    """Each row with up to `max_flips` random bits flipped (some rows stay exact copies)."""
    out = desc.copy()
    rows = np.arange(len(out))
    for _ in range(max_flips):
        m = rng.random(len(out)) < 0.6
        bit = rng.integers(0, 256, len(out))
        out[rows[m], bit[m] >> 3] ^= (1 << (bit[m] & 7)).astype(np.uint8)
    return out
