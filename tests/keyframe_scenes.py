"""Scenes for the tests of Fuse x2 and SearchByProjection(pKF, Scw, ...) on resident map points
(tests/test_keyframe_projection_reference.py, tests/test_gpu_keyframe_points.py): tests/projection_scenes.py's map points made
from the target KeyFrame's own keypoints, so that a real share of them fuses, plus points that leave the loop at every
reject branch, plus points whose best candidate lies beyond TH_LOW."""
import numpy as np

import projection_scenes as ps
from visual_sgraphs_amd import orb

F32 = np.float32
# bounds with fractions on both sides, as Frame::ComputeImageBounds leaves them for a distorted camera: the KeyFrame's
# `const int` copies are (-26, -22, 671, 510)
FRACTIONAL_BOUNDS = (-26.6, -22.4, 671.3, 510.8)


def synthetic_keypoints(seed, n=900, w=640, h=480):
    """Keypoints and descriptors of no image: what the CPU tests put in a real extraction's place."""
    rng = np.random.default_rng(5000 + seed)
    kps = np.zeros(n, orb.KP_DTYPE)
    kps["x"], kps["y"] = rng.uniform(1, w - 1, n), rng.uniform(1, h - 1, n)
    kps["octave"] = rng.integers(0, 8, n)
    kps["angle"] = rng.uniform(0, 360, n)
    kps["size"] = 31.0 * F32(1.2) ** kps["octave"]
    return kps, rng.integers(0, 256, (n, 32), dtype=np.uint8)


def keyframe_map(kps, desc, ur, pose, seed, n_other=300, far=0.1, mirror=False):
    """ps.map_points (every keypoint un-projected once, normals along the viewing ray, the keypoint's descriptor with up to
    20 bits flipped; n_other points of tests/frustum_reference.py's scenario behind the camera, outside the image, outside
    the band and seen from the side), with 90 more bits flipped on a share `far` of the keypoints' points: their best
    candidate is beyond TH_LOW.  mirror: the keypoints' points lie BEHIND the camera.  Returns (fields, src)."""
    fields, src = ps.map_points(kps, desc, ur, pose, seed, mirror=mirror, n_other=n_other)
    rng = np.random.default_rng(9000 + seed)
    for i in np.flatnonzero((src >= 0) & (rng.random(len(src)) < far)):
        bits = rng.choice(256, 90, replace=False)
        np.bitwise_xor.at(fields["desc"][i], bits // 8, (1 << (bits % 8)).astype(np.uint8))
    return fields, src
