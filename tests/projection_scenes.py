"""Scenes for the GPU tests of the motion-model and relocalisation projection searches (tests/test_gpu_search_last_frame.py,
tests/test_gpu_search_keyframe_points.py): map points made from a current frame's own keypoints, so that a real share of
them matches, and a last frame / KeyFrame that observes them."""
import numpy as np

import frustum_reference as fr
from visual_sgraphs_amd import orb

F32 = np.float32
FIELDS = ("world_pos", "normal", "min_dist", "max_dist", "desc", "observed")
CAM = fr.CAMERAS["tum1"]
MB = CAM[6] / CAM[2]  # Frame::mb = mbf / fx


def current_pose(seed):
    return fr.scenario(seed, "tum1", n=1)[0]


def map_points(kps, desc, ur, pose, seed, per_keypoint=1, mirror=False, n_other=0):
    """Every keypoint un-projected `per_keypoint` times at a random depth through the pose, with pixel jitter and up to 20
    flipped descriptor bits; with mvuRight, 80 % of the depths agree with it.  mfMaxDistance puts the predicted level at the
    keypoint's octave or one above.  mirror: the points lie BEHIND the camera and project to the same pixels.
    n_other points of tests/frustum_reference.py's scenario follow (behind the camera, outside the image, outside the band).
    Returns (fields, src) with src[i] = the keypoint point i was made from, -1 for the scenario's."""
    rng = np.random.default_rng(seed)
    k = np.tile(kps, per_keypoint)
    src = np.tile(np.arange(len(kps)), per_keypoint)
    n = len(k)
    R, t = pose["Rcw"].astype(np.float64), pose["tcw"].astype(np.float64)
    z = rng.uniform(1.0, 8.0, n)
    if ur is not None:
        u_r = ur[src]
        ok = (u_r > 0) & (rng.random(n) < 0.8)
        z[ok] = pose["mbf"] / (k["x"][ok].astype(np.float64) - u_r[ok])
        z = np.where(np.isfinite(z) & (z > 0.1), z, 3.0)
    x = (k["x"].astype(np.float64) + rng.normal(0, 0.7, n) - pose["cx"]) / pose["fx"] * z
    y = (k["y"].astype(np.float64) + rng.normal(0, 0.7, n) - pose["cy"]) / pose["fy"] * z
    Pc = np.stack([x, y, z], 1)
    if mirror:
        Pc = -Pc
    Pw = ((Pc - t) @ R).astype(F32)  # R^T (Pc - t)
    PO = Pw.astype(np.float64) - pose["Ow"]
    dist = np.linalg.norm(PO, axis=1)
    Nn = (PO / dist[:, None]).astype(F32)
    lvl = k["octave"].astype(np.float64) + rng.integers(0, 2, n)
    mf_max = (dist * 1.2 ** (lvl - 0.5)).astype(F32)
    mf_min = (mf_max / F32(1.2) ** F32(7)).astype(F32)
    d = desc[src].copy()
    for i in range(n):  # up to 20 flipped bits
        bits = rng.integers(0, 256, rng.integers(0, 21))
        d[i, bits // 8] ^= (1 << (bits % 8)).astype(np.uint8)
    fields = dict(world_pos=Pw, normal=Nn, min_dist=mf_min, max_dist=mf_max, desc=d,
                  observed=(rng.random(n) < 0.8).astype(np.uint8))
    if n_other:
        other = fr.scenario(seed, "tum1", n=n_other)[2]
        fields = {key: np.concatenate([fields[key], other[key]]) for key in FIELDS}
        src = np.concatenate([src, np.full(n_other, -1)])
    return fields, src


def observer_angles(kps, src, rng):
    """The current keypoint's angle plus small noise; about 15 % random, so that the three-maxima filter removes something."""
    a = kps["angle"][src].astype(np.float64) + rng.normal(0, 3.0, len(src))
    rnd = rng.random(len(src)) < 0.15
    a[rnd] = rng.uniform(0, 360, int(rnd.sum()))
    return np.mod(a, 360.0).astype(F32)


def last_pose_of(pose, along_axis, seed):
    """A last pose whose camera sees the current camera centre at (0, 0, along_axis): tlc = dR (Rcw Ow + tcw) + (0, 0, d)."""
    rng = np.random.default_rng(seed)
    dR = fr.rotation(rng, 0.02).astype(np.float64)
    R = dR @ pose["Rcw"].astype(np.float64)
    t = dR @ pose["tcw"].astype(np.float64) + np.array([0.0, 0.0, along_axis])
    return fr.make_pose(R, t, pose["fx"], pose["fy"], pose["cx"], pose["cy"], pose["mbf"])


def last_frame_arrays(kps, fields, src, last_pose, bounds, seed, extra=0.25, outliers=0.10, capacity=None):
    """(last_kps, last_desc, last_slots, store_slots): the points projected through the last pose (clipped to the image: the
    search never reads a last-frame position) plus `extra` features with no map point, shuffled; octaves = the current
    keypoint's +-1; about `outliers` of the slots are -1.  store_slots[j] = where point j lives in a store of `capacity`
    (a permutation with gaps when capacity exceeds the points)."""
    rng = np.random.default_rng(seed)
    n = len(src)
    ne = int(extra * n)
    P = fields["world_pos"].astype(np.float64)
    Pc = P @ last_pose["Rcw"].astype(np.float64).T + last_pose["tcw"].astype(np.float64)
    with np.errstate(all="ignore"):
        u = last_pose["fx"] * Pc[:, 0] / Pc[:, 2] + last_pose["cx"]
        v = last_pose["fy"] * Pc[:, 1] / Pc[:, 2] + last_pose["cy"]
    lk = np.zeros(n + ne, orb.KP_DTYPE)
    lk["x"][:n] = np.clip(np.nan_to_num(u, nan=1.0), bounds[0] + 1, bounds[2] - 1)
    lk["y"][:n] = np.clip(np.nan_to_num(v, nan=1.0), bounds[1] + 1, bounds[3] - 1)
    lk["x"][n:], lk["y"][n:] = rng.uniform(bounds[0] + 1, bounds[2] - 1, ne), rng.uniform(bounds[1] + 1, bounds[3] - 1, ne)
    lk["octave"][:n] = np.clip(kps["octave"][src] + rng.integers(-1, 2, n), 0, 7)
    lk["angle"][:n] = observer_angles(kps, src, rng)
    free = np.concatenate([src < 0, np.ones(ne, bool)])  # observers of scenario points, features without a map point
    lk["octave"][free], lk["angle"][free] = rng.integers(0, 8, int(free.sum())), rng.uniform(0, 360, int(free.sum()))
    lk["size"] = 31.0 * F32(1.2) ** lk["octave"]
    cap = capacity or n
    # its own generator: the placement does not change which features are outliers or how they are shuffled
    store_slots = (np.random.default_rng(seed + 7777).permutation(cap)[:n] if capacity else np.arange(n)).astype(np.int32)
    slots = np.full(n + ne, -1, np.int32)
    slots[:n] = store_slots
    slots[:n][rng.random(n) < outliers] = -1  # mvbOutlier
    order = rng.permutation(n + ne)
    lk, slots = lk[order], slots[order]
    ldesc = rng.integers(0, 256, (n + ne, 32), dtype=np.uint8)  # the last frame's own descriptors are never read
    return lk, ldesc, slots, store_slots


def last_frame(kps, fields, src, last_pose, bounds, seed, extra=0.25, outliers=0.10, capacity=None):
    """last_frame_arrays uploaded: (Frame, last_kps, last_slots, store_slots)."""
    lk, ldesc, slots, store_slots = last_frame_arrays(kps, fields, src, last_pose, bounds, seed, extra, outliers, capacity)
    L = orb.Frame(len(lk) + 1)
    L.upload(lk, ldesc, bounds)
    return L, lk, slots, store_slots


def store_of(fields, store_slots, capacity=None):
    mp = orb.MapPoints(capacity or len(store_slots))
    mp.update(store_slots, **{k: fields[k] for k in FIELDS})
    return mp


def per_slot(fields, store_slots, capacity=None):
    """The fields indexed by SLOT (what a reference indexed through the slot list reads)."""
    cap = capacity or len(store_slots)
    out = {}
    for k in FIELDS:
        a = np.zeros((cap,) + fields[k].shape[1:], fields[k].dtype)
        a[store_slots] = fields[k]
        out[k] = a
    return out
