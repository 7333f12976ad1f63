"""Seeded relocalisation scenes for the MLPnP tests: a frame's undistorted keypoints with octaves 0-7 at TUM1 intrinsics, a
map-point store larger than the scene, slots with negative entries interleaved, and the minimal sets of every hypothesis.
Pixel noise is 0.5 px times the level's scale factor, 30 % of the correspondences are outliers (a keypoint anywhere in the
image).  kind: "general" (points in a volume), "plane0" (points in the world plane z = 0, THROUGH THE ORIGIN with one
coordinate exactly 0: the only scenes that reach the 9-column branch), "plane1" (the plane z = 1: off the origin, the uncentred
points3 * points3^T has full rank and the 12-column branch runs)."""
import numpy as np

F32, I32 = np.float32, np.int32
CAM = (517.306408, 516.469215, 318.643040, 255.313989)  # TUM1.yaml
NLEVELS, SCALE = 8, 1.2
LEVEL_SIGMA2 = np.array([(SCALE ** l) ** 2 for l in range(NLEVELS)], F32)
TH2 = 5.991
SEEDS = (11, 12, 13)
SIZES = (30, 100, 300)


def rot(w):
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) if th == 0 else np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)


def make(seed, n=100, kind="general", outliers=0.3, noise=0.5, n_hyp=300, capacity=None, extra=None):
    """dict(n, n_feat, kx, ky, octave, slots, world_pos (the store's contents), capacity, sets, outlier, Rcw, tcw)."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = CAM
    Rcw = rot(rng.normal(size=3) * 0.3)
    # camera-frame points in front of the camera, then to the world
    uv = np.stack([rng.uniform(20, 620, n), rng.uniform(20, 460, n)], 1)
    if kind == "general":
        z = rng.uniform(1.0, 6.0, n)
        Xc = np.stack([(uv[:, 0] - cx) / fx * z, (uv[:, 1] - cy) / fy * z, z], 1)
        tcw = rng.normal(size=3) * 0.5
        Xw = (Xc - tcw) @ Rcw  # Rcw^T (Xc - tcw)
    else:
        # a world plane z = z0 seen from a camera 3..5 m away, looking at it obliquely
        z0 = 0.0 if kind == "plane0" else 1.0
        Xw = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), np.full(n, z0)], 1)
        tcw = np.array([rng.normal() * 0.2, rng.normal() * 0.2, rng.uniform(3.0, 5.0)]) - Rcw @ np.array([0, 0, z0])
    Xw = Xw.astype(F32)
    Xc = Xw.astype(np.float64) @ Rcw.T + tcw
    octave = rng.integers(0, NLEVELS, n).astype(I32)
    px = np.stack([fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy], 1)
    px += rng.normal(size=(n, 2)) * noise * (SCALE ** octave)[:, None]
    out = rng.random(n) < outliers
    px[out] = np.stack([rng.uniform(0, 640, out.sum()), rng.uniform(0, 480, out.sum())], 1)
    # the frame: n_feat features, not a multiple of 64, the correspondences scattered among them
    n_feat = n + (n // 3 if extra is None else extra) + 7
    if n_feat % 64 == 0:
        n_feat += 1
    where = np.sort(rng.permutation(n_feat)[:n])
    kx, ky = rng.uniform(0, 640, n_feat).astype(F32), rng.uniform(0, 480, n_feat).astype(F32)
    octs = rng.integers(0, NLEVELS, n_feat).astype(I32)
    kx[where], ky[where], octs[where] = px[:, 0], px[:, 1], octave
    capacity = capacity or 2 * n + 50
    slot_of = rng.permutation(capacity)[:n].astype(I32)
    slots = np.full(n_feat, -1, I32)
    slots[where] = slot_of
    world = rng.normal(size=(capacity, 3)).astype(F32)
    world[slot_of] = Xw
    sets = np.stack([rng.permutation(n)[:6] for _ in range(n_hyp)]).astype(I32) if n >= 6 else np.zeros((n_hyp, 6), I32)
    return dict(n=n, n_feat=n_feat, kx=kx, ky=ky, octave=octs, slots=slots, world_pos=world, capacity=capacity, sets=sets,
                outlier=out, Rcw=Rcw, tcw=tcw, where=where, kind=kind)


# (n, extra): correspondences around the 256-lane stride of k_mlpnp_points and k_mlpnp_select, among n + extra + 7 features
LARGE = ((255, 40), (256, 300), (257, 100), (513, 200))


def large_scene(n, extra, kind="general"):
    """n correspondences interleaved with extra + 7 slot-less features, 5 hypotheses; (513, 200): 720 features, so that the
    clearing loop over the features and the scatter through feat[] both take three trips of 256.  Hypotheses 2 and 4 are drawn
    from true correspondences, so the returned pose has inliers at every index range.  The planar scene takes the viewpoint of
    SEEDS[1]: from some viewpoints (seed 500 + 257 is one) the 9-column branch finds no pose even from true correspondences."""
    s = make(500 + n if kind == "general" else SEEDS[1], n=n, kind=kind, n_hyp=5, extra=extra)
    # the last correspondence (the only entry of the last trip at 257 and 513): noise-free at octave 7, so that every pose
    # near the truth flags it
    w = s["where"][-1]
    Xc = s["Rcw"] @ s["world_pos"][s["slots"][w]].astype(np.float64) + s["tcw"]
    s["kx"][w], s["ky"][w], s["octave"][w] = CAM[0] * Xc[0] / Xc[2] + CAM[2], CAM[1] * Xc[1] / Xc[2] + CAM[3], NLEVELS - 1
    s["outlier"][-1] = False
    s["sets"][[2, 4]] = good_sets(s, 2, n)
    return s


def winner_last(n_hyp, seed=31, n=100):
    """(scene, sets [n_hyp x 6]): n_hyp - 1 different sets of outliers only, then one set of true correspondences."""
    s = make(seed, n=n, n_hyp=1)
    return s, np.concatenate([bad_sets(s, n_hyp - 1, seed), good_sets(s, 1, seed)])


def winner_last_min_inliers(hyp_inliers):
    """The min_inliers of winner_last from the host build's counts: the largest count of an outlier set (6 at the least, the
    smallest the call takes), which only the last hypothesis is above."""
    mi = max(6, int(np.max(hyp_inliers[:-1])))
    assert hyp_inliers[-1] > mi
    return mi


def good_sets(s, count, seed=0):
    """`count` minimal sets drawn from the scene's true correspondences only."""
    rng = np.random.default_rng(seed)
    good = np.flatnonzero(~s["outlier"])
    return np.stack([rng.permutation(good)[:6] for _ in range(count)]).astype(I32)


def bad_sets(s, count, seed=0):
    rng = np.random.default_rng(seed)
    bad = np.flatnonzero(s["outlier"])
    return np.stack([rng.permutation(bad)[:6] for _ in range(count)]).astype(I32)


def group_scene(groups, order=None):
    """Groups of groups[j] noise-free correspondences at octave 0, group j consistent with a pose of its own: hypothesis j (the
    first six of group j) counts groups[j] inliers, so hypotheses in ascending group size are all records."""
    parts = [make(900 + j, n=m, outliers=0.0, noise=0.0, n_hyp=1) for j, m in enumerate(groups)]
    s = make(899, n=sum(groups), n_hyp=1)
    at, sets = 0, []
    for p in parts:
        w = s["where"][at:at + p["n"]]
        s["kx"][w], s["ky"][w], s["octave"][w] = p["kx"][p["where"]], p["ky"][p["where"]], 0
        s["world_pos"][s["slots"][w]] = p["world_pos"][p["slots"][p["where"]]]
        sets.append(np.arange(at, at + 6))
        at += p["n"]
    s["sets"] = np.stack(sets if order is None else [sets[j] for j in order]).astype(I32)
    s["outlier"] = np.zeros(s["n"], bool)
    return s
