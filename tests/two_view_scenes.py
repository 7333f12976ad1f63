"""Seeded two-view scenes for the TwoViewReconstruction tests: two frames of undistorted keypoints, vMatches12, K and the
minimal sets.  TUM1 intrinsics; points at 3-8 m or on a plane at 5 m; 4 degrees about y, t = (-0.4, 0.05, 0.02); pixel noise;
a share of the matches replaced by uniform points of the 640 x 480 image; unmatched keypoints interleaved in both frames."""
import numpy as np

F32, I32 = np.float32, np.int32
FX, FY, CX, CY = 517.3, 516.5, 318.6, 255.3
W, H = 640, 480
SIZES = (100, 300)
# Four seeds per (planar, matches): the first four from 11 on which the REFERENCE's restatement (tests/two_view_reference.py)
# initialises from the intended model -- it legitimately refuses others (no clear winner among the motion hypotheses)
SEEDS = {(False, 100): (11, 12, 13, 14), (False, 300): (11, 12, 13, 15), (True, 100): (12, 13, 15, 17), (True, 300): (11, 12, 13, 14)}
# a general scene the reference refuses with "no clear winner" (reason 3) although its F has 221 inliers
REFUSED_GENERAL = (14, 300)


def K():
    return np.array([[FX, 0, CX], [0, FY, CY], [0, 0, 1]], F32)


def rot_y(deg):
    a = np.deg2rad(deg)
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], np.float64)


def draw_sets(n, n_iter, random_int):
    """The loop of TwoViewReconstruction.cc:82-97, transcribed: random_int(lo, hi) inclusive."""
    sets = np.zeros((n_iter, 8), I32)
    for it in range(n_iter):
        avail = list(range(n))
        for j in range(8):
            r = random_int(0, len(avail) - 1)
            sets[it, j] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    return sets


def project(X):
    return np.stack([FX * X[:, 0] / X[:, 2] + CX, FY * X[:, 1] / X[:, 2] + CY], 1)


def make(seed, n=100, planar=False, extra1=37, extra2=53, noise=0.5, outliers=0.2, deg=4.0, t=(-0.4, 0.05, 0.02), n_iter=200,
         depth=(3.0, 8.0), farthest_first=False):
    """n matches between a frame of n + extra1 and a frame of n + extra2 keypoints.  Returns dict(xy1, xy2, matches12, K,
    sets, R, t, n, n1, n2, is_outlier [n, in the order of the compacted matches]).  farthest_first: the compacted matches in
    descending order of their point's depth."""
    rng = np.random.default_rng(seed)
    R, t = rot_y(deg), np.asarray(t, np.float64)
    X = np.zeros((0, 3))
    while len(X) < n:  # points both cameras see
        u = rng.uniform([20, 20], [W - 20, H - 20], (4 * n, 2))
        z = np.full(4 * n, 5.0) if planar else rng.uniform(depth[0], depth[1], 4 * n)
        if planar:  # a plane through (0, 0, 5), tilted a little: z = 5 + 0.1 x
            z = 5.0 / (1.0 - 0.1 * (u[:, 0] - CX) / FX)
        P = np.stack([(u[:, 0] - CX) / FX * z, (u[:, 1] - CY) / FY * z, z], 1)
        P2 = P @ R.T + t
        p2 = project(P2)
        ok = (P2[:, 2] > 0.1) & (p2[:, 0] > 0) & (p2[:, 0] < W) & (p2[:, 1] > 0) & (p2[:, 1] < H)
        X = np.concatenate([X, P[ok]])
    X = X[:n]
    if farthest_first:
        X = X[np.argsort(-X[:, 2], kind="stable")]
    p1 = project(X) + rng.normal(0, noise, (n, 2)) if noise else project(X)
    p2 = project(X @ R.T + t) + (rng.normal(0, noise, (n, 2)) if noise else 0)
    is_out = np.zeros(n, bool)
    n_out = int(round(outliers * n))
    if n_out:
        idx = rng.choice(n, n_out, replace=False)
        is_out[idx] = True
        p2[idx] = rng.uniform([0, 0], [W, H], (n_out, 2))
    n1, n2 = n + extra1, n + extra2
    xy1, xy2 = rng.uniform([0, 0], [W, H], (n1, 2)), rng.uniform([0, 0], [W, H], (n2, 2))
    slot1, slot2 = np.sort(rng.choice(n1, n, replace=False)), rng.permutation(n2)[:n]
    xy1[slot1], xy2[slot2] = p1, p2
    m12 = np.full(n1, -1, I32)
    m12[slot1] = slot2
    sets = draw_sets(n, n_iter, lambda lo, hi: int(rng.integers(lo, hi + 1)))
    return dict(xy1=xy1.astype(F32), xy2=xy2.astype(F32), matches12=m12, K=K(), sets=sets, R=R, t=t, n=n, n1=n1, n2=n2,
                is_outlier=is_out, seed=seed)


def issue_scene(seed, n, planar):
    return make(seed * 10 + (1 if planar else 0) + n, n=n, planar=planar)


def issue_scenes():
    """The sixteen scenes of the issue: general and planar, 100 and 300 matches, four seeds each."""
    return [(planar, n, seed, issue_scene(seed, n, planar)) for planar in (False, True) for n in SIZES for seed in SEEDS[(planar, n)]]


TILE = 1024               # kTvTile of csrc/vsg_two_view.hip: the rank count of k_tv_check_rt goes through LDS tiles of this size
TILE_SIZES = (1023, 1024, 1025, 2049)


def tile_scene(n):
    """A general scene of n matches around the tile, 10 % outliers, 16 sets.  0.25 px of noise: with so few sets the best
    eight-point F of a 0.5 px scene often passes too few matches through CheckRT for the routine to initialise, and the
    rank count is at work only where more than 51 matches are counted."""
    return make(700 + n, n=n, outliers=0.1, noise=0.25, n_iter=16, extra1=21, extra2=34)


def rank_holder_late():
    """1500 noise-free matches, the farthest point first: the small cosines (the near points) sit at the highest indices, so
    the candidate trips of the rank count go past index 1024 before one holds rank 50."""
    return make(731, n=1500, outliers=0.0, noise=0.0, n_iter=12, extra1=21, extra2=34, farthest_first=True)


def tie_base():
    return make(741, n=1100, outliers=0.0, noise=0.0, n_iter=12, extra1=21, extra2=34)


def tie_across_the_tile(a, b):
    """tie_base() in which the match b takes the keypoints of the match a in both frames (one keypoint twice in each frame)
    and the matches are permuted so that the two sit at the compacted indices 1023 and 1024.  The caller chooses a (the
    match whose cosine holds rank 50) and b (one of a larger cosine) on tie_base() with the host build."""
    base = tie_base()
    s = dict(base, xy1=base["xy1"].copy(), xy2=base["xy2"].copy(), matches12=base["matches12"].copy())
    i1 = np.nonzero(s["matches12"] >= 0)[0]
    i2 = s["matches12"][i1]
    s["xy1"][i1[b]], s["xy2"][i2[b]] = s["xy1"][i1[a]], s["xy2"][i2[a]]
    order = [k for k in range(len(i1)) if k not in (a, b)]
    order[TILE - 1:TILE - 1] = [a, b]
    s["xy1"][i1], s["matches12"][i1] = s["xy1"][i1[order]], i2[order]
    return s


def winner_last(n_iter=1024, seed=751):
    """100 matches; n_iter - 1 copies of one set of outlier matches, then one set of true matches: the last hypothesis wins."""
    s = make(seed, n=100, n_iter=1)
    rng = np.random.default_rng(seed)
    bad, good = np.flatnonzero(s["is_outlier"]), np.flatnonzero(~s["is_outlier"])
    s["sets"] = np.concatenate([np.tile(rng.choice(bad, 8, replace=False), (n_iter - 1, 1)), rng.choice(good, 8, replace=False)[None]]).astype(I32)
    return s


def pure_rotation(seed, n=120):
    return make(seed, n=n, outliers=0.0, noise=0.0, t=(0.0, 0.0, 0.0), deg=5.0)


def tiny_baseline(seed, n=120):
    """A 1 mm baseline before points 8 to 14 cm away: parallax between 0.4 and 0.7 degrees, so the cosines stay below 0.99998
    (the depth gates work and one motion hypothesis wins) and the routine ends at the parallax gate."""
    return make(seed, n=n, outliers=0.0, noise=0.0, t=(-0.001, 0.0, 0.0), deg=0.0, depth=(0.08, 0.14))


def nan_hypothesis_scene(seed=51, n=200):
    """A good general scene whose set 0 samples eight matches that all sit on one pixel in both frames: that hypothesis's
    matrices are not finite, so its score is NaN and must never win."""
    s = make(seed, n=n, outliers=0.1, n_iter=24)
    i1 = np.nonzero(s["matches12"] >= 0)[0][:8]
    s["xy1"][i1], s["xy2"][s["matches12"][i1]] = (100.0, 120.0), (100.0, 120.0)
    s["sets"][0] = np.arange(8)
    return s


def identical_keypoints(n=40):
    """Every keypoint of both frames at one place: every score is zero."""
    s = make(5, n=n, extra1=0, extra2=0, outliers=0.0)
    s["xy1"][:], s["xy2"][:] = (300.0, 200.0), (300.0, 200.0)
    return s
