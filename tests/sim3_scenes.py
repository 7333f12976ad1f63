"""Seeded scenes for the Sim3Solver tests: two keyframes in two maps, correspondences between their map points related by a
known similarity, noise and gross outliers, octaves, thresholds and the RANSAC samples.  Every scene is a dict:
kf1 / kf2 (Rcw, tcw, fx, fy, cx, cy), Xw1 / Xw2 (n x 3 float32 world positions), oct1 / oct2, max_err1 / max_err2 (as the
comparison sees them), samples (n_hyp x 3 int32), truth (R12, t12, s12)."""
import functools

import numpy as np

import sim3_reference as sr

F32, F64, I32 = np.float32, np.float64, np.int32
SIGMA2 = sr.level_sigma2()


def rot(axis, deg):
    a = np.asarray(axis, F64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.deg2rad(deg)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K


def camera(rng, fx=458.0, fy=457.0, cx=367.0, cy=248.0):
    R = rot(rng.normal(size=3), rng.uniform(0, 40))
    return dict(Rcw=R.astype(F32), tcw=rng.uniform(-1, 1, 3).astype(F32), fx=fx, fy=fy, cx=cx, cy=cy)


def to_world(kf, Xc):
    """Xw with Rcw Xw + tcw = Xc, in double, rounded once."""
    return ((np.asarray(Xc, F64) - kf["tcw"].astype(F64)) @ kf["Rcw"].astype(F64)).astype(F32)


def frustum_points(rng, n, zmin=2.0, zmax=8.0):
    z = rng.uniform(zmin, zmax, n)
    return np.stack([rng.uniform(-0.6, 0.6, n) * z, rng.uniform(-0.4, 0.4, n) * z, z], 1)


def draw(rng, n, n_hyp):
    return sr.draw_samples(n, n_hyp, lambda lo, hi: int(rng.integers(lo, hi + 1)))


def make(seed, n=60, outliers=0.3, noise=0.01, scale=1.3, deg=20.0, n_hyp=300, same_kf=False):
    rng = np.random.default_rng(seed)
    kf1 = camera(rng)
    kf2 = kf1 if same_kf else camera(rng, 460.0, 459.0, 365.0, 250.0)
    R12, t12 = rot(rng.normal(size=3), deg), rng.uniform(-0.3, 0.3, 3)
    X2 = frustum_points(rng, n)
    X1 = scale * X2 @ R12.T + t12 + rng.normal(scale=noise, size=(n, 3))
    bad = rng.permutation(n)[:int(round(outliers * n))]
    X1[bad] = frustum_points(rng, len(bad), 2.0 * scale, 8.0 * scale)
    oct1, oct2 = rng.integers(0, 8, n).astype(I32), rng.integers(0, 8, n).astype(I32)
    return dict(kf1=kf1, kf2=kf2, Xw1=to_world(kf1, X1), Xw2=to_world(kf2, X2), oct1=oct1, oct2=oct2, n=n,
                max_err1=sr.max_err(SIGMA2[oct1]), max_err2=sr.max_err(SIGMA2[oct2]), samples=draw(rng, n, n_hyp) if n >= 3 else
                np.zeros((n_hyp, 3), I32), outlier=np.isin(np.arange(n), bad), truth=dict(R12=R12, t12=t12, s12=scale))


@functools.lru_cache(maxsize=None)
def issue_scene(seed):
    """The scene of the per-hypothesis comparison: 60 correspondences, 30 % gross outliers, 1 cm noise, scale 1.3, rotation
    20 degrees, octaves 0..7, 300 hypotheses."""
    return make(seed)


SEEDS = (11, 12, 13, 14)


LARGE_SIZES = (255, 256, 257, 513)  # around the 256-lane stride of k_sim3_points and k_sim3_select, and two strides + 1


@functools.lru_cache(maxsize=None)
def large_scene(n):
    """n correspondences with 9 hypotheses: more than one workgroup of k_sim3_points, more than one trip of k_sim3_select.
    Scale 1, so that the hypotheses of fix_scale have inliers too; triples 4 and 8 are drawn from true correspondences and the
    last correspondence (the only entry of the last trip at 257 and 513) is a noise-free one of octave 7, which every
    hypothesis near the truth flags: a flag is set in every trip."""
    s = make(400 + n, n=n, n_hyp=9, scale=1.0)
    tr, k1, k2 = s["truth"], s["kf1"], s["kf2"]
    X2 = k2["Rcw"].astype(F64) @ s["Xw2"][-1].astype(F64) + k2["tcw"].astype(F64)
    s["Xw1"][-1] = to_world(k1, (tr["s12"] * tr["R12"] @ X2 + tr["t12"])[None])[0]
    s["oct1"][-1] = s["oct2"][-1] = 7
    s["max_err1"], s["max_err2"] = sr.max_err(SIGMA2[s["oct1"]]), sr.max_err(SIGMA2[s["oct2"]])
    s["outlier"][-1] = False
    good = np.flatnonzero(~s["outlier"])
    rng = np.random.default_rng(n)
    s["samples"][4], s["samples"][8] = rng.choice(good, 3, replace=False), rng.choice(good, 3, replace=False)
    return s


def winner_last(n_hyp, seed=21):
    """(scene, samples [n_hyp x 3]) at n = 60: n_hyp - 1 different triples that each hold a gross outlier, then one all-inlier
    triple.  With min_inliers = the largest count among the former only the last triple can be above it."""
    s = make(seed, n_hyp=1)
    rng = np.random.default_rng(seed + 1000)
    good, bad = np.flatnonzero(~s["outlier"]), np.flatnonzero(s["outlier"])
    sm = np.zeros((n_hyp, 3), I32)
    for k in range(n_hyp - 1):
        sm[k] = [bad[k % len(bad)], *rng.choice(good, 2, replace=False)]
        sm[k] = sm[k][rng.permutation(3)]
    sm[-1] = good[:3]
    return s, sm


def winner_last_min_inliers(hyp_inliers):
    """The min_inliers of winner_last from the host build's counts: the largest count of a triple with an outlier."""
    mi = int(np.max(hyp_inliers[:-1]))
    assert hyp_inliers[-1] > mi  # the all-inlier triple is the only one above it
    return mi


def identical_triple(s):
    """Correspondences 0..2 get the SAME camera coordinates on both sides (M symmetric, N block diagonal, the eigenvector
    exactly (1, 0, 0, 0)): hypothesis (0, 1, 2) has a zero imaginary part."""
    s = dict(s, Xw1=s["Xw1"].copy(), Xw2=s["Xw2"].copy(), kf2=s["kf1"])
    s["Xw2"][:3] = s["Xw1"][:3]
    return s


def collinear_triple(s):
    """Correspondences 0..2 lie on one line in both maps: N has a double largest eigenvalue."""
    s = dict(s, Xw1=s["Xw1"].copy(), Xw2=s["Xw2"].copy())
    for X in (s["Xw1"], s["Xw2"]):
        X[1] = X[0] + F32(0.25) * (X[2] - X[0])
    return s
