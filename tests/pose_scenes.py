"""Seeded scenes for the pose-optimisation tests (tests/test_pose_*.py, tests/test_gpu_pose_optimization.py): a random
pose, points in front of a TUM1-like camera (bf = 40), observations with UNIFORM noise within +-0.8 sigma of the
keypoint's level per axis (so an inlier's chi2 stays under 3 * 0.64 = 1.92, far from 5.991 / 7.815), outliers displaced
by at least 20 px.  Sizes are the smallest at which the kernel can go wrong: the return-0 paths (0, 2 edges), the `< 10`
break (3, 9, 10), the wavefront edge (63, 64, 65), the workgroup stride (255, 256, 257), a frame of 1000 features with
300 slots scattered among -1s; all-mono, all-stereo and mixed; 0 % and 30 % outliers.  Directed scenes follow, each with
a condition that tests/test_pose_reference.py asserts on the restatement alone.

Every scene must keep every compared chi2 more than 1e-3 (relative) away from its threshold, under 8 random
permutations of the edge order too (test_pose_reference.py::test_fixture_condition): then no feature needs excluding
from any flag comparison.

SPREAD / TOL below are MEASURED, not chosen: the largest deviation of the restatement from itself over those 8
permutations, per quantity, over all scenes, and 64 times that (the permutations sample summation order only; the
header's own sin / cos and up to 40 chained updates add a few ulp each).  Produced by
    python tests/pose_scenes.py --measure
"""
import functools
import math
import sys

import numpy as np

import pose_reference as pr

F32, I32 = np.float32, np.int32
NLEVELS = 8
SIGMA2 = (F32(1.2) ** np.arange(NLEVELS, dtype=F32)) ** 2
INV_SIGMA2 = (F32(1.0) / SIGMA2).astype(F32)
TUM1 = (517.306408, 516.469215, 318.643040, 255.313989, 40.0)
DYADIC = (512.0, 512.0, 320.0, 256.0, 32.0)  # a camera whose projections of dyadic points are exact
N_PERM = 8

# measured (see the module docstring): largest |difference| between edge orders, and 64 x that.  q and t are measured
# values.  chi2_rel is NOT: the measured spread of the chi2 floats is below one float ulp (they come out identical under
# every order but for rounding-boundary cases), so the constant is the FLOOR 2^-23 = one ulp of the compared float, a
# chosen number reasoned from the format, and the tolerance is 64 float ulps.
SPREAD = dict(q=1.0380585280245214e-13, t=7.557288128623441e-13, chi2_rel=1.1920928955078125e-07)
TOL = {k: 64 * v for k, v in SPREAD.items()}


def _rot(axis_angle):
    return pr.q_to_matrix(pr.se3_exp(np.concatenate([axis_angle, np.zeros(3)]))[0])


def make(seed, n_feat, n_slots, kind="mixed", outliers=0.0, start=(0.02, 1.0), noise=0.8, cam=TUM1, truth=None,
         capacity=None):
    """-> scene dict.  start = (metres, degrees) the start pose is off the truth by; kind: mono | stereo | mixed."""
    rng = np.random.default_rng(seed)
    if truth is None:
        R = _rot(rng.normal(0, 0.3, 3))
        t = rng.normal(0, 1.0, 3)
    else:
        R, t = truth
    fx, fy, cx, cy, bf = [float(F32(c)) for c in cam]
    capacity = capacity or max(n_slots + 7, 16)
    z = rng.uniform(1.0, 8.0, n_feat)
    u, v = rng.uniform(20, 620, n_feat), rng.uniform(20, 460, n_feat)
    Xc = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1)
    Xw = ((Xc - t) @ R).astype(F32)  # R^T (Xc - t)
    Xc = Xw.astype(np.float64) @ R.T + t
    octave = rng.integers(0, NLEVELS, n_feat).astype(I32)
    sig = np.sqrt(SIGMA2.astype(np.float64))[octave]
    pu = fx * Xc[:, 0] / Xc[:, 2] + cx
    pv = fy * Xc[:, 1] / Xc[:, 2] + cy
    pr_ = pu - bf / Xc[:, 2]
    nz = rng.uniform(-noise, noise, (n_feat, 3)) * sig[:, None]
    feat_slots = np.full(n_feat, -1, I32)
    with_slot = np.sort(rng.choice(n_feat, n_slots, replace=False)) if n_slots else np.zeros(0, np.int64)
    feat_slots[with_slot] = rng.permutation(capacity)[:n_slots].astype(I32)
    is_out = np.zeros(n_feat, bool)
    if outliers > 0 and n_slots:
        is_out[rng.choice(with_slot, int(round(outliers * n_slots)), replace=False)] = True
    ang, mag = rng.uniform(0, 2 * math.pi, n_feat), rng.uniform(20, 60, n_feat)
    du, dv = np.where(is_out, mag * np.cos(ang), 0.0), np.where(is_out, mag * np.sin(ang), 0.0)
    kx, ky = (pu + nz[:, 0] + du).astype(F32), (pv + nz[:, 1] + dv).astype(F32)
    stereo = {"mono": np.zeros(n_feat, bool), "stereo": np.ones(n_feat, bool), "mixed": rng.random(n_feat) < 0.5}[kind]
    u_right = np.where(stereo, pr_ + nz[:, 2] + du, -1.0).astype(F32)
    world_pos = rng.normal(0, 5, (capacity, 3)).astype(F32)
    world_pos[feat_slots[with_slot]] = Xw[with_slot]
    d = rng.normal(0, 1, 3)
    a = rng.normal(0, 1, 3)
    dR = _rot(a / np.linalg.norm(a) * math.radians(start[1]))
    Rs, ts = dR @ R, dR @ t + d / np.linalg.norm(d) * start[0]
    return dict(n=n_feat, feat_slots=feat_slots, capacity=capacity, world_pos=world_pos, kx=kx, ky=ky, octave=octave,
                u_right=None if kind == "mono" else u_right, q=pr.q_from_matrix(Rs).astype(F32), t=ts.astype(F32),
                cam=tuple(F32(c) for c in cam), inv_sigma2=INV_SIGMA2, nlevels=NLEVELS, truth=(R, t), is_out=is_out,
                removed=None)


def _with_pose(s, q, t):
    s = dict(s)
    s["q"], s["t"] = np.asarray(q, F32), np.asarray(t, F32)
    return s


def _dyadic(z0_feature=False):
    """Identity pose, a camera and points whose projections are exact: every error is exactly 0 at the start."""
    rng = np.random.default_rng(11)
    n = 24
    z = rng.choice([2.0, 4.0], n)
    X = np.stack([rng.integers(-8, 9, n) / 8.0, rng.integers(-6, 7, n) / 8.0, z], 1)
    fx, fy, cx, cy, bf = DYADIC
    s = make(11, n, n, "mixed", cam=DYADIC, capacity=32)
    slots = s["feat_slots"]
    s["world_pos"][slots] = X.astype(F32)
    s["kx"], s["ky"] = (fx * X[:, 0] / z + cx).astype(F32), (fy * X[:, 1] / z + cy).astype(F32)
    st = s["u_right"] >= 0
    s["u_right"] = np.where(st, fx * X[:, 0] / z + cx - bf / z, -1.0).astype(F32)
    s["q"], s["t"] = np.array([0, 0, 0, 1], F32), np.zeros(3, F32)
    s["truth"], s["is_out"] = (np.eye(3), np.zeros(3)), np.zeros(n, bool)
    if z0_feature:
        s["world_pos"][slots[5]] = (0.5, 0.25, 0.0)  # camera-frame z == 0 at the input pose
    return s


def _stale_errors(n_pairs=50, n_exact=150):
    """A FINITE scene in which the stale-error rule decides compared floats.  Identity pose, exact projections.  Each of
    n_pairs points is observed twice, at +2 px and -2 px (chi2 = 4 each: inliers whose gradients cancel exactly); n_exact
    observations are exact; ONE of them is moved by one float step.  The gradient is ~1e-5, the first step ~1e-10 and
    accepted; the second step gains less than half an ulp of the cost (~400), so tempChi == currentChi, rho == 0: the
    trial is REJECTED and the round Terminates with the errors of the rejected state.  For the exact observations the
    error at the estimate and at the rejected state differ by far more than a float ulp of their (tiny) chi2."""
    rng = np.random.default_rng(31)
    n = 2 * n_pairs + n_exact
    fx, fy, cx, cy, bf = DYADIC
    s = make(31, n, n, "mono", cam=DYADIC, capacity=n + 8)
    X = np.stack([rng.integers(-8, 9, n) / 8.0, rng.integers(-6, 7, n) / 8.0, rng.choice([2.0, 4.0], n)], 1)
    X[1:2 * n_pairs:2] = X[0:2 * n_pairs:2]
    s["world_pos"][s["feat_slots"]] = X.astype(F32)
    kx, ky = fx * X[:, 0] / X[:, 2] + cx, fy * X[:, 1] / X[:, 2] + cy
    kx[0:2 * n_pairs:2] += 2.0
    kx[1:2 * n_pairs:2] -= 2.0
    s["octave"] = np.zeros(n, I32)
    s["octave"][-1] = 7
    kx = kx.astype(F32)
    kx[-1] = np.nextafter(kx[-1], F32(1e9))
    s["kx"], s["ky"], s["u_right"] = kx, ky.astype(F32), None
    s["q"], s["t"] = np.array([0, 0, 0, 1], F32), np.zeros(3, F32)
    s["truth"], s["is_out"] = (np.eye(3), np.zeros(3)), np.zeros(n, bool)
    return s


def stale_features(ref):
    """Of the last round of a result: {feature: (compared stale float, float at the estimate)} where the two differ and
    both are finite."""
    log = ref["log"][-1]
    return {f: (c, log["fresh"][f]) for f, c, _ in log["compared"]
            if f in log["fresh"] and np.isfinite(c) and np.isfinite(log["fresh"][f]) and c != log["fresh"][f]}


def follows_stale_rule(ref, chi2):
    """Does chi2 (per feature) carry the STALE values of ref where stale and fresh differ?  An implementation that
    recomputed the errors at the estimate during classification lands on the fresh ones."""
    st = stale_features(ref)
    return len(st), sum(1 for f, (c, fr) in st.items() if abs(float(chi2[f]) - float(c)) < abs(float(chi2[f]) - float(fr)))


def _planted():
    """Noise-free inliers at the true pose plus eight features planted at 0.8x and 1.25x of their threshold."""
    s = make(21, 72, 72, "mixed", noise=0.0, start=(0.0, 0.0))
    st = s["u_right"] >= 0
    mono, ster = np.flatnonzero(~st)[:4], np.flatnonzero(st)[:4]
    s["planted"] = {}
    for idx, th in ((mono, 5.991), (ster, 7.815)):
        for i, f in zip(idx, (0.8, 1.25, 0.8, 1.25)):
            d = math.sqrt(f * th * float(SIGMA2[s["octave"][i]]))
            if i in idx[:2]:
                s["kx"][i] += F32(d)
            else:
                s["ky"][i] -= F32(d)
            s["planted"][int(i)] = f
    return s


@functools.lru_cache(maxsize=None)
def scenes():
    """name -> scene, in a fixed order."""
    out = {}
    for e in (0, 2, 3, 9, 10):
        out["edges_%d" % e] = make(100 + e, e + 5, e, "mixed")
    for e in (63, 64, 65, 255, 256, 257):
        out["edges_%d" % e] = make(100 + e, e + 9, e, "mixed", outliers=0.3)
    for kind in ("mono", "stereo"):
        out["%s_clean" % kind] = make(201, 70, 65, kind)
        out["%s_outliers" % kind] = make(202, 70, 65, kind, outliers=0.3)
    out["mixed_clean"] = make(203, 70, 65, "mixed")
    out["frame_1000_300"] = make(204, 1000, 300, "mixed", outliers=0.3, capacity=4096)
    out["far_start"] = make(301, 120, 100, "mixed", outliers=0.1, start=(0.3, 15.0))
    # a start at the optimum of an earlier run (rounded to float): every step gains less than 0.1 % of the cost, so every
    # optimize() ends by _nBad >= 3 after an accepted trial
    base = make(302, 90, 80, "mixed")
    r = reference(base)
    out["converged_start"] = _with_pose(base, r["q"], r["t"])
    out["exact_start"] = _dyadic()
    out["stale_errors"] = _stale_errors()
    out["planted"] = _planted()
    out["z_zero"] = _dyadic(z0_feature=True)
    rem = make(303, 140, 120, "mixed", outliers=0.2)
    removed = np.zeros(rem["n"], np.uint8)
    removed[np.flatnonzero(rem["feat_slots"] >= 0)[::7]] = 1
    removed[np.flatnonzero(rem["feat_slots"] < 0)[:3]] = 1  # a feature without a map point: nothing to remove
    rem["removed"] = removed
    out["plane_step"] = rem
    few = make(304, 20, 12, "mixed")  # 12 edges, 4 removed in round 2: 8 < 10 ends the loop there
    removed = np.zeros(few["n"], np.uint8)
    removed[np.flatnonzero(few["feat_slots"] >= 0)[:4]] = 1
    few["removed"] = removed
    out["plane_step_ends_loop"] = few
    return out


def reference(s, order=None, hold=None):
    """The restatement's result for a scene; a scene with a removed set is run with the hold."""
    hold = (s["removed"] is not None) if hold is None else hold
    kps = np.stack([s["kx"], s["ky"]], 1)
    return pr.pose_optimization(s["feat_slots"], s["world_pos"], kps, s["octave"], s["u_right"], s["q"], s["t"], s["cam"],
                                s["inv_sigma2"], 2 if hold else -1, s["removed"] if hold else None, order)


@functools.lru_cache(maxsize=None)
def references():
    """name -> the restatement's result in feature order, computed once for all tests."""
    return {name: reference(s) for name, s in scenes().items()}


@functools.lru_cache(maxsize=None)
def permuted_references():
    """name -> the restatement's results under N_PERM random edge orders."""
    out = {}
    for k, (name, s) in enumerate(scenes().items()):
        rng = np.random.default_rng(900 + k)
        E = int((s["feat_slots"] >= 0).sum())
        out[name] = [reference(s, rng.permutation(E)) for _ in range(N_PERM)]
    return out


def deviations(a, b):
    """Largest differences between two results that agree on the flags: q, t absolute, chi2 relative."""
    dq = float(np.nanmax(np.abs(a["q"] - b["q"]), initial=0.0))
    dt = float(np.nanmax(np.abs(a["t"] - b["t"]), initial=0.0))
    dc = 0.0
    for f, c in a["chi2"].items():
        c2 = b["chi2"][f]
        if np.isfinite(c) and np.isfinite(c2) and max(abs(c), abs(c2)) > 0:
            dc = max(dc, abs(float(c) - float(c2)) / max(abs(float(c)), abs(float(c2)), 1e-6))
    return dict(q=dq, t=dt, chi2_rel=dc)


def measure():
    spread = dict(q=0.0, t=0.0, chi2_rel=0.0)
    for name, ref in references().items():
        for p in permuted_references()[name]:
            for k, v in deviations(ref, p).items():
                spread[k] = max(spread[k], v)
    return spread


if __name__ == "__main__" and "--measure" in sys.argv:
    sp = measure()
    # never below one rounding of the quantity itself: unit-size doubles for q / t, one float ulp for the chi2 floats
    sp = dict(q=max(sp["q"], 2.0 ** -52), t=max(sp["t"], 2.0 ** -52), chi2_rel=max(sp["chi2_rel"], 2.0 ** -23))
    print("SPREAD = dict(q=%r, t=%r, chi2_rel=%r)" % (sp["q"], sp["t"], sp["chi2_rel"]))
