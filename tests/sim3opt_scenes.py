"""Seeded scenes for the Sim3-optimisation tests (tests/test_sim3opt_*.py, tests/test_gpu_sim3_optimization.py): two
keyframes with TUM1-like cameras, two stores, pairs of map points related by a true Sim3 S12 (X1c = S12 X2c), observations
with UNIFORM noise within +-0.8 sigma of the keypoint's level per axis (so an inlier's chi2 stays under 2 * 0.64 = 1.28 at
the truth, far from th2 = 10), outliers displaced by at least 6 sigma of their level (chi2 >= 36).  Sizes are the smallest
at which the kernel can go wrong: no pair, one, the `< 10` return on either side (9, 10, 11), the wavefront edge (63, 64,
65), the workgroup stride (255, 256, 257), each with a few features without a match in between; one keyframe-sized scene
(1000 features, 300 pairs, stores of 4096 slots); 0 % and 30 % outliers, fix_scale 0 / 1, true scale 1 / 1.3, all_points
0 / 1 with a third of idx2 < 0, two stores and one shared store.  Directed scenes follow, each with a condition that
tests/test_sim3opt_reference.py asserts on the restatement alone.

Every scene must keep every compared chi2 more than 1e-3 (relative) away from th2 under every member of the perturbation
set (test_sim3opt_reference.py::test_fixture_condition): then no pair needs excluding from any flag comparison.

SPREAD / TOL below are MEASURED, not chosen: the largest deviation of the restatement from itself, per quantity, over all
scenes, over a perturbation set of N_PERT = 8 members -- each a random pair order (summation order), every sin / cos / exp
result moved by a seeded random 0 or +-1 ulp, and numpy.linalg.solve in place of the unpivoted LDL^T in every second
member -- and TOL = 16 x SPREAD (a maximum over 8 draws underestimates the tail), floored at one rounding of the quantity.
The figures are far wider than pose_scenes.TOL: the 1e-9 central differences amplify last-bit differences of the errors
by 1 / 2e-9.  chi2 deviations are relative to max(|chi2|, 1): a chi2 matters against th2 = 10 only, and a noise-free
pair's chi2 of 1e-12 has no meaningful relative error.  Produced by
    python tests/sim3opt_scenes.py --measure
"""
import functools
import math
import sys

import numpy as np

import sim3opt_reference as sr

F32, I32, U8 = np.float32, np.int32, np.uint8
NLEVELS = 8
SIGMA2 = (F32(1.2) ** np.arange(NLEVELS, dtype=F32)) ** 2
INV_SIGMA2 = (F32(1.0) / SIGMA2).astype(F32)
TUM1 = (517.306408, 516.469215, 318.643040, 255.313989)
DYADIC = (512.0, 512.0, 320.0, 256.0)  # a camera whose projections of dyadic points are exact
TH2 = 10.0                               # LoopClosing.cc:538, :747
N_PERT = 8

# measured (see the module docstring): SPREAD, and TOL = 16 x SPREAD
SPREAD = dict(q=4.510560883130843e-10, t=1.1146005896023325e-08, s=1.463340939651837e-07, chi2_rel=3.2109795672363717e-06)
TOL = {k: 16 * v for k, v in SPREAD.items()}


def _rot(axis_angle):
    return sr.q_rotate(sr.sim3_exp(np.concatenate([axis_angle, np.zeros(4)]))[0], np.eye(3)).T


def _pose(R, t, cam):
    return dict(Rcw=np.asarray(R, F32).reshape(9), tcw=np.asarray(t, F32), fx=F32(cam[0]), fy=F32(cam[1]), cx=F32(cam[2]),
                cy=F32(cam[3]))


def make(seed, n_pairs, extra=5, outliers=0.0, fix_scale=0, scale=1.0, all_points=0, no_idx2=0.0, capacity=None,
         shared=False, noise=0.8, start=(0.02, 1.0, 1.02), cam=TUM1, n1=None, identity=False):
    """-> scene dict.  start = (metres, degrees, scale factor) the input S12 is off the truth by."""
    rng = np.random.default_rng(seed)
    n1 = n1 or n_pairs + extra
    n2 = n_pairs + 7
    fx, fy, cx, cy = [float(F32(c)) for c in cam]
    if identity:
        R1, t1, R2, t2, Rs, ts = np.eye(3), np.zeros(3), np.eye(3), np.zeros(3), np.eye(3), np.zeros(3)
    else:
        R1, t1 = _rot(rng.normal(0, 0.3, 3)), rng.normal(0, 1.0, 3)
        R2, t2 = _rot(rng.normal(0, 0.3, 3)), rng.normal(0, 1.0, 3)
        Rs, ts = _rot(rng.normal(0, 0.08, 3)), rng.normal(0, 0.15, 3)
    truth = (sr.q_from_matrix(Rs), ts, float(scale))
    truth_inv = sr.sim3_inverse(truth)
    # the matched features of KF1, scattered among the unmatched
    feat = np.sort(rng.choice(n1, n_pairs, replace=False)) if n_pairs else np.zeros(0, np.int64)
    z = rng.uniform(2.0, 8.0, n_pairs)
    u, v = rng.uniform(60, 580, n_pairs), rng.uniform(60, 420, n_pairs)
    X1c = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1)
    X2c = sr.sim3_map(truth_inv, X1c) if n_pairs else np.zeros((0, 3))
    P1w, P2w = ((X1c - t1) @ R1).astype(F32), ((X2c - t2) @ R2).astype(F32)
    pose1, pose2 = _pose(R1, t1, cam), _pose(R2, t2, cam)
    X1c = sr.camera_points(pose1["Rcw"], pose1["tcw"], P1w).astype(np.float64)  # as the routine will see them
    X2c = sr.camera_points(pose2["Rcw"], pose2["tcw"], P2w).astype(np.float64)
    cap1 = capacity or max(n1 + 9, 16)
    cap2 = capacity or max(n2 + 11, 16)
    pos1 = rng.normal(0, 5, (cap1 + (cap2 if shared else 0), 3)).astype(F32)
    pos2 = pos1 if shared else rng.normal(0, 5, (cap2, 3)).astype(F32)
    perm1 = rng.permutation(cap1)
    perm2 = (cap1 + rng.permutation(cap2)) if shared else rng.permutation(cap2)
    if shared:
        cap1 = cap2 = cap1 + cap2
    slots1, slots2 = np.full(n1, -1, I32), np.full(n1, -1, I32)
    slots1[feat], slots2[feat] = perm1[:n_pairs], perm2[:n_pairs]
    # the unmatched: a point in KF1 only, a match without a point in KF1 (:3355-3373), neither
    rest = np.setdiff1d(np.arange(n1), feat)
    for k, i in enumerate(rest):
        if k % 3 == 0:
            slots1[i] = perm1[n_pairs + k]
        elif k % 3 == 1:
            slots2[i] = perm2[n_pairs + k]
    pos1[slots1[feat]] = P1w
    pos2[slots2[feat]] = P2w
    idx2 = np.full(n1, -1, I32)
    idx2[feat] = rng.permutation(n2)[:n_pairs]
    idx2[rest] = rng.integers(-1, n2, len(rest))
    if no_idx2 > 0 and n_pairs:
        idx2[rng.choice(feat, int(round(no_idx2 * n_pairs)), replace=False)] = -1
    level2 = rng.integers(0, NLEVELS, n1).astype(I32)
    oct1, oct2 = rng.integers(0, NLEVELS, n1).astype(I32), rng.integers(0, NLEVELS, n2).astype(I32)
    k1x, k1y = rng.uniform(20, 620, n1).astype(F32), rng.uniform(20, 460, n1).astype(F32)
    k2x, k2y = rng.uniform(20, 620, n2).astype(F32), rng.uniform(20, 460, n2).astype(F32)
    sig = np.sqrt(SIGMA2.astype(np.float64))
    is_out = np.zeros(n1, bool)
    if outliers > 0 and n_pairs:
        is_out[rng.choice(feat, int(round(outliers * n_pairs)), replace=False)] = True
    if n_pairs:
        p1 = sr.Problem._project((fx, fy, cx, cy), sr.sim3_map(truth, X2c))
        p2 = sr.Problem._project((fx, fy, cx, cy), sr.sim3_map(truth_inv, X1c))
        ang, mag = rng.uniform(0, 2 * math.pi, n_pairs), rng.uniform(6, 20, n_pairs)
        side = rng.random(n_pairs) < 0.5
        for k, i in enumerate(feat):
            i2 = idx2[i]
            s1 = sig[oct1[i]]
            d = np.array([math.cos(ang[k]), math.sin(ang[k])]) * mag[k] if is_out[i] else np.zeros(2)
            on1 = side[k] or i2 < 0
            o1 = p1[k] + rng.uniform(-noise, noise, 2) * s1 + (d * s1 if on1 else 0.0)
            k1x[i], k1y[i] = o1
            if i2 >= 0:
                s2 = sig[oct2[i2]]
                o2 = p2[k] + rng.uniform(-noise, noise, 2) * s2 + (0.0 if on1 else d * s2)
                k2x[i2], k2y[i2] = o2
    dr, dt = rng.normal(0, 1, 3), rng.normal(0, 1, 3)
    dS = (sr.q_from_matrix(_rot(dr / np.linalg.norm(dr) * math.radians(start[1]))), dt / np.linalg.norm(dt) * start[0],
          1.0 if fix_scale else start[2])
    S12 = sr.sim3_mul(dS, truth)
    return dict(n1=n1, n2=n2, slots1=slots1, slots2=slots2, idx2=idx2, level2=level2, cap1=cap1, cap2=cap2, pos1=pos1,
                pos2=pos2, shared=shared, kps1=dict(x=k1x, y=k1y, octave=oct1), kps2=dict(x=k2x, y=k2y, octave=oct2),
                pose1=pose1, pose2=pose2, sig1=INV_SIGMA2, sig2=INV_SIGMA2, nlevels=NLEVELS, S12=S12, th2=F32(TH2),
                fix_scale=int(fix_scale), all_points=int(all_points), truth=truth, is_out=is_out, feat=feat)


def candidates(s):
    return np.flatnonzero((s["slots1"] >= 0) & (s["slots2"] >= 0))


def _z_negative():
    s = make(401, 40, outliers=0.1)
    R2, t2 = s["pose2"]["Rcw"].reshape(3, 3).astype(np.float64), s["pose2"]["tcw"].astype(np.float64)
    s["z_negative"] = s["feat"][::6].copy()
    for i in s["z_negative"]:
        Xc = sr.camera_points(s["pose2"]["Rcw"], s["pose2"]["tcw"], s["pos2"][s["slots2"][i]])[0].astype(np.float64)
        Xc[2] = -Xc[2]
        s["pos2"][s["slots2"][i]] = ((Xc - t2) @ R2).astype(F32)
    return s


def _exact(n_pairs=24, seed=11):
    """Identity poses and S12, a dyadic camera and points: every error is exactly 0 at the start."""
    rng = np.random.default_rng(seed)
    s = make(seed, n_pairs, cam=DYADIC, identity=True, noise=0.0, start=(0.0, 0.0, 1.0))
    fx, fy, cx, cy = DYADIC
    X = np.stack([rng.integers(-8, 9, n_pairs) / 8.0, rng.integers(-6, 7, n_pairs) / 8.0, rng.choice([2.0, 4.0], n_pairs)], 1)
    f = s["feat"]
    s["pos1"][s["slots1"][f]] = X.astype(F32)
    s["pos2"][s["slots2"][f]] = X.astype(F32)
    px, py = (fx * X[:, 0] / X[:, 2] + cx).astype(F32), (fy * X[:, 1] / X[:, 2] + cy).astype(F32)
    s["kps1"]["x"][f], s["kps1"]["y"][f] = px, py
    s["kps2"]["x"][s["idx2"][f]], s["kps2"]["y"][s["idx2"][f]] = px, py
    s["S12"] = sr.sim3([0, 0, 0, 1], [0, 0, 0], 1.0)
    s["truth"] = s["S12"]
    return s


def _stale_errors(n_dbl=50, n_out=5, n_exact=150):
    """A FINITE scene in which the stale-error rule decides bits, on the recipe of pose_scenes._stale_errors.  Identity
    poses and S12, exact projections.  Each of n_dbl points is observed twice in KF1, at +2 px and -2 px (chi2 = 4 each:
    inliers whose gradients cancel), n_out more at +20 px and -20 px (chi2 = 400 each: they cancel as well, and the first
    check nulls them, so THEIR chi2 in the output are the first check's), n_exact observations are exact and ONE of them
    is moved by one float step.  The first step is accepted; a later one gains less than half an ulp of the cost, so
    tempChi == currentChi, rho == 0: the trial is REJECTED and the optimisation Terminates with the errors of the
    rejected state, which differ from those at the estimate by about 2e-8 on the 400.  That is below every tolerance
    against the restatement (the numeric Jacobian's noise decides how many trials it takes: a perturbed run
    can end by ten rejected trials instead, whose last step is too small to change a bit), so the rule is
    pinned on bits: the host build against its own FIRST_FRESH variant, the device against the host build."""
    n = 2 * (n_dbl + n_out) + n_exact
    s = _exact(n, seed=31)
    f = s["feat"]
    for k in range(n_dbl + n_out):
        a, b = f[2 * k], f[2 * k + 1]
        s["pos1"][s["slots1"][b]] = s["pos1"][s["slots1"][a]]
        s["pos2"][s["slots2"][b]] = s["pos2"][s["slots2"][a]]
        for kp, ia, ib in ((s["kps1"], a, b), (s["kps2"], s["idx2"][a], s["idx2"][b])):
            kp["x"][ib], kp["y"][ib] = kp["x"][ia], kp["y"][ia]
        d = F32(2.0 if k < n_dbl else 20.0)
        s["kps1"]["x"][a] += d
        s["kps1"]["x"][b] -= d
    s["kps1"]["octave"][:] = 0
    s["kps2"]["octave"][:] = 0
    s["kps1"]["x"][f[-1]] = np.nextafter(s["kps1"]["x"][f[-1]], F32(1e9))
    return s


def _stale_nan():
    """The stale-error rule where it decides VALUES: 9 pairs, so the call returns at the `< 10` gate and its chi2 outputs
    are the first check's.  One point is NaN: every trial's chi2 sum is NaN, so every trial is rejected (rho > 0 is
    false) and each of the five iterations leaves the errors of its rejected NaN candidate behind.  The first check
    therefore compares NaN for EVERY pair (NaN > th2 is false: nothing is nulled), where errors recomputed at the
    estimate -- the input, nothing was accepted -- are finite for eight of them."""
    s = make(31, 9)
    s["pos1"][s["slots1"][s["feat"][4]], 1] = np.nan
    return s


def _planted(seed=29):
    """Noise-free inliers with the input at the truth, plus eight pairs planted at 0.8x and 1.25x of th2, on either
    edge alone."""
    s = make(seed, 72, noise=0.0, start=(0.0, 0.0, 1.0))
    s["planted"] = {}
    sig = np.sqrt(SIGMA2.astype(np.float64))
    for k, (i, f) in enumerate(zip(s["feat"][:8], (0.8, 1.25) * 4)):
        on1 = k < 4
        i2 = s["idx2"][i]
        sg = sig[s["kps1"]["octave"][i]] if on1 else sig[s["kps2"]["octave"][i2]]
        d = F32(math.sqrt(f * TH2) * sg)
        kp, j = (s["kps1"], i) if on1 else (s["kps2"], i2)
        if k % 4 < 2:
            kp["x"][j] += d
        else:
            kp["y"][j] -= d
        s["planted"][int(i)] = f
    return s


@functools.lru_cache(maxsize=None)
def scenes():
    """name -> scene, in a fixed order."""
    out = {}
    for k, e in enumerate((0, 1, 9, 10, 11)):
        out["pairs_%d" % e] = make(100 + e, e, fix_scale=k % 2)
    for k, e in enumerate((63, 64, 65, 255, 256, 257)):
        out["pairs_%d" % e] = make(100 + e, e, extra=9, outliers=0.3, fix_scale=k % 2, scale=(1.0, 1.3)[(k // 2) % 2])
    out["kf_1000_300"] = make(204, 300, n1=1000, outliers=0.3, scale=1.3, capacity=4096)
    for fix in (0, 1):
        for sc in (1.0, 1.3):
            tag = "fix%d_s%s" % (fix, "1" if sc == 1.0 else "13")
            out["clean_" + tag] = make(210 + 2 * fix + (sc > 1), 65, fix_scale=fix, scale=sc)
            out["outliers_" + tag] = make(220 + 2 * fix + (sc > 1), 65, outliers=0.3, fix_scale=fix, scale=sc)
    out["all_points_0"] = make(231, 90, outliers=0.1, all_points=0, no_idx2=1.0 / 3.0)
    out["all_points_1"] = make(231, 90, outliers=0.1, all_points=1, no_idx2=1.0 / 3.0)
    out["shared_store"] = make(232, 70, outliers=0.2, shared=True)
    out["far_start"] = make(233, 100, outliers=0.1, start=(0.1, 4.0, 1.1))
    out["z_negative"] = _z_negative()
    out["return_zero_after_nulling"] = make(241, 12, outliers=4.0 / 12.0)
    out["no_bad_five_iterations"] = make(242, 40)
    out["bad_ten_iterations"] = make(242, 40, outliers=0.25)
    out["planted"] = _planted()
    out["exact_start"] = _exact()
    out["stale_errors"] = _stale_errors()
    out["stale_nan"] = _stale_nan()
    un = make(243, 50, outliers=0.2)
    un["S12"] = (un["S12"][0] * 1.001, un["S12"][1], un["S12"][2])  # a quaternion of norm 1.001, taken as it is
    out["unnormalised_input"] = un
    nanp = make(244, 30, outliers=0.1, start=(0.0, 0.0, 1.0))
    nanp["pos2"][nanp["slots2"][nanp["feat"][7]], 0] = np.nan
    out["nan_point"] = nanp
    return out


def reference(s, order=None, jitter=None, solver="ldlt"):
    return sr.optimize_sim3(s["slots1"], s["slots2"], s["idx2"], s["level2"], s["pos1"], s["pos2"], s["kps1"], s["kps2"],
                            s["pose1"], s["pose2"], s["sig1"], s["sig2"], s["S12"], s["th2"], s["fix_scale"],
                            s["all_points"], order, jitter, solver)


@functools.lru_cache(maxsize=None)
def references():
    """name -> the restatement's result, computed once for all tests."""
    return {name: reference(s) for name, s in scenes().items()}


@functools.lru_cache(maxsize=None)
def perturbed_references():
    """name -> the restatement's results under the N_PERT members of the perturbation set."""
    out = {}
    for k, (name, s) in enumerate(scenes().items()):
        rng = np.random.default_rng(900 + k)
        E = references()[name]["n_correspondences"]
        out[name] = [reference(s, rng.permutation(E), sr.Jitter(7000 + 10 * k + m), "numpy" if m % 2 else "ldlt")
                     for m in range(N_PERT)]
    return out


def deviations(a, b):
    """Largest differences between two results that agree on the states: q, t absolute, s relative, chi2 relative to
    max(|chi2|, 1).  NaN entries (both) are skipped."""
    def amax(x, y):
        d = np.abs(np.asarray(x, np.float64) - np.asarray(y, np.float64))
        d = d[np.isfinite(d)]
        return float(d.max()) if d.size else 0.0
    dq, dt = amax(a["S12"][0], b["S12"][0]), amax(a["S12"][1], b["S12"][1])
    sa, sb = float(a["S12"][2]), float(b["S12"][2])
    ds = abs(sa - sb) / abs(sa) if math.isfinite(sa) and math.isfinite(sb) and sa != 0 else 0.0
    dc = 0.0
    for f, ca in a["chi2"].items():
        for x, y in zip(ca, b["chi2"][f]):
            if np.isfinite(x) and np.isfinite(y):
                dc = max(dc, abs(float(x) - float(y)) / max(abs(float(x)), abs(float(y)), 1.0))
    return dict(q=dq, t=dt, s=ds, chi2_rel=dc)


def same_decisions(a, b):
    return (a["ret"] == b["ret"] and a["n_bad"] == b["n_bad"] and a["n_in"] == b["n_in"] and
            a["more_iterations"] == b["more_iterations"] and np.array_equal(a["state"], b["state"]))


def measure():
    spread = dict(q=0.0, t=0.0, s=0.0, chi2_rel=0.0)
    worst = dict(spread)
    for name, ref in references().items():
        for p in perturbed_references()[name]:
            for k, v in deviations(ref, p).items():
                if v > spread[k]:
                    spread[k], worst[k] = v, name
    return spread, worst


if __name__ == "__main__" and "--measure" in sys.argv:
    sp, worst = measure()
    # never below one rounding of the quantity itself (unit-size doubles)
    sp = {k: max(v, 2.0 ** -52) for k, v in sp.items()}
    print("SPREAD = dict(q=%r, t=%r, s=%r, chi2_rel=%r)" % (sp["q"], sp["t"], sp["s"], sp["chi2_rel"]))
    print("# worst scenes:", worst)
