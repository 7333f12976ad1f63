"""Seeded scenes for the local-BA tests (tests/test_lba_*.py, tests/test_gpu_local_bundle_adjustment.py): keyframes around
the origin looking down +z with a TUM1-like camera (bf = 40), map points 3 to 8 m in front of them, every observation a
feature of its keyframe with UNIFORM noise within +-0.8 sigma of its level per axis (an inlier's chi2 stays under
3 * 0.64 = 1.92, far from 5.991 / 7.815), outliers displaced by at least 20 px, the optimised keyframes and the points
started 1 cm / 0.5 degrees off.  Mono-only scenes have at least two fixed keyframes, so that scale is held.

Sizes are the smallest at which the kernels can go wrong: 1 / 2 / 3 optimised keyframes with 1 / 2 fixed; 1, 63 / 64 / 65
(seen by every keyframe: a keyframe with 63 / 64 / 65 edges) and 255 / 256 / 257 points; a point with 1, 2 and 40
observations; 40 optimised keyframes (a reduced system of 240 rows); all-mono, all-stereo, mixed; 0 % and 20 % outliers;
an optimised keyframe without edges, a point seen only by fixed keyframes, a point with an empty list, fixed keyframes at
the head (kfs[0]) and at the tail of the array.  Directed scenes follow, each with a condition that
tests/test_lba_reference.py asserts on the restatement alone.

Every scene keeps every compared chi2 more than 1e-3 (relative) away from its threshold, under 8 random permutations of
the edge order too (test_lba_reference.py::test_fixture_condition): no edge is excluded from any flag comparison.

SPREAD / TOL below are MEASURED, not chosen: the largest deviation of the restatement from itself over those 8
permutations, per quantity, over all scenes, and 64 times that (the rule and the reasons of pose_scenes.py).  Where a
spread measures below one rounding of the quantity the FLOOR of one ulp of the compared type is used instead, a chosen
number: 2^-52 for the unit-size doubles of a pose and the relative chi2, 2^-23 (relative to at least 1 m) for the float positions.
Produced by
    python tests/lba_scenes.py --measure

cap_scenes() holds three further scenes, 16 / 17 / 128 optimised keyframes (96 / 102 / 768 rows of the reduced system), apart
from scenes() and with a spread of their own, SPREAD_CAP / TOL_CAP, measured the same way over those three alone.
"""
import functools
import math
import sys

import numpy as np

import lba_reference as lr
import pose_reference as pr
from pose_scenes import DYADIC, INV_SIGMA2, NLEVELS, SIGMA2, TUM1, _rot

F32, I32, U8 = np.float32, np.int32, np.uint8
N_PERM = 8

# measured (see the module docstring): largest |difference| between edge orders, and 64 x that
# q, t and chi2_rel are measured values.  pos_rel is NOT: the float positions come out identical under every order, so the
# constant is the FLOOR 2^-23 = one ulp of the compared float, a chosen number reasoned from the format.
SPREAD = dict(q=1.4952444664373399e-12, t=1.2295858775601687e-11, pos_rel=1.1920928955078125e-07, chi2_rel=4.986082785789947e-08)
TOL = {k: 64 * v for k, v in SPREAD.items()}
# the same measurement over cap_scenes() ALONE (the three scenes of the reduced system at its tile and at its cap), with
# the same floors (pos_rel is the floor here too); the code under test takes no part in it
SPREAD_CAP = dict(q=9.811595980124821e-15, t=1.4410694859634532e-13, pos_rel=1.1920928955078125e-07, chi2_rel=1.0829712049060172e-10)
TOL_CAP = {k: 64 * v for k, v in SPREAD_CAP.items()}


def _pose7(R, t):
    return np.concatenate([pr.q_normalize(pr.q_from_matrix(R)), t])


def make(seed, n_opt, n_fix, n_points, n_obs, kind="mixed", outliers=0.0, start=(0.01, 0.5), fixed_first=True, noise=0.8,
         cam=TUM1, iterations=10, empty_kf=False, fixed_only_point=False, empty_point=False, obs_all_first=False,
         single_obs_point=False):
    """-> scene dict.  n_obs = observations per point (at most the keyframe count); start = (metres, degrees)."""
    rng = np.random.default_rng(seed)
    K = n_opt + n_fix
    fixed = np.zeros(K, U8)
    fixed[:n_fix] = 1
    if not fixed_first:
        fixed = fixed[::-1].copy()
    fx, fy, cx, cy, bf = [float(F32(c)) for c in cam]
    Rs = [_rot(rng.normal(0, 0.04, 3)) for _ in range(K)]
    cs = [np.array([rng.uniform(-0.6, 0.6), rng.uniform(-0.4, 0.4), rng.uniform(-0.2, 0.2)]) for _ in range(K)]
    ts = [-R @ c for R, c in zip(Rs, cs)]
    Xw = np.stack([rng.uniform(-1.5, 1.5, n_points), rng.uniform(-1.0, 1.0, n_points), rng.uniform(3.0, 8.0, n_points)], 1).astype(F32)
    kfs = [dict(x=[F32(rng.uniform(20, 620)), F32(rng.uniform(20, 620))], y=[F32(rng.uniform(20, 460)), F32(rng.uniform(20, 460))],
                octave=[0, 1], ur=[F32(-1), F32(-1)]) for _ in range(K)]  # two features no point observes
    stereo_kind = {"mono": lambda: False, "stereo": lambda: True, "mixed": lambda: bool(rng.random() < 0.5)}[kind]
    obs_off, obs_kf, obs_idx, is_out = [0], [], [], []
    fixed_ids, opt_ids = np.flatnonzero(fixed), np.flatnonzero(fixed == 0)
    for p in range(n_points):
        m = min(K, n_obs)
        seen = np.sort(rng.choice(K, m, replace=False))
        if obs_all_first and p == 0:
            seen = np.arange(K)
        if fixed_only_point and p == 1:
            seen = fixed_ids
        if single_obs_point and p == 2:
            seen = opt_ids[:1]
        if empty_point and p == 3:
            seen = seen[:0]
        for k in seen:
            Xc = Rs[k] @ Xw[p].astype(np.float64) + ts[k]
            o = int(rng.integers(0, NLEVELS))
            sg = math.sqrt(float(SIGMA2[o]))
            nz = rng.uniform(-noise, noise, 3) * sg
            out = bool(rng.random() < outliers)
            ang, mag = rng.uniform(0, 2 * math.pi), rng.uniform(20, 60)
            du, dv = (mag * math.cos(ang), mag * math.sin(ang)) if out else (0.0, 0.0)
            u, v = fx * Xc[0] / Xc[2] + cx, fy * Xc[1] / Xc[2] + cy
            st = stereo_kind() or (single_obs_point and p == 2) or (fixed_only_point and p == 1 and len(fixed_ids) < 2)
            f = kfs[k]
            f["x"].append(F32(u + nz[0] + du)), f["y"].append(F32(v + nz[1] + dv)), f["octave"].append(o)
            f["ur"].append(F32(u - bf / Xc[2] + nz[2] + du) if st else F32(-1))
            obs_kf.append(k), obs_idx.append(len(f["x"]) - 1), is_out.append(out)
        obs_off.append(len(obs_kf))
    if empty_kf:  # an optimised keyframe nothing observes, in the middle of the array
        at = K // 2
        kfs.insert(at, dict(x=[F32(100), F32(200)], y=[F32(100), F32(200)], octave=[0, 1], ur=[F32(-1), F32(-1)]))
        Rs.insert(at, np.eye(3)), ts.insert(at, np.array([0.1, 0.2, 0.3]))
        fixed = np.insert(fixed, at, 0)
        obs_kf = [k + 1 if k >= at else k for k in obs_kf]
        K += 1
    Tcw = np.zeros((K, 7), F32)
    for k in range(K):
        R, t = Rs[k], ts[k]
        if not fixed[k]:
            a, d = rng.normal(0, 1, 3), rng.normal(0, 1, 3)
            dR = _rot(a / np.linalg.norm(a) * math.radians(start[1]))
            R, t = dR @ R, dR @ t + d / np.linalg.norm(d) * start[0]
        Tcw[k] = _pose7(R, t).astype(F32)
    capacity = max(n_points + 9, 16)
    slots = rng.permutation(capacity)[:n_points].astype(I32)
    store_pos = rng.normal(0, 5, (capacity, 3)).astype(F32)
    d = rng.normal(0, 1, (n_points, 3))
    store_pos[slots] = (Xw + d / np.linalg.norm(d, axis=1)[:, None] * start[0]).astype(F32)
    for f in kfs:
        f["x"], f["y"], f["octave"] = np.array(f["x"], F32), np.array(f["y"], F32), np.array(f["octave"], I32)
        f["ur"] = None if kind == "mono" and not (np.array(f["ur"]) >= 0).any() else np.array(f["ur"], F32)
    return dict(kfs=kfs, Tcw=Tcw, fixed=fixed.astype(U8), cam=np.tile(np.array(cam, F32), (K, 1)), sig=INV_SIGMA2, nlevels=NLEVELS,
                iterations=iterations, capacity=capacity, store_pos=store_pos, slots=slots, obs_off=np.array(obs_off, I32),
                obs_kf=np.array(obs_kf, I32), obs_idx=np.array(obs_idx, I32), is_out=np.array(is_out, bool))


def _with_start(s, ref):
    """The scene started where an earlier run ended (rounded to float)."""
    s = dict(s)
    s["Tcw"] = ref["kf_out"].astype(F32)
    s["store_pos"] = s["store_pos"].copy()
    s["store_pos"][s["slots"]] = ref["pos_out"]
    return s


def _exact(stale=False, n_pairs=50):
    """Identity rotations, dyadic translations, a camera and points whose projections are exact: every error is exactly 0
    at the start, the first step is exactly 0, rho == 0: Terminate in iteration 0.

    stale: a FINITE scene in which the stale-error rule decides compared doubles, under every summation order.  n_pairs
    further points are seen by the fixed keyframe 0 alone, each TWICE, at +2 px and -2 px (chi2 = 4 each: inliers whose
    gradients cancel exactly, a constant cost of 8 per point), and ONE exact observation, of level 7 whose information this
    scene sets to 1e-8, is moved by one float step: its chi2 of about 1e-17 is below half an ulp of 4, so the cost is 400
    exactly in any order, before and after the first step.  tempChi == currentChi, rho == 0: the FIRST trial is REJECTED
    and the run Terminates.  The gradient is not zero, the step moved every coordinate that was 0, and the errors compared
    are those of that rejected state: tiny where the restored estimates give exactly 0."""
    rng = np.random.default_rng(41)
    fx, fy, cx, cy, bf = DYADIC
    K, n = 4, 24
    ts = [np.zeros(3), np.array([0.25, 0.0, 0.0]), np.array([0.0, 0.125, 0.0]), np.array([-0.25, 0.125, 0.0])]
    X = np.stack([rng.integers(-8, 9, n) / 8.0, rng.integers(-6, 7, n) / 8.0, rng.choice([2.0, 4.0], n)], 1)
    if stale:
        X = np.concatenate([X, np.stack([rng.integers(-8, 9, n_pairs) / 8.0, rng.integers(-6, 7, n_pairs) / 8.0,
                                         rng.choice([2.0, 4.0], n_pairs)], 1)])
    P = len(X)
    kfs = [dict(x=[], y=[], octave=[], ur=[]) for _ in range(K)]
    obs_off, obs_kf, obs_idx = [0], [], []
    for p in range(P):
        pair = p >= n
        for k in ([0, 0] if pair else range(K)):
            Xc = X[p] + ts[k]
            u, v = fx * Xc[0] / Xc[2] + cx, fy * Xc[1] / Xc[2] + cy
            st = (p + k) % 2 == 0 and not stale  # the float 1 / z of a stereo edge is a step function at this scale
            if pair:
                u += 2.0 if len(obs_kf) == obs_off[-1] else -2.0
            f = kfs[k]
            f["x"].append(F32(u)), f["y"].append(F32(v)), f["octave"].append(0), f["ur"].append(F32(u - bf / Xc[2]) if st else F32(-1))
            obs_kf.append(k), obs_idx.append(len(f["x"]) - 1)
        obs_off.append(len(obs_kf))
    if stale:  # the last observation of point 0 (the last keyframe): one float step off
        i = obs_idx[obs_off[1] - 1]
        kfs[K - 1]["octave"][i] = 7
        kfs[K - 1]["x"][i] = np.nextafter(kfs[K - 1]["x"][i], F32(1e9))
    for f in kfs:
        f["x"], f["y"], f["octave"], f["ur"] = np.array(f["x"], F32), np.array(f["y"], F32), np.array(f["octave"], I32), np.array(f["ur"], F32)
    Tcw = np.array([np.concatenate([[0, 0, 0, 1], t]) for t in ts], F32)
    capacity = P + 8
    slots = np.arange(P, dtype=I32)[::-1].copy() + 3
    store_pos = rng.normal(0, 5, (capacity, 3)).astype(F32)
    store_pos[slots] = X.astype(F32)
    sig = INV_SIGMA2.copy()
    if stale:
        sig[7] = F32(1e-8)
    return dict(kfs=kfs, Tcw=Tcw, fixed=np.array([1, 1, 0, 0], U8), cam=np.tile(np.array(DYADIC, F32), (K, 1)), sig=sig,
                nlevels=NLEVELS, iterations=10, capacity=capacity, store_pos=store_pos, slots=slots, obs_off=np.array(obs_off, I32),
                obs_kf=np.array(obs_kf, I32), obs_idx=np.array(obs_idx, I32), is_out=np.zeros(len(obs_kf), bool))


def _behind():
    """A fixed keyframe that looks the other way observes eight points at their pinhole projections: small errors, negative
    depth -- erased by isDepthPositive alone."""
    s = make(501, 2, 2, 40, 3)
    rng = np.random.default_rng(502)
    fx, fy, cx, cy, bf = [float(F32(c)) for c in TUM1]
    R, t = np.diag([-1.0, 1.0, -1.0]), np.array([0.1, 0.0, 0.5])  # half a turn about y
    f = dict(x=[], y=[], octave=[], ur=[])
    off, kf, idx = list(s["obs_off"]), list(s["obs_kf"]), list(s["obs_idx"])
    K = len(s["kfs"])
    truth = s["store_pos"][s["slots"]].astype(np.float64)
    new_kf, new_idx, new_off = [], [], [0]
    for p in range(len(s["slots"])):
        new_kf += kf[off[p]:off[p + 1]]
        new_idx += idx[off[p]:off[p + 1]]
        if p % 5 == 0:
            Xc = R @ truth[p] + t
            f["x"].append(F32(fx * Xc[0] / Xc[2] + cx + rng.uniform(-0.5, 0.5))), f["y"].append(F32(fy * Xc[1] / Xc[2] + cy + rng.uniform(-0.5, 0.5)))
            f["octave"].append(0), f["ur"].append(F32(-1))
            new_kf.append(K), new_idx.append(len(f["x"]) - 1)
        new_off.append(len(new_kf))
    f["x"], f["y"], f["octave"], f["ur"] = np.array(f["x"], F32), np.array(f["y"], F32), np.array(f["octave"], I32), np.array(f["ur"], F32)
    s["kfs"] = s["kfs"] + [f]
    s["Tcw"] = np.concatenate([s["Tcw"], _pose7(R, t).astype(F32)[None]])
    s["fixed"] = np.concatenate([s["fixed"], [1]]).astype(U8)
    s["cam"] = np.tile(np.array(TUM1, F32), (K + 1, 1))
    s["obs_off"], s["obs_kf"], s["obs_idx"] = np.array(new_off, I32), np.array(new_kf, I32), np.array(new_idx, I32)
    s["is_out"] = np.zeros(len(new_kf), bool)
    return s


def _negative_information():
    """mvInvLevelSigma2 with its sign flipped: every block of the system is negative, the reduced factorisation meets a
    non-positive pivot (ok2 = false, tempChi = DBL_MAX) until lambda outgrows the diagonal."""
    s = make(503, 2, 1, 30, 3, "stereo")
    s["sig"] = (-INV_SIGMA2).astype(F32)
    return s


@functools.lru_cache(maxsize=None)
def scenes():
    """name -> scene, in a fixed order."""
    out = {}
    out["one_point"] = make(601, 1, 1, 1, 2, "stereo")
    for n_opt, n_fix in ((1, 1), (2, 1), (3, 2), (1, 2)):
        out["kf_%d_%d" % (n_opt, n_fix)] = make(610 + 3 * n_opt + n_fix, n_opt, n_fix, 40, 3)
    for n in (63, 64, 65):
        out["points_%d_all" % n] = make(620 + n, 2, 1, n, 3, outliers=0.2 if n == 64 else 0.0)
    for n in (255, 256, 257):
        out["points_%d" % n] = make(630 + n, 3, 2, n, 3, outliers=0.2 if n == 257 else 0.0)
    out["mono_clean"] = make(641, 3, 2, 80, 4, "mono")
    out["mono_outliers"] = make(642, 3, 2, 80, 4, "mono", outliers=0.2)
    out["stereo_clean"] = make(643, 2, 1, 80, 3, "stereo")
    out["stereo_outliers"] = make(644, 2, 1, 80, 3, "stereo", outliers=0.2)
    out["two_observations"] = make(645, 2, 2, 70, 2)
    out["fixed_last"] = make(646, 2, 2, 50, 3, fixed_first=False)
    out["special_vertices"] = make(647, 3, 2, 60, 3, empty_kf=True, fixed_only_point=True, empty_point=True, single_obs_point=True)
    out["kf_40"] = make(648, 40, 2, 120, 5, obs_all_first=True)
    out["far_start"] = make(651, 3, 2, 80, 4, outliers=0.1, start=(0.25, 6.0))  # an iteration whose first trial is rejected
    base = make(652, 2, 2, 60, 3)
    out["converged_start"] = _with_start(base, lr.local_ba(base))  # ends by _nBad >= 3
    out["exact_start"] = _exact()                                   # ends by Terminate (rho == 0)
    out["stale_errors"] = _exact(stale=True)                        # a rejected last trial: the compared chi2 is stale
    out["behind_camera"] = _behind()
    out["negative_information"] = _negative_information()           # a non-positive pivot
    return out


@functools.lru_cache(maxsize=None)
def references():
    """name -> the restatement's result, computed once for all tests."""
    return {name: lr.local_ba(s) for name, s in scenes().items()}


@functools.lru_cache(maxsize=None)
def permuted_references():
    """name -> the restatement's results under N_PERM random edge orders."""
    out = {}
    for k, (name, s) in enumerate(scenes().items()):
        rng = np.random.default_rng(900 + k)
        out[name] = [lr.local_ba(s, rng.permutation(int(s["obs_off"][-1]))) for _ in range(N_PERM)]
    return out


# n_opt -> (seed, points, iterations): 96 rows (three whole tiles of lba::kSolveTile = 32), 102 rows (three tiles and six
# rows) and 768 rows (the cap, 6 * lba::kMaxOptKf: l, D and y of k_solve full).  Four observations per point among the
# n_opt + 2 keyframes; the seeds are the first from 861 / 871 / 881 on for which every optimised keyframe is observed and the
# restatement meets the fixture condition (test_lba_reference.py::test_cap_fixture_condition).
CAP_SCENES = {16: (861, 60, 10), 17: (871, 60, 10), 128: (881, 400, 10)}
CAP_NAMES = tuple("rows_%d" % (6 * n_opt) for n_opt in CAP_SCENES)


@functools.lru_cache(maxsize=None)
def cap_scenes():
    """name -> scene: the reduced system at whole tiles, one keyframe past them, and at its cap.  Kept apart from scenes():
    SPREAD and TOL are measured over scenes() alone."""
    return {"rows_%d" % (6 * n_opt): make(seed, n_opt, 2, n_points, 4, iterations=its)
            for n_opt, (seed, n_points, its) in CAP_SCENES.items()}


@functools.lru_cache(maxsize=None)
def cap_references():
    return {name: lr.local_ba(s) for name, s in cap_scenes().items()}


@functools.lru_cache(maxsize=None)
def cap_permuted_references():
    out = {}
    for k, (name, s) in enumerate(cap_scenes().items()):
        rng = np.random.default_rng(950 + k)
        out[name] = [lr.local_ba(s, rng.permutation(int(s["obs_off"][-1]))) for _ in range(N_PERM)]
    return out


def deviations(a, b):
    """Largest differences between two results: q, t absolute; positions relative to max(|coordinate|, 1 m); chi2 relative
    to max(|chi2|, 1e-6)."""
    with np.errstate(all="ignore"):
        dq = float(np.nanmax(np.abs(a["kf_out"][:, :4] - b["kf_out"][:, :4]), initial=0.0))
        dt = float(np.nanmax(np.abs(a["kf_out"][:, 4:] - b["kf_out"][:, 4:]), initial=0.0))
        pa, pb = a["pos_out"].astype(np.float64), b["pos_out"].astype(np.float64)
        dp = float(np.nanmax(np.abs(pa - pb) / np.maximum(np.maximum(np.abs(pa), np.abs(pb)), 1.0), initial=0.0))
        ca, cb = np.asarray(a["chi2"], np.float64), np.asarray(b["chi2"], np.float64)
        ok = np.isfinite(ca) & np.isfinite(cb)
        dc = float(np.nanmax((np.abs(ca - cb) / np.maximum(np.maximum(np.abs(ca), np.abs(cb)), 1e-6))[ok], initial=0.0))
    return dict(q=dq, t=dt, pos_rel=dp, chi2_rel=dc)


def measure(cap=False):
    """The spread over scenes(), or over cap_scenes() alone."""
    refs, perms = (cap_references(), cap_permuted_references()) if cap else (references(), permuted_references())
    spread = dict(q=0.0, t=0.0, pos_rel=0.0, chi2_rel=0.0)
    for name, ref in refs.items():
        for p in perms[name]:
            for k, v in deviations(ref, p).items():
                spread[k] = max(spread[k], v)
    return spread


if __name__ == "__main__" and "--measure" in sys.argv:
    floor = dict(q=2.0 ** -52, t=2.0 ** -52, pos_rel=2.0 ** -23, chi2_rel=2.0 ** -52)
    for name, cap in (("SPREAD", False), ("SPREAD_CAP", True)):
        sp = {k: max(v, floor[k]) for k, v in measure(cap).items()}
        print("%s = dict(q=%r, t=%r, pos_rel=%r, chi2_rel=%r)" % (name, sp["q"], sp["t"], sp["pos_rel"], sp["chi2_rel"]))
