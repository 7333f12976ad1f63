"""Seeded pose graphs for Optimizer::OptimizeEssentialGraph: a drifting chain of keyframes with a loop, covisibility edges
and CorrectedSim3 on the keyframes around the current one, at scale drift 1.0 and 1.3 crossed with fix_scale 0 and 1, and
directed scenes (a keyframe without an edge, no fixed keyframe, a duplicate edge pair, a fixed-fixed edge, one edge starting
in each of the four branches of Sim3::log(), an estimate whose errors overflow to NaN).

ITERATIONS.  With lambda starting at 1e-16 the loop converges in a few steps and then sits at the noise floor, where the last
bit of a sum decides whether a trial is accepted: g2o itself would decide those trials differently on another libm.  The
tests compare the decisions EXACTLY, so a scene whose endgame is decided that way stops after 3 iterations, before it; the
others run the reference's 20.  The singular scene's seed is one whose pivots' signs (noise too) come out the same over the
whole perturbation set.  tests/test_eg_reference.py asserts, on the restatement alone, that every member of the perturbation
set takes the decisions of the unperturbed run in every scene.

references() runs the restatement (eg_reference.py) once per scene; perturbed_references() runs it under the perturbation
set (libm results moved by +-1 ulp, LAPACK in the place of the LDL^T); measure() is the spread of the restatement over that
set, the numeric Jacobian amplifying rounding by 5e8.  SPREAD is that measurement as committed, TOL = 16 SPREAD what the
header's host build is held to (tests/test_eg_hostmath.py); test_eg_reference.py bounds a fresh measurement against the
committed one from both sides.

    python tests/eg_scenes.py --measure     prints the SPREAD line"""
import functools
import math
import sys

import numpy as np

import eg_reference as er

F32, F64, I32, U8 = np.float32, np.float64, np.int32, np.uint8
N_PERT = 4
SPREAD = dict(q=4.075358664445451e-06, t=5.5400122882742764e-05, s=1.3578494249062019e-06, pos=8.082389831542969e-05,
              chi2_rel=2.476683556573711e-07)
TOL = {k: 16 * v for k, v in SPREAD.items()}


def _axis_angle(axis, angle):
    axis = np.asarray(axis, F64) / np.linalg.norm(axis)
    return np.concatenate([math.sin(angle / 2) * axis, [math.cos(angle / 2)]])


def _sim3(q, t, s):
    return np.concatenate([np.asarray(q, F64), np.asarray(t, F64), [float(s)]])


def _mul(a, b):
    return er.pack(er.s_mul(er.sim3(a), er.sim3(b)))


def _inv(a):
    return er.pack(er.s_inv(er.sim3(a)))


def graph(K, cur, loop_kf):
    """parent / children = the chain, covisibles by falling weight, one older loop edge, the LoopConnections of a loop
    between cur and loop_kf with one connection under minFeat that is kept (the pair itself) and one that is dropped."""
    parent = [k - 1 for k in range(K)]
    children = [{k + 1} if k + 1 < K else set() for k in range(K)]
    cov = [[j for d in (1, 2, 3) for j in (k - d, k + d) if 0 <= j < K] for k in range(K)]
    loops = [[] for _ in range(K)]
    if K >= 9:
        loops[7].append(2), loops[2].append(7)
    lc = [(cur, [(loop_kf, 30), (loop_kf + 1, 150)]), (cur - 1, [(loop_kf, 120), (loop_kf + 1, 50)])]
    return dict(parent=parent, children=children, covisibles=cov, loops=loops, loop_connections=lc, cur=cur, loop_kf=loop_kf)


def _poses(rng, K, scale, n_corrected, rot, trans):
    """(GetPose(), 1.0) of K keyframes on a drifting arc; the last n_corrected carry CorrectedSim3 = pose * C and keep their
    pose as NonCorrectedSim3."""
    S = np.zeros((K, 8))
    for k in range(K):
        a = 2 * math.pi * 0.85 * k / K
        q_wc = er.q_mul(_axis_angle([0, 0, 1], a + 0.004 * k * k / K), _axis_angle(rng.normal(size=3), 0.05))
        t_wc = np.array([5 * math.cos(a), 5 * math.sin(a), 0.1 * rng.normal()]) * (1 + 0.01 * k) + 0.03 * rng.normal(size=3)
        q_cw = q_wc * np.array([-1.0, -1, -1, 1])
        S[k] = _sim3(q_cw, -er.q_rotate(q_cw, t_wc), 1.0)
    C = _sim3(_axis_angle(rng.normal(size=3), rot), trans * rng.normal(size=3), scale)
    nonc, has = np.zeros((K, 8)), np.zeros(K, U8)
    nonc[:, 3] = nonc[:, 7] = 1.0
    Scw = S.copy()
    for k in range(max(K - n_corrected, 1), K):
        nonc[k], has[k], Scw[k] = S[k], 1, _mul(S[k], C)
    return Scw, nonc, has


def sized(seed, n_opt, n_edges=None, hub=None, covis=0, scale=1.1, fix_scale=0, iterations=2, points_per_kf=2, n_fixed=1):
    """A graph of a given SIZE for the device tests: n_fixed fixed keyframes, then n_opt optimised ones on a chain (keyframe k
    joined to k - 1, and to k - 2 .. k - 1 - covis); then random further edges up to n_edges in all, or, with hub = (vertex,
    count), edges between that vertex and the others in turn until it has `count` (duplicate pairs among them)."""
    rng = np.random.default_rng(seed)
    K = n_opt + n_fixed
    Scw, nonc, has = _poses(rng, K, scale, min(3, n_opt), 0.08, 0.3)
    ei = [k for k in range(1, K) for d in range(1, covis + 2) if k - d >= 0]
    ej = [k - d for k in range(1, K) for d in range(1, covis + 2) if k - d >= 0]
    el = [0] * len(ei)
    if n_edges is not None:
        ei, ej, el = ei[:n_edges], ej[:n_edges], el[:n_edges]
        while len(ei) < n_edges:
            i, j = (int(v) for v in rng.choice(K, 2, replace=False))
            ei.append(max(i, j)), ej.append(min(i, j)), el.append(int(rng.integers(0, 2)))
    if hub is not None:
        v, count = hub
        have, turn = sum(1 for i, j in zip(ei, ej) if v in (i, j)), 0
        while have < count:
            o = turn % K
            turn += 1
            if o == v:
                continue
            (ei.append(v), ej.append(o)) if turn % 2 else (ei.append(o), ej.append(v))
            el.append(turn % 3 == 0)
            have += 1
    fixed = np.zeros(K, U8)
    fixed[:n_fixed] = 1
    P = points_per_kf * K
    cap = P + 5
    return dict(Scw=Scw, nonc=nonc, has=has, fixed=fixed, ei=np.array(ei, I32), ej=np.array(ej, I32), eloop=np.array(el, U8),
                fix_scale=fix_scale, iterations=iterations, slots=rng.permutation(cap)[:P].astype(I32),
                point_ref=rng.integers(0, K, P).astype(I32), store_pos=rng.uniform(-5, 5, (cap, 3)).astype(F32), capacity=cap,
                graph=None)


def make(seed, K=12, scale=1.0, fix_scale=0, n_corrected=3, points_per_kf=4, iterations=20, rot=0.08, trans=0.3):
    rng = np.random.default_rng(seed)
    Scw, nonc, has = _poses(rng, K, scale, n_corrected, rot, trans)
    g = graph(K, K - 1, 1)
    ei, ej, el = er.build_edges(g["parent"], g["loops"], g["children"], g["covisibles"], g["loop_connections"], g["cur"], g["loop_kf"])
    fixed = np.zeros(K, U8)
    fixed[0] = 1
    P = points_per_kf * K
    cap = P + 7
    return dict(Scw=Scw, nonc=nonc, has=has, fixed=fixed, ei=ei, ej=ej, eloop=el, fix_scale=fix_scale, iterations=iterations,
                slots=rng.permutation(cap)[:P].astype(I32), point_ref=rng.integers(0, K, P).astype(I32),
                store_pos=rng.uniform(-5, 5, (cap, 3)).astype(F32), capacity=cap, graph=g)


def _log_branches():
    """Keyframe 0 fixed; keyframes 1 .. 4 each joined to it by one normal edge whose first error is the correction C_k:
    small sigma / near, small sigma / far, large sigma / near, large sigma / far."""
    s = make(301, K=5, n_corrected=0, points_per_kf=3, iterations=3)
    Cs = [_sim3(_axis_angle([1, 2, 3], 1e-4), [0.02, -0.01, 0.03], 1.0), _sim3(_axis_angle([1, -1, 2], 0.2), [0.1, 0.2, -0.1], 1.0),
          _sim3(_axis_angle([3, 1, -2], 1e-4), [0.05, 0.02, -0.04], 1.2), _sim3(_axis_angle([-1, 2, 1], 0.3), [-0.2, 0.1, 0.1], 0.8)]
    for k, C in enumerate(Cs, 1):
        s["nonc"][k], s["has"][k] = s["Scw"][k], 1
        s["Scw"][k] = _mul(s["Scw"][k], C)
    s["ei"], s["ej"], s["eloop"] = np.arange(1, 5, dtype=I32), np.zeros(4, I32), np.zeros(4, U8)
    s["graph"] = None
    return s


@functools.lru_cache(maxsize=None)
def scenes():
    out = {}
    for fix in (0, 1):
        for sc in (1.0, 1.3):
            out["loop_fix%d_s%s" % (fix, "1" if sc == 1.0 else "13")] = make(110 + 2 * fix + (sc > 1), scale=sc, fix_scale=fix,
                                                                             iterations=3 if fix else 20)
    iso = make(120, K=10)
    keep = (iso["ei"] != 4) & (iso["ej"] != 4)
    iso["ei"], iso["ej"], iso["eloop"], iso["graph"] = iso["ei"][keep], iso["ej"][keep], iso["eloop"][keep], None
    out["kf_without_edge"] = iso
    nf = make(131, K=8, iterations=4)
    nf["fixed"] = np.zeros(8, U8)
    out["no_fixed_kf"] = nf
    dup = make(122, K=9)
    dup["ei"], dup["ej"] = np.append(dup["ei"], [5, 4]).astype(I32), np.append(dup["ej"], [4, 5]).astype(I32)
    dup["eloop"], dup["graph"] = np.append(dup["eloop"], [1, 0]).astype(U8), None
    out["duplicate_pair"] = dup
    ff = make(123, K=9, iterations=3)
    ff["fixed"][1] = 1
    out["fixed_fixed_edge"] = ff
    out["log_branches"] = _log_branches()
    nan = make(124, K=8, iterations=5)
    nan["Scw"][4, 4] = 1e300
    out["nan_estimate"] = nan
    return out


def reference(s, jitter=None, solver="ldlt"):
    r = er.optimize(s["Scw"], s["nonc"], s["has"], s["fixed"], s["ei"], s["ej"], s["eloop"], s["fix_scale"], s["iterations"],
                    jitter, solver)
    pos = np.asarray(s["store_pos"], F32)[s["slots"]]
    r["world_pos"] = er.correct_points(s["Scw"], r["kf_Scw"], s["point_ref"], pos) if r["ran"] else pos.copy()
    return r


@functools.lru_cache(maxsize=None)
def references():
    """name -> the restatement's result, computed once for all tests."""
    return {name: reference(s) for name, s in scenes().items()}


@functools.lru_cache(maxsize=None)
def perturbed_references():
    """name -> the restatement's results under the N_PERT members of the perturbation set."""
    return {name: [reference(s, er.Jitter(5000 + 10 * k + m), "numpy" if m % 2 else "ldlt") for m in range(N_PERT)]
            for k, (name, s) in enumerate(scenes().items())}


def decisions(r):
    return (r["ran"], tuple(bool(a) for a in r["accepted"]), r["stop_reason"], r["iterations_run"], r["trials_run"])


def deviations(a, b):
    """Largest differences between two results: q, t, pos absolute, s and chi2 relative (chi2 to max(|chi2|, 1)).  Entries
    that are not finite on both sides are skipped."""
    def amax(x, y, rel=None):
        x, y = np.asarray(x, F64), np.asarray(y, F64)
        with np.errstate(all="ignore"):
            d = np.abs(x - y)
            if rel is not None:
                d = d / np.maximum(np.maximum(np.abs(x), np.abs(y)), rel)
        d = d[np.isfinite(d)]
        return float(d.max()) if d.size else 0.0
    A, B = np.asarray(a["kf_Scw"]), np.asarray(b["kf_Scw"])
    return dict(q=amax(A[:, :4], B[:, :4]), t=amax(A[:, 4:7], B[:, 4:7]), s=amax(A[:, 7], B[:, 7], 1e-300),
                pos=amax(a["world_pos"], b["world_pos"]), chi2_rel=amax(a["chi2"], b["chi2"], 1.0))


def measure():
    spread, worst = {k: 0.0 for k in SPREAD}, {k: None for k in SPREAD}
    for name, ref in references().items():
        for p in perturbed_references()[name]:
            if decisions(p) != decisions(ref):
                continue  # test_eg_reference.py asserts there is none
            for k, v in deviations(ref, p).items():
                if v > spread[k]:
                    spread[k], worst[k] = v, name
    return spread, worst


if __name__ == "__main__" and "--measure" in sys.argv:
    sp, worst = measure()
    # never below one rounding of the quantity itself (unit-size doubles; a float position of size 8)
    floor = dict(q=2.0 ** -52, t=2.0 ** -52, s=2.0 ** -52, chi2_rel=2.0 ** -52, pos=2.0 ** -21)
    sp = {k: max(v, floor[k]) for k, v in sp.items()}
    print("SPREAD = dict(q=%r, t=%r, s=%r, pos=%r, chi2_rel=%r)" % (sp["q"], sp["t"], sp["s"], sp["pos"], sp["chi2_rel"]))
    print("# worst scenes:", worst)
    for name, r in references().items():
        print("#", name, decisions(r), "min_d_dist %.3g min_sigma_dist %.3g" % (r["min_d_dist"], r["min_sigma_dist"]))
