"""Seeded scenes for the global-BA tests (tests/test_gba_*.py, tests/test_gpu_global_bundle_adjustment.py), built on
lba_scenes.make: the same cameras, points, noise and outliers, with the three arguments the global call adds as fields of
the scene (robust, write_store, iterations) and ONE fixed keyframe (the map's initial keyframe) unless a scene says otherwise.

Sizes are the smallest at which the new code can go wrong.  PANEL = 48 and TILE = 64 are the reduced solve's constants
(test_gba_hostmath.py asserts that they are the ones in force):
  * 1 optimised + 1 fixed keyframe, mono only, robust, 20 iterations: the shape of CreateInitialMapMonocular;
  * no fixed keyframe at all, stereo edges;
  * 7 / 8 / 9 optimised keyframes: 42 / 48 / 54 rows, just under, at and just over one panel;
  * 25 optimised keyframes: 150 = 3 PANEL + 6 rows, three panels and a ragged one;
  * 19 optimised keyframes: 114 rows, so that the first panel's trailing update has 66 rows: one tile and a ragged remainder;
  * 129 optimised keyframes (774 rows), one past the local call's cap, 400 points each seen by 4 to 6 keyframes (with 60
    points most keyframes have two or three edges and the scene's spread measures 400 times the others' median: the
    conditioning rule below asks for another scene, not a wider tolerance; the host build takes half a second on it);
  * mixed mono and stereo with the kernel on and off, 0 % and 20 % outliers (without the kernel the outliers pull the
    solution: that is the reference's behaviour and the restatement shows it);
  * an optimised keyframe without edges, a point with an empty list, a point seen only by the fixed keyframe, the fixed
    keyframe at the head and in the middle of the array; write_store 0 and 1;
  * directed: negated informations, so that the reduced factorisation meets non-positive pivots and trials are rejected
    with ok2 = false (its cost is negative and ends at DBL_MAX: no convergence is asked of it), and an exact start that
    ends by Terminate (rho == 0, stop_reason 1; its cost is 0 before and after).

SPREAD / TOL below are MEASURED, not chosen, by the rule of lba_scenes.py: the largest deviation of the restatement from
itself over N_PERM random permutations of the edge order, per quantity, over all scenes, and 64 times that.  Where a spread
measures below one rounding of the quantity the floor of one ulp of the compared type is used instead: 2^-52 for the doubles,
2^-23 for the float positions.  Produced by
    python tests/gba_scenes.py --measure
which also prints every scene's own spread; test_gba_reference.py asserts that no scene's is more than 100 times the median
of the others'.
"""
import functools
import sys

import numpy as np

import gba_reference as gr
import lba_scenes as ls

F32, I32, U8 = np.float32, np.int32, np.uint8
N_PERM = 8
PANEL, TILE = 48, 64

# measured (see the module docstring): largest |difference| between edge orders, and 64 x that
# q, t and chi2_rel are measured values.  pos_rel is NOT: the float positions come out identical under every order, so the
# constant is the FLOOR 2^-23 = one ulp of the compared float, a chosen number reasoned from the format.
SPREAD = dict(q=3.8552234321587164e-13, t=4.390932062392494e-12, pos_rel=1.1920928955078125e-07, chi2_rel=2.487251206543656e-09)
TOL = {k: 64 * v for k, v in SPREAD.items()}


def _with(s, robust, write_store, iterations=None):
    s = dict(s, robust=int(robust), write_store=int(write_store))
    if iterations is not None:
        s["iterations"] = iterations
    return s


def _move_fixed(s, at):
    """The scene with its first keyframe (the fixed one) moved to index `at` of the keyframe array."""
    K = len(s["kfs"])
    order = list(range(1, K))
    order.insert(at, 0)  # new index -> old index
    new_of = np.empty(K, np.int64)
    new_of[order] = np.arange(K)
    s = dict(s)
    s["kfs"] = [s["kfs"][o] for o in order]
    s["Tcw"], s["fixed"], s["cam"] = s["Tcw"][order], s["fixed"][order], s["cam"][order]
    s["obs_kf"] = new_of[s["obs_kf"]].astype(I32)
    return s


def _trim(s, seed, lo):
    """Every point keeps between lo and all of its observations (the first ones of its list)."""
    rng = np.random.default_rng(seed)
    off = s["obs_off"]
    keep = np.zeros(int(off[-1]), bool)
    new_off = [0]
    for p in range(len(off) - 1):
        n = int(off[p + 1] - off[p])
        m = int(rng.integers(min(lo, n), n + 1))
        keep[off[p]:off[p] + m] = True
        new_off.append(new_off[-1] + m)
    s = dict(s)
    s["obs_off"] = np.array(new_off, I32)
    s["obs_kf"], s["obs_idx"], s["is_out"] = s["obs_kf"][keep], s["obs_idx"][keep], s["is_out"][keep]
    return s


@functools.lru_cache(maxsize=None)
def scenes():
    """name -> scene, in a fixed order."""
    out = {}
    out["initialisation"] = _with(ls.make(801, 1, 1, 60, 2, "mono"), 1, 1, 20)
    out["no_fixed_stereo"] = _with(ls.make(802, 3, 0, 60, 3, "stereo"), 0, 0)
    for n_opt in (7, 8, 9):
        out["rows_%d" % (6 * n_opt)] = _with(ls.make(803 + n_opt, n_opt, 1, 60, 4), n_opt % 2, n_opt % 2)
    out["rows_150"] = _with(ls.make(821, 25, 1, 120, 5), 0, 0)
    out["rows_114"] = _with(ls.make(822, 19, 1, 100, 5), 1, 1)
    out["kf_129"] = _with(_trim(ls.make(823, 129, 1, 400, 6), 824, 4), 0, 0)
    for robust in (1, 0):
        for pct in (0, 20):
            out["mixed_%s_%d" % ("robust" if robust else "plain", pct)] = _with(
                ls.make(830 + 2 * robust + pct // 20, 3, 1, 80, 4, outliers=pct / 100.0), robust, robust ^ (pct // 20))
    out["special_vertices"] = _with(ls.make(841, 3, 1, 60, 3, empty_kf=True, fixed_only_point=True, empty_point=True), 1, 1)
    out["special_vertices_kept"] = _with(out["special_vertices"], 1, 0)
    out["fixed_in_the_middle"] = _with(_move_fixed(ls.make(842, 4, 1, 60, 3), 2), 0, 1)
    bad = ls.make(503, 3, 1, 80, 4, "stereo")  # non-positive pivots: trials rejected with ok2 = false
    out["bad_pivot"] = _with(dict(bad, sig=(-ls.INV_SIGMA2).astype(F32)), 0, 0)
    out["exact_start"] = _with(ls._exact(), 1, 1)                                                # ends by Terminate
    return out


@functools.lru_cache(maxsize=None)
def references():
    """name -> the restatement's result, computed once for all tests."""
    return {name: gr.global_ba(s) for name, s in scenes().items()}


@functools.lru_cache(maxsize=None)
def permuted_references():
    """name -> the restatement's results under N_PERM random edge orders."""
    out = {}
    for k, (name, s) in enumerate(scenes().items()):
        rng = np.random.default_rng(950 + k)
        out[name] = [gr.global_ba(s, rng.permutation(int(s["obs_off"][-1]))) for _ in range(N_PERM)]
    return out


deviations = ls.deviations
FLOOR = dict(q=2.0 ** -52, t=2.0 ** -52, pos_rel=2.0 ** -23, chi2_rel=2.0 ** -52)


@functools.lru_cache(maxsize=None)
def scene_spreads():
    """name -> the scene's own spread per quantity (not floored)."""
    out = {}
    for name, ref in references().items():
        sp = dict(q=0.0, t=0.0, pos_rel=0.0, chi2_rel=0.0)
        for p in permuted_references()[name]:
            for k, v in deviations(ref, p).items():
                sp[k] = max(sp[k], v)
        out[name] = sp
    return out


def measure():
    return {k: max(max(sp[k] for sp in scene_spreads().values()), FLOOR[k]) for k in FLOOR}


if __name__ == "__main__" and "--measure" in sys.argv:
    for name, sp in scene_spreads().items():
        print("%-24s q=%.3e t=%.3e pos_rel=%.3e chi2_rel=%.3e" % (name, sp["q"], sp["t"], sp["pos_rel"], sp["chi2_rel"]))
    sp = measure()
    print("SPREAD = dict(q=%r, t=%r, pos_rel=%r, chi2_rel=%r)" % (sp["q"], sp["t"], sp["pos_rel"], sp["chi2_rel"]))
