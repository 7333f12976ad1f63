"""Seeded scenes for the tests of vsg_mappoints_local_bundle_adjustment_sgraph (tests/test_sgba_*.py,
tests/test_gpu_sgraph_local_ba.py): the scenes of lba_scenes.make with planes and rooms in `sem`.

The planes are the walls, the ground and the ceiling of a room that is turned against the world axes (25 degrees of yaw,
12 of pitch, 8 of roll: no normal lies on atan2's seam or at elevation +-pi/2, in the world or in a keyframe), 2 to 6 m from
the keyframes, their normals towards the keyframes (d > 0: isDistanceCorrect holds); scenes that need more planes add
oblique ones under the same two conditions.  An observation is the plane in the keyframe's frame -- the keyframe's pose as
the VISUAL restatement leaves it, the nearest thing to the truth that lba_scenes keeps -- with 0.2 degrees / 3 mm of
noise, and Gij summed from 50 to 300 points on the observed plane with 3 mm of noise along its normal.  The planes start
1 cm / 0.5 degrees off.  Weights are confidence (0.5 to 1) times the gains of config/common_system_params.yaml (plane_kf
0.5, plane_point 0.3).  Directed scenes follow; tests/test_sgba_reference.py asserts each one's condition on the restatement.

SPREAD / TOL are MEASURED by the project's rule (python tests/sgba_scenes.py --measure): the largest deviation of the
restatement from itself over a perturbation set -- N_PERM = 8 random orders of the visual AND of the semantic edges, and
the +-1-ulp libm of eg_reference (a numeric Jacobian divides a difference of two roundings by 2e-9, so the libm's last bit
is amplified where an edge order is not) -- per quantity over all scenes, times 64 as in lba_scenes: the measured spreads
stay small enough (below) that the essential graph's 16 x at shortened scenes is not needed.  The floors are lba_scenes'.
The code under test takes no part in the measurement.
"""
import functools
import math
import sys

import numpy as np

import lba_reference as lr
import lba_scenes as ls
import sgba_reference as sr
from pose_scenes import _rot

F32, I32, U8, F64 = np.float32, np.int32, np.uint8, np.float64
N_PERM = 8
GAIN_KF, GAIN_PP = 0.5, 0.3

# measured (see the module docstring), and 64 x that
SPREAD = dict(q=8.084427441726327e-09, t=1.1742303727968473e-07, pos_rel=1.792419053235294e-07, chi2_rel=6.015757840286915e-05,
              plane=1.3601954264585991e-06, room=7.714693202043321e-07, chi2_sem_rel=0.00015666603607571782)
TOL = {k: 64 * v for k, v in SPREAD.items()}
# the same measurement over big_scenes() ALONE (two iterations each: at four, the weakly held keyframes of the larger scenes
# spread ten times as far)
SPREAD_BIG = dict(q=1.2379257403102167e-07, t=8.734690483125362e-07, pos_rel=3.183401489959233e-07, chi2_rel=0.0006591894210778597,
                  plane=2.392719877675198e-06, room=5.5724517916688754e-08, chi2_sem_rel=0.0003223236589942076)
TOL_BIG = {k: 64 * v for k, v in SPREAD_BIG.items()}

ROOM_R = _rot(np.array([0.0, math.radians(25), 0.0])) @ _rot(np.array([math.radians(12), 0.0, 0.0])) @ _rot(np.array([0.0, 0.0, math.radians(8)]))
# inward normals of the room's six faces in room axes, and their distances from the origin
FACES = [((-1, 0, 0), 3.0), ((1, 0, 0), 4.0), ((0, 0, -1), 5.5), ((0, 0, 1), 2.5), ((0, -1, 0), 2.0), ((0, 1, 0), 2.2)]


def face(i):
    n, d = FACES[i]
    return np.concatenate([ROOM_R @ np.array(n, F64), [d]])


def safe_normal(n):
    """Neither near atan2's seam (x < 0, y = 0) nor near the poles (x = y = 0)."""
    h = math.hypot(n[0], n[1])
    return h > 0.25 and not (n[0] < 0 and abs(n[1]) / h < 0.15)


def oblique(rng):
    while True:
        n = rng.normal(0, 1, 3)
        n /= np.linalg.norm(n)
        if safe_normal(n) and safe_normal(-n):
            return np.concatenate([n, [rng.uniform(2.0, 6.0)]])


def est_of(T):
    return (np.asarray(T[:4], F64), np.asarray(T[4:], F64))


def observation(rng, pose7, plane, shift=0.0):
    """-> (localPlane (4), Gij (4, 4)) of `plane` seen from a keyframe; shift moves the observed POINTS along the normal."""
    local = sr.plane_transform(est_of(pose7), plane)
    n, d = local[:3], local[3]
    a = np.cross(n, [0.3, 0.5, 0.8])
    a /= np.linalg.norm(a)
    b = np.cross(n, a)
    N = int(rng.integers(50, 301))
    uv = rng.uniform(-1.0, 1.0, (N, 2))
    pts = -d * n + uv[:, :1] * a + uv[:, 1:] * b + (rng.normal(0, 0.003, (N, 1)) + shift) * n
    ph = np.concatenate([pts, np.ones((N, 1))], 1)
    G = ph.T @ ph
    axis = rng.normal(0, 1, 3)
    axis /= np.linalg.norm(axis)
    noisy = np.concatenate([_rot(axis * math.radians(0.2)) @ n, [d + rng.normal(0, 0.003)]])
    return noisy, G


def start_plane(rng, plane):
    axis = rng.normal(0, 1, 3)
    axis /= np.linalg.norm(axis)
    return np.concatenate([_rot(axis * math.radians(0.5)) @ plane[:3], [plane[3] + 0.01 * (1 if rng.random() < 0.5 else -1)]])


@functools.lru_cache(maxsize=None)
def _visual(key):
    """A visual scene and its keyframes' poses as the visual restatement leaves them."""
    s = ls.make(*key[0], **dict(key[1]))
    ref = lr.local_ba(s)
    return s, (ref["kf_out"] if ref["ran"] else np.asarray(s["Tcw"], F64))


def make(seed, visual, planes, seen, kf=True, pp=True, rooms=(), shift=None, d_off=None, start=True, iterations=4):
    """visual = (args, kwargs) of lba_scenes.make; planes = list of (4,) true planes; seen[i] = the keyframes that observe
    plane i; kf / pp = whether the two factors are enabled; rooms = list of wall index tuples (2 or 4); shift / d_off =
    {(plane, keyframe): metres} moving the observed points / the observed localPlane's distance."""
    s, poses = _visual((tuple(visual[0]), tuple(sorted(visual[1].items()))))
    s = dict(s)
    if iterations is not None:
        s["iterations"] = iterations
    rng = np.random.default_rng(seed)
    off, okf, loc, G, wk, wp = [0], [], [], [], [], []
    for i, pl in enumerate(planes):
        for k in seen[i]:
            l, g = observation(rng, poses[k], pl, (shift or {}).get((i, k), 0.0))
            l[3] += (d_off or {}).get((i, k), 0.0)
            conf = rng.uniform(0.5, 1.0)
            okf.append(k), loc.append(l), G.append(g), wk.append(conf * GAIN_KF if kf else 0.0), wp.append(conf * GAIN_PP if pp else 0.0)
        off.append(len(okf))
    eq = np.array([start_plane(rng, p) if start else p for p in planes], F64).reshape(-1, 4)
    centers, nw, walls = [], [], []
    for r in rooms:
        c = room_center([planes[w] for w in r])
        centers.append(c + rng.normal(0, 0.02, 3)), nw.append(len(r)), walls.append(list(r) + [0] * (4 - len(r)))
    s["sem"] = dict(plane_eq=eq, pl_obs_off=np.array(off, I32), pl_obs_kf=np.array(okf, I32), pl_obs_local=np.array(loc, F64).reshape(-1, 4),
                    pl_obs_G=np.array(G, F64).reshape(-1, 4, 4), w_plane_kf=np.array(wk, F64), w_plane_point=np.array(wp, F64),
                    room_center=np.array(centers, F64).reshape(-1, 3), room_n_walls=np.array(nw, I32),
                    room_wall=np.array(walls, I32).reshape(-1, 4))
    return s


def room_center(walls):
    m = sr.Math()
    c = sr.wall_pair(m, walls[0], walls[1])
    return c + sr.wall_pair(m, walls[2], walls[3]) if len(walls) == 4 else c


def no_sem(s):
    s = dict(s)
    s["sem"] = dict(plane_eq=np.zeros((0, 4)), pl_obs_off=np.zeros(1, I32), pl_obs_kf=np.zeros(0, I32), pl_obs_local=np.zeros((0, 4)),
                    pl_obs_G=np.zeros((0, 4, 4)), w_plane_kf=np.zeros(0), w_plane_point=np.zeros(0), room_center=np.zeros((0, 3)),
                    room_n_walls=np.zeros(0, I32), room_wall=np.zeros((0, 4), I32))
    return s


V11 = ((701, 1, 1, 40, 2, "stereo"), {})
V22 = ((702, 2, 2, 40, 3), {})
V32E = ((703, 3, 2, 40, 3), dict(empty_kf=True))  # keyframe 2 of 6 has no visual edge


def pairs(rng, n_planes, n_kf, count):
    """`count` distinct (plane, keyframe) pairs, every plane at least once -> seen lists."""
    allp = [(i, k) for i in range(n_planes) for k in range(n_kf)]
    first = [(i, int(rng.integers(0, n_kf))) for i in range(n_planes)]
    rest = [p for p in allp if p not in first]
    pick = first + [rest[j] for j in rng.permutation(len(rest))[:count - n_planes]]
    return [sorted(k for i, k in pick if i == pl) for pl in range(n_planes)]


@functools.lru_cache(maxsize=None)
def scenes():
    """name -> scene, in a fixed order."""
    out = {}
    W = [face(i) for i in range(6)]
    out["pp_only"] = make(801, V11, [W[0]], [[0, 1]], kf=False)
    out["pk_only"] = make(802, V11, [W[0]], [[0, 1]], pp=False)
    out["both"] = make(803, V11, [W[0]], [[0, 1]])
    # plane 1 is seen by the fixed keyframes alone; plane 2 has no observation and no room: no vertex
    out["fixed_only_plane"] = make(804, V22, [W[0], W[4], W[2]], [[0, 1, 2, 3], [0, 1], []])
    # keyframe 2 (optimised, no visual edge) has plane edges alone
    out["plane_only_kf"] = make(805, V32E, [W[0], W[4]], [[0, 2, 3], [1, 2, 5]])
    out["corridor"] = make(806, V22, [W[0], W[1], W[4]], [[0, 2], [1, 3], [2]], rooms=[(0, 1)])
    out["room4"] = make(807, V22, W[:4], [[0, 2], [1, 3], [2, 3], [0, 1]], rooms=[(0, 1, 2, 3)])
    far = np.concatenate([W[0][:3], [7.0]])  # the next room's far wall, parallel to wall 0
    out["two_rooms_shared_wall"] = make(808, V22, W[:4] + [far], [[0, 2], [1, 3], [2, 3], [0, 1], [2]], rooms=[(0, 1, 2, 3), (0, 4)])
    out["room_unobserved_walls"] = make(809, V22, W[:5], [[], [], [], [], [0, 2, 3]], rooms=[(0, 1, 2, 3)])
    # every side of correctPlaneDirection and of fabs(d1) > fabs(d2): walls nothing observes, signs and sizes mixed
    mixed = [W[0], -W[1], -np.concatenate([W[2][:3], [1.5]]), W[3], -W[5], np.concatenate([W[4][:3], [3.5]])]
    out["room_branches"] = make(810, V22, mixed + [W[4]], [[], [], [], [], [], [], [0, 2]], rooms=[(0, 1, 2, 3), (4, 5), (1, 0)])
    # plane 0 clean; plane 1: its points 0.5 m off in keyframe 2 (the point edge flags, the plane edge does not); plane 2
    # looks away from the keyframes (isDistanceCorrect fails, chi2 small); plane 3: localPlane 8 m off in keyframe 3 (both)
    out["classification"] = make(811, V22, [W[0], W[4], -W[1], W[3]], [[0, 2, 3], [1, 2, 3], [0, 2], [1, 3]],
                                 shift={(1, 2): 0.5, (3, 3): 0.5}, d_off={(3, 3): 8.0})
    out["edges_4"] = make(812, V11, [W[0], W[4]], [[0, 1], [0, 1]], kf=False)
    out["edges_5"] = make(813, V22, [W[0], W[4]], [[0, 1, 2], [0, 3]], kf=False)
    out["iterations_1"] = make(814, V22, W[:4], [[0, 2], [1, 3], [2, 3], [0, 1]], rooms=[(0, 1, 2, 3)], iterations=1)
    # rooms are the only semantic edges, and there is no visual edge: :2277 returns
    s = make(815, V22, W[:2], [[], []], rooms=[(0, 1)])
    s["obs_off"] = np.zeros_like(s["obs_off"])
    out["rooms_only_edges"] = s
    return out


BIG_VISUAL = ((704, 18, 2, 60, 4), dict(iterations=3))
ONE_PLANE = {n: ((705 + n, n - 2, 2, 80, 4), dict(iterations=2)) for n in (63, 64, 65)}
CAP_VISUAL = ((706, 100, 2, 300, 4), dict(iterations=2))


@functools.lru_cache(maxsize=None)
def big_scenes():
    """Sizes that cross launch geometry, and the cap.  Kept apart from scenes() with a spread of their own."""
    out = {}
    rng = np.random.default_rng(820)
    many = [face(i) for i in range(6)] + [oblique(rng) for _ in range(7)]
    for n in (255, 256, 257):  # plane observations: one past kThreads in the chi2 partials, 20 keyframes x 13 planes
        out["obs_%d" % n] = make(821 + n, BIG_VISUAL, many, pairs(np.random.default_rng(830 + n), 13, 20, n), kf=False, iterations=2)
    for n in (63, 64, 65):  # observations of ONE plane
        out["one_plane_%d" % n] = make(840 + n, ONE_PLANE[n], [face(0)], [list(range(n))], kf=False, iterations=2)
    rng = np.random.default_rng(850)
    planes = [face(i) for i in range(6)] + [oblique(rng) for _ in range(48)]
    seen = pairs(np.random.default_rng(851), 54, 102, 108)
    out["rows_768"] = make(852, CAP_VISUAL, planes, seen, rooms=[(0, 1, 2, 3)], iterations=2)  # 100 keyframes + 54 planes + 1 room
    return out


def rows_771():
    """rows_768 with one more plane: VSG_ERR_UNSUPPORTED."""
    rng = np.random.default_rng(850)
    planes = [face(i) for i in range(6)] + [oblique(rng) for _ in range(49)]
    seen = pairs(np.random.default_rng(851), 54, 102, 108) + [[5]]
    return make(852, CAP_VISUAL, planes, seen, rooms=[(0, 1, 2, 3)], iterations=2)


@functools.lru_cache(maxsize=None)
def references(big=False):
    return {name: sr.local_ba_sgraph(s) for name, s in (big_scenes() if big else scenes()).items()}


def n_sem_edges(s):
    q = s["sem"]
    return int((q["w_plane_kf"] > 0).sum() + (q["w_plane_point"] > 0).sum()) + len(q["room_n_walls"])


@functools.lru_cache(maxsize=None)
def perturbed_references(big=False):
    """name -> the restatement under N_PERM random edge orders (visual and semantic), then under the other libm."""
    out = {}
    for k, (name, s) in enumerate((big_scenes() if big else scenes()).items()):
        rng = np.random.default_rng((1950 if big else 1900) + k)
        E, Es = int(s["obs_off"][-1]), n_sem_edges(s)
        out[name] = [sr.local_ba_sgraph(s, rng.permutation(E), rng.permutation(Es)) for _ in range(N_PERM)]
        out[name].append(sr.local_ba_sgraph(s, jit=sr.scalar_jitter(7 + k)))
    return out


def deviations(a, b):
    """lba_scenes.deviations, and: plane coefficients and room centres relative to max(|value|, 1); the semantic chi2
    relative to max(|chi2|, 1e-6)."""
    d = ls.deviations(a, b)
    with np.errstate(all="ignore"):
        for key, name in (("plane_out", "plane"), ("room_out", "room")):
            x, y = np.asarray(a[key], F64), np.asarray(b[key], F64)
            d[name] = float(np.nanmax(np.abs(x - y) / np.maximum(np.maximum(np.abs(x), np.abs(y)), 1.0), initial=0.0))
        dc = 0.0
        for key in ("chi2_pk", "chi2_pp"):
            x, y = np.asarray(a[key], F64), np.asarray(b[key], F64)
            ok = np.isfinite(x) & np.isfinite(y)
            dc = max(dc, float(np.nanmax((np.abs(x - y) / np.maximum(np.maximum(np.abs(x), np.abs(y)), 1e-6))[ok], initial=0.0)))
        d["chi2_sem_rel"] = dc
    return d


def measure(big=False):
    spread = dict.fromkeys(SPREAD, 0.0)
    refs, pert = references(big), perturbed_references(big)
    for name, ref in refs.items():
        for p in pert[name]:
            for k, v in deviations(ref, p).items():
                spread[k] = max(spread[k], v)
    return spread


if __name__ == "__main__" and "--measure" in sys.argv:
    floor = dict(q=2.0 ** -52, t=2.0 ** -52, pos_rel=2.0 ** -23, chi2_rel=2.0 ** -52, plane=2.0 ** -52, room=2.0 ** -52, chi2_sem_rel=2.0 ** -52)
    for name, big in (("SPREAD", False), ("SPREAD_BIG", True)):
        if big and "--small" in sys.argv:
            continue
        sp = {k: max(v, floor[k]) for k, v in measure(big).items()}
        print("%s = dict(%s)" % (name, ", ".join("%s=%r" % kv for kv in sp.items())))
