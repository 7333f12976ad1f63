"""Routine runners and case tables shared by tests/test_gpu_frame_edges.py (HIP against the oracle) and
tests/test_frame_edge_scenarios.py (the oracle alone: every runner takes f = None and then only returns the oracle's
count, so that the floors the GPU tests assert are checked where there is no GPU)."""
import numpy as np

import oracle_lib as ol
import scenarios as sc
from visual_sgraphs_amd import orb

S16, INV16 = sc.SCALE_FACTORS16, sc.INV_SIGMA2_16


def resident(fr, cap=None, gpu=True):
    """(resident frame, oracle frame); gpu = False: (None, oracle frame)"""
    f = None
    if gpu:
        f = orb.Frame(cap or max(len(fr["keys"]), 1)).upload(fr["keys"], fr["desc"], fr["bounds"], fr["u_right"], fr["nleft"])
    return f, sc.oracle_of(fr)


def same(got, ref, what=""):
    """every element of two result tuples equal (scalars, integer arrays); got = a callable that is not run when f is None
    (`got` then is None): returns the oracle's count"""
    if got is None:
        return ref[0]
    assert len(got) >= 2 and len(ref) >= len(got), what
    for i, (g, r) in enumerate(zip(got, ref)):
        assert np.array_equal(np.asarray(g), np.asarray(r)), (what, i)
    return ref[0]


# ---------------------------------------------------------------------------------------------- the routines, by name
def areas(f, o, x, y, r, lo=None, hi=None, right=False):
    """GetFeaturesInArea in both forms against the oracle, list by list (order included); returns the list lengths"""
    if f is not None:
        off, idx = f.GetFeaturesInArea(x, y, r, bRight=right)
    lens = []
    for i in range(len(x)):
        ref = o.features_in_area(x[i], y[i], r[i], right=right, kf_form=True)
        assert f is None or np.array_equal(idx[off[i]:off[i + 1]], ref), ("kf", i)
        lens.append(len(ref))
    if lo is not None and f is not None:
        off, idx = f.GetFeaturesInArea(x, y, r, lo, hi, bRight=right)
        for i in range(len(x)):
            assert np.array_equal(idx[off[i]:off[i + 1]], o.features_in_area(x[i], y[i], r[i], lo[i], hi[i], right)), ("f", i)
    return lens


def local_points(fr, q, qr=None, seed=0):
    """map points of SearchByProjection(F, vpMapPoints, th) from a query set (qr: the right-camera projections)"""
    n = len(q["u"])
    rng = np.random.default_rng(900 + seed)
    mp = dict(desc=q["q_desc"], observed=q["observed"], in_view=q["in_view"], proj_x=q["u"], proj_y=q["v"], proj_xr=q["ur"],
              scale_level=np.maximum(q["level"], 0), view_cos=q["view_cos"])
    ltr = rtl = None
    if fr["nleft"] != -1:
        lvl_r = np.maximum(qr["level"], 0)
        lvl_r[rng.random(n) < 0.05] = -1
        mp.update(in_view_r=qr["in_view"], proj_x_r=qr["u"], proj_y_r=qr["v"], scale_level_r=lvl_r, view_cos_r=qr["view_cos"])
        nl, nr = fr["nleft"], len(fr["keys"]) - fr["nleft"]
        ltr, rtl = np.full(nl, -1, np.int32), np.full(nr, -1, np.int32)
        m = min(nl, nr) // 3
        if m:
            a, b = rng.choice(nl, m, replace=False), rng.choice(nr, m, replace=False)
            ltr[a], rtl[b] = b, a
    blocked = (rng.random(len(fr["keys"])) < 0.1).astype(np.uint8)
    return mp, blocked, ltr, rtl


def run_local(f, o, fr, q, qr=None, th=3.0):
    mp, blocked, ltr, rtl = local_points(fr, q, qr)
    a = (mp, th, 0.8, S16, blocked, ltr, rtl)
    return same(f.SearchByProjection(*a) if f is not None else None, o.search_by_projection(*a), "local")


def run_last(f, o, fr, q, qr=None, th=7.0, direction=0):
    blocked = (np.random.default_rng(901).random(len(fr["keys"])) < 0.1).astype(np.uint8)
    total = 0
    for ori in (True, False):
        a = (q["q_desc"], q["observed"], q["u"], q["v"], q["ur"], np.maximum(q["level"], 0), q["angle"], th, direction, S16,
             ori, blocked)
        kw = dict(u_r=qr["u"], v_r=qr["v"]) if fr["nleft"] != -1 else {}
        total += same(f.SearchByProjection_Last(*a, **kw) if f is not None else None, o.search_by_projection_last(*a, **kw), "last")
    return total


def run_sim3(f, o, fr, q, ratio=1.0):
    matched = np.full(len(fr["keys"]), -1, np.int32)
    matched[np.random.default_rng(902).random(len(matched)) < 0.15] = 12345
    a = (q["q_desc"], q["u"], q["v"], q["radius"], q["level"], ratio, matched)
    return same(f.SearchByProjection_Sim3(*a) if f is not None else None, o.search_by_projection_sim3(*a), "sim3")


def run_kf(f, o, fr, q, orb_dist=100):
    occ = (np.random.default_rng(903).random(len(fr["keys"])) < 0.15).astype(np.uint8)
    a = (q["q_desc"], q["u"], q["v"], q["radius"], q["level"], q["angle"], orb_dist, True, occ)
    return same(f.SearchByProjection_KF(*a) if f is not None else None, o.search_by_projection_kf(*a), "kf")


def run_by_sim3(f, o, fr, q):
    """both directions on the same KeyFrame pair (f, f): a point agrees when its best candidate's best candidate is it"""
    d = dict(idx=q["src"], desc=q["q_desc"], u=q["u"], v=q["v"], radius=q["radius"], level=q["level"])
    e = dict(d, desc=fr["desc"][q["src"]])
    return same(orb.SearchBySim3(f, f, d, e) if f is not None else None, ol.search_by_sim3(o, o, d, e), "by_sim3")


def run_fuse(f, o, fr, q, right=False):
    nq, nk = len(q["u"]), len(fr["keys"])
    z = np.zeros(nq + nk, np.int32)
    got = f.Fuse(q["q_desc"], q["u"], q["v"], q["ur"], q["radius"], q["level"], INV16, right=right) if f is not None else None
    ref = o.fuse(np.arange(nq), q["q_desc"], q["u"], q["v"], q["ur"], q["radius"], q["level"], INV16,
                 np.full(nk, -1, np.int32), z, z.astype(np.uint8), right=right)
    return same(got, ref[:3], "fuse")


def run_fuse_sim3(f, o, fr, q):
    nq, nk = len(q["u"]), len(fr["keys"])
    z = np.zeros(nq + nk, np.int32)
    got = f.Fuse_Sim3(q["q_desc"], q["u"], q["v"], q["radius"], q["level"]) if f is not None else None
    ref = o.fuse_sim3(np.arange(nq), q["q_desc"], q["u"], q["v"], q["radius"], q["level"], np.full(nk, -1, np.int32), z,
                      z.astype(np.uint8))
    return same(got, ref[:3], "fuse_sim3")


def run_init(f, o, fr, window=30):
    """F1 = F2 = the frame, vbPrevMatched = its own keypoints moved by (2, -1)"""
    px, py = (fr["keys"]["x"] + np.float32(2)).astype(np.float32), (fr["keys"]["y"] - np.float32(1)).astype(np.float32)
    total = 0
    for ori in (True, False):
        total += same(f.SearchForInitialization(f, px, py, window, 0.9, ori) if f is not None else None,
                      o.search_for_initialization(o, px, py, window, 0.9, ori), "init")
    return total


def levels_of(q):
    return (q["level"] - 1).astype(np.int32), (q["level"] + 1).astype(np.int32)


# floors: the largest round numbers below the oracle's own counts on the CPU, asserted there as well
# (local 111, last 217, sim3 72, kf 37, by_sim3 88, fuse 64, fuse_no_ur 84, fuse_sim3 88, init 404)
DENSE_FLOORS = {"local": 110, "last": 210, "sim3": 70, "kf": 30, "by_sim3": 80, "fuse": 60, "fuse_no_ur": 80, "fuse_sim3": 80,
                "init": 400}
# the fisheye-stereo frame: right Fuse 103, left Fuse 99, local 165, last 255
DENSE_RIGHT_FLOORS = {"fuse_right": 100, "fuse_left": 90, "local": 160, "last": 250}

GEOMETRIES = [(640, 480, 1000), (752, 480, 1200), (1280, 720, 2000)]
# floors: the largest round number below the oracle's own count on the CPU over the three cameras (seed 1)
PRODUCTION_FLOORS = {
    # oracle: local 346-348, last 660-661, sim3 456-457, kf 643-646, by_sim3 244-245, fuse 294-296, fuse_sim3 520, init 109
    (640, 480, 1000): dict(local=340, last=660, sim3=450, kf=640, by_sim3=240, fuse=290, fuse_sim3=510, init=100),
    # oracle: 408-410, 795-796, 501, 782-785, 295, 305-307, 567, 107; stereo forms 1020-1022, 1759-1765, right Fuse 478-480
    (752, 480, 1200): dict(local=400, last=790, sim3=500, kf=780, by_sim3=290, fuse=300, fuse_sim3=560, init=100,
                           local_stereo=1000, last_stereo=1700, fuse_right=470),
    # oracle: 930-931, 1067-1069, 839-841, 1242-1245, 473, 506-507, 967-969, 186
    (1280, 720, 2000): dict(local=920, last=1060, sim3=830, kf=1240, by_sim3=470, fuse=500, fuse_sim3=960, init=180),
}


def production_counts(gpu, geom, seed=1):
    """The routine tests of tests/test_gpu_frame.py at a production geometry under the current camera.
    gpu: compare the resident frames' results with the oracle's; otherwise the oracle alone.  Returns {name: the oracle's count}."""
    w, h, nf = geom
    out = {}

    def frame(keys, desc, u_right=None, nleft=-1):
        o = ol.OracleFrame(keys, desc, sc.BOUNDS, u_right, nleft)
        return (orb.Frame(max(len(keys), 1)).upload(keys, desc, sc.BOUNDS, u_right, nleft) if gpu else None), o

    def both(name, g, o_):
        if gpu:
            same(g(), o_(), name)
        out[name] = o_()[0]
    stereo_forms = (False, True) if geom == GEOMETRIES[1] else (False,)
    for st in stereo_forms:
        s = sc.local_map_scenario(seed, st, w, h, nf)
        f, o = frame(s["keys"], s["desc"], s["u_right"], s["nleft"])
        a = (s["mp"], s["th"], s["nnratio"], sc.SCALE_FACTORS, s["blocked"], s["ltr"], s["rtl"])
        both("local_stereo" if st else "local", lambda: f.SearchByProjection(*a), lambda: o.search_by_projection(*a))
        s = sc.last_frame_scenario(seed, st, w, h, nf)
        f, o = frame(s["keys"], s["desc"], s["u_right"], s["nleft"])
        a = (s["q_desc"], s["observed"], s["u"], s["v"], s["ur"], s["octave"], s["angle"], s["th"], s["direction"],
             sc.SCALE_FACTORS, True, s["blocked"])
        kw = dict(u_r=s["u_r"], v_r=s["v_r"])
        both("last_stereo" if st else "last", lambda: f.SearchByProjection_Last(*a, **kw),
             lambda: o.search_by_projection_last(*a, **kw))
    s = sc.kf_projection_scenario(seed, w, h, nf)
    f, o = frame(s["keys"], s["desc"], s["u_right"])
    nq, nk = len(s["u"]), len(s["keys"])
    m0 = np.full(nk, -1, np.int32)
    a = (s["q_desc"], s["u"], s["v"], s["radius"], s["level"], 1.0, m0)
    both("sim3", lambda: f.SearchByProjection_Sim3(*a), lambda: o.search_by_projection_sim3(*a))
    a2 = (s["q_desc"], s["u"], s["v"], s["radius"], s["level"], s["angle"], 100, True, np.zeros(nk, np.uint8))
    both("kf", lambda: f.SearchByProjection_KF(*a2), lambda: o.search_by_projection_kf(*a2))
    z = np.zeros(nq + nk, np.int32)
    slot = np.full(nk, -1, np.int32)
    both("fuse", lambda: f.Fuse(s["q_desc"], s["u"], s["v"], s["ur"], s["radius"], s["level"], sc.INV_SIGMA2),
         lambda: o.fuse(np.arange(nq), s["q_desc"], s["u"], s["v"], s["ur"], s["radius"], s["level"], sc.INV_SIGMA2, slot, z,
                        z.astype(np.uint8))[:3])
    both("fuse_sim3", lambda: f.Fuse_Sim3(s["q_desc"], s["u"], s["v"], s["radius"], s["level"]),
         lambda: o.fuse_sim3(np.arange(nq), s["q_desc"], s["u"], s["v"], s["radius"], s["level"], slot, z,
                             z.astype(np.uint8))[:3])
    if geom == GEOMETRIES[1]:
        keys, desc, nleft = sc.stereo_pair(seed, w, h, nf)
        fs, os_ = frame(keys, desc, None, nleft)
        zs = np.zeros(nq + len(keys), np.int32)
        both("fuse_right",
             lambda: fs.Fuse(s["q_desc"], s["u"], s["v"], s["ur"], s["radius"], s["level"], sc.INV_SIGMA2, right=True),
             lambda: os_.fuse(np.arange(nq), s["q_desc"], s["u"], s["v"], s["ur"], s["radius"], s["level"], sc.INV_SIGMA2,
                              np.full(len(keys), -1, np.int32), zs, zs.astype(np.uint8), right=True)[:3])
    # SearchBySim3 + SearchForInitialization between the two frames of the sequence
    k1, d1 = sc.features(seed, 0, w, h, nf)
    k2, d2 = sc.features(seed, 1, w, h, nf)
    (f1, o1), (f2, o2) = frame(k1, d1), frame(k2, d2)
    rng = np.random.default_rng(seed + 77)

    def direction(src_k, src_d, shift):
        idx = np.sort(rng.choice(len(src_k), int(0.8 * len(src_k)), replace=False)).astype(np.int32)
        u, v = sc.projections(rng, src_k[idx], shift=shift)
        lvl = np.clip(src_k["octave"][idx] + rng.integers(-1, 2, len(idx)), 0, 7).astype(np.int32)
        return dict(idx=idx, desc=sc.noisy_desc(rng, src_d[idx], 6), u=u, v=v,
                    radius=(np.float32(7.5) * sc.SCALE_FACTORS[lvl]).astype(np.float32), level=lvl)
    q1, q2 = direction(k1, d1, (-3.0, -2.0)), direction(k2, d2, (3.0, 2.0))
    both("by_sim3", lambda: orb.SearchBySim3(f1, f2, q1, q2), lambda: ol.search_by_sim3(o1, o2, q1, q2))
    both("init", lambda: f1.SearchForInitialization(f2, k1["x"], k1["y"], 100, 0.9, True),
         lambda: o1.search_for_initialization(o2, k1["x"], k1["y"], 100, 0.9, True))
    return out


def rewrite_uploads():
    """section h: the frames its upload steps (1, 2, 5) write"""
    return {1: sc.synthetic_frame(90, 40, "uniform", ur_share=(0.2, 0.2)),
            2: sc.synthetic_frame(91, 3000, "clustered", nleft=1500, clusters=6),
            5: sc.synthetic_frame(92, 2500, "clustered", ur_share=(0.3, 0.1), bounds=sc.D435I_LIKE)}


SPLIT_N = 1500


def split_case(split):
    """section g: (frame, left queries, right queries) for Nleft in {0, 1, n - 1, n}; with a lone feature on one side, half
    of that side's windows are aimed at it"""
    n = SPLIT_N
    nleft = {"0": 0, "1": 1, "n-1": n - 1, "n": n}[split]
    fr = sc.synthetic_frame(80, n, "clustered", nleft=nleft, clusters=6) if nleft in (0, n) else \
        sc.synthetic_frame(80, n, "uniform", nleft=nleft)
    q, qr = sc.synthetic_queries(81, fr, 150, right=False), sc.synthetic_queries(82, fr, 150, right=True)
    if nleft == 1:
        q["u"][::2], q["v"][::2], q["radius"][::2] = fr["keys"]["x"][0], fr["keys"]["y"][0], 9.0
    if nleft == n - 1:
        qr["u"][::2], qr["v"][::2], qr["radius"][::2] = fr["keys"]["x"][n - 1], fr["keys"]["y"][n - 1], 9.0
    return fr, q, qr


def reach_split(fr, q, qr, ll, lr):
    """ll / lr: the oracle's list lengths of the left / right windows (areas()): a side has lists exactly when it has
    features, and a lone feature is really listed by the windows aimed at it"""
    n, nleft = len(fr["keys"]), fr["nleft"]
    assert (max(ll) > 0) == (nleft > 0) and (max(lr) > 0) == (nleft < n)
    if nleft == 1:
        assert sum(v == 1 for v in ll[::2]) >= 70 and max(ll) == 1
    if nleft == n - 1:
        assert sum(v == 1 for v in lr[::2]) >= 70 and max(lr) == 1
    if nleft in (0, n):
        assert max(ll + lr) > 32   # the populated side is clustered


TAIL_NQ = (1, 2, 3, 4, 5, 7, 8, 9)


def tail_case(nq):
    """section g: the first nq usable queries of the dense case with inactive ones between active ones: in_view == 0 at odd
    positions (list mode), nPredictedLevel < 0 at positions 1, 4, 7 (best mode)"""
    fr, q, _ = sc.dense_case(False)
    on = np.nonzero((q["level"] >= 0))[0][:nq]
    qq = {k: (v[on].copy() if isinstance(v, np.ndarray) else v) for k, v in q.items()}
    qq["in_view"] = (np.arange(nq) % 2 == 0).astype(np.uint8)
    qq["level"][1::3] = -1
    return fr, qq


def reach_tail(fr, qq, lens):
    nq = len(qq["u"])
    assert lens[0] > 0 and qq["in_view"][0] == 1 and qq["level"][0] >= 0   # query 0 is active and lists something
    if nq >= 2:
        assert (qq["in_view"] == 0).any() and (qq["level"] < 0).any()
    if nq >= 3:
        assert qq["in_view"][2] == 1 and qq["level"][2] >= 0               # ... and an active one follows the inactive one


SWEEP_BOUNDS = (sc.HD_BOUNDS, sc.TUM1_LIKE, sc.D435I_LIKE, (0.0, 0.0, 640.0, 480.0), (-3.25, -2.5, 757.5, 484.0))
SWEEP_ROUTINES = ("area", "local", "last", "sim3", "kf", "by_sim3", "fuse", "fuse_sim3", "init")


def sweep_case(seed):
    rng = np.random.default_rng(7000 + seed)
    bounds = SWEEP_BOUNDS[int(rng.integers(0, len(SWEEP_BOUNDS)))]
    n = int(np.exp(rng.uniform(0, np.log(32768.0)))) - 1      # log-uniform in [0, 32767]
    law = ("uniform", "clustered", "lattice", "one_cell")[int(rng.integers(0, 4))]
    if law == "clustered" and n < 1500:
        law = "uniform"
    if law == "one_cell":
        n = min(n, 700)
    stereo = rng.random() < 0.35
    nleft = int(rng.integers(0, n + 1)) if stereo else -1
    if law == "clustered" and stereo:
        nleft = int(np.clip(nleft, 1200, n - 1200)) if n >= 2400 else -1
    ur = (0.3, 0.1) if (nleft == -1 and rng.random() < 0.5) else None
    fr = sc.synthetic_frame(7100 + seed, n, law, bounds=bounds, ur_share=ur, nleft=nleft, clusters=5)
    nq = int(rng.choice([1, 3, 6, 50, 300]))
    rad = [(0.3, 8.0), (2.0, 80.0), (20.0, 3000.0)][int(rng.integers(0, 3))]
    routine = SWEEP_ROUTINES[seed % len(SWEEP_ROUTINES)]
    if nleft != -1 and routine in ("sim3", "kf", "by_sim3", "fuse_sim3", "init"):
        routine = ("area", "local", "last", "fuse")[seed % 4]
    if routine == "by_sim3" and n == 0:   # its query indices name features: none to name
        routine = "sim3"
    if routine == "init" and rad[1] > 100:
        rad = (2.0, 80.0)
    return fr, nq, rad, routine
