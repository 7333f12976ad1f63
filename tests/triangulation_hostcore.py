"""The host build of csrc/vsg_triangulate.h (tests/_triangulatecore) through ctypes: what the triangulation tests compare the
restatement and the device against."""
import ctypes as C
import functools
import subprocess
from pathlib import Path

import numpy as np

F32, I32, U8 = np.float32, np.int32, np.uint8
DIR = Path(__file__).resolve().parent / "_triangulatecore"
_vp = C.c_void_p


@functools.lru_cache(maxsize=None)
def lib():
    subprocess.check_call(["make", "-C", str(DIR)], stdout=subprocess.DEVNULL)
    L = C.CDLL(str(DIR / "libvsg_triangulatecore.so"))
    L.tc_null_vectors.argtypes = [C.c_int, _vp, _vp]
    L.tc_pairs.argtypes = [C.c_int] + [_vp] * 6
    L.tc_parallax.argtypes = [C.c_int] + [_vp] * 4
    L.tc_normal_and_depth.argtypes = [_vp, _vp, C.c_int, _vp, C.c_int, _vp, _vp, _vp]
    L.tc_args_ok.argtypes = [C.c_int, C.c_int, _vp, _vp, _vp, C.c_int, C.c_int, _vp, C.c_int]
    L.tc_loop.argtypes = [_vp, C.c_int, _vp, _vp, _vp, C.c_int, _vp, _vp, _vp, _vp, C.c_int, _vp, _vp, _vp, C.c_int, _vp, _vp,
                          _vp, _vp]
    return L


def _p(a):
    return None if a is None else a.ctypes.data_as(_vp)


def params_blob(P):
    """A reference params dict (triangulation_reference.params) as the bytes of vsg_triangulation_params."""
    def cam(c):
        return np.concatenate([c["Rcw"].reshape(9), c["tcw"], c["Ow"], [c["fx"], c["fy"], c["cx"], c["cy"], c["mbf"], 0.0]]
                              ).astype(F32).tobytes() + I32(0).tobytes()
    b = cam(P["kf1"]) + cam(P["kf2"]) + np.array([P["ratio_factor"], P["th_far_points"]], F32).tobytes() + \
        np.array([P["inertial"], P["far_points"], P["kf2_first"]], I32).tobytes()
    assert len(b) == lib().tc_params_size() == 196
    return np.frombuffer(b, U8).copy()


def null_vectors(A):
    A = np.ascontiguousarray(A, F32).reshape(-1, 16)
    v = np.zeros((len(A), 4), np.float64)
    lib().tc_null_vectors(len(A), _p(A), _p(v))
    return v


def features(f):
    """List of reference feature dicts -> n x 9 float32 (vsg::TriFeature)."""
    return np.array([[q["x"], q["y"], q["uright"], q["scale_factor"], q["level_sigma2"], q["cos_stereo"], *q["xyz_c"]] for q in f],
                    F32).reshape(-1, 9)


def pairs(P, f1, f2):
    a, b, pb = features(f1), features(f2), params_blob(P)
    n = len(a)
    reason, source, x3d = np.zeros(max(n, 1), U8), np.zeros(max(n, 1), U8), np.zeros((max(n, 1), 3), F32)
    lib().tc_pairs(n, _p(pb), _p(a), _p(b), _p(reason), _p(source), _p(x3d))
    return reason[:n], source[:n], x3d[:n]


def parallax(P, f1, f2):
    """n x {ray1, ray2, cosParallaxRays}."""
    a, b, pb = features(f1), features(f2), params_blob(P)
    out = np.zeros((max(len(a), 1), 7), F32)
    lib().tc_parallax(len(a), _p(pb), _p(a), _p(b), _p(out))
    return out[:len(a)]


def normal_and_depth(P, x3D, octave1, scale_factors1, nlevels):
    pb, x, sf = params_blob(P), np.ascontiguousarray(x3D, F32), np.ascontiguousarray(scale_factors1, F32)
    nrm, mn, mx = np.zeros(3, F32), np.zeros(1, F32), np.zeros(1, F32)
    lib().tc_normal_and_depth(_p(pb), _p(x), int(octave1), _p(sf), int(nlevels), _p(nrm), _p(mn), _p(mx))
    return nrm, mn[0], mx[0]


def args_ok(n1, n2, matches12, octave1, octave2, nlevels, capacity=0, free_slots=None):
    m, o1, o2 = (np.ascontiguousarray(a, I32) for a in (matches12, octave1, octave2))
    fs = np.ascontiguousarray(free_slots if free_slots is not None else [], I32)
    return bool(lib().tc_args_ok(n1, n2, _p(m) if len(m) else None, _p(o1), _p(o2), nlevels, capacity, _p(fs) if len(fs) else None,
                                 len(fs)))


def _frame(s, t):
    """Frame t ("1" / "2") of a scene as tc_loop takes it; returns (pointer table, octave, desc, arrays kept alive)."""
    k = s["k" + t]
    ur, st = s.get("ur" + t), s.get("stereo" + t)
    arr = [np.ascontiguousarray(k["x"], F32), np.ascontiguousarray(k["y"], F32), None if ur is None else np.ascontiguousarray(ur, F32),
           None if st is None else np.ascontiguousarray(st, F32), np.ascontiguousarray(s["sf" + t], F32),
           np.ascontiguousarray(s["sigma2_" + t], F32)]
    tab = (_vp * 6)(*[None if a is None else a.ctypes.data for a in arr])
    return tab, np.ascontiguousarray(k["octave"], I32), np.ascontiguousarray(s["d" + t], U8), arr


def loop(s, matches12, store=None, free_slots=None):
    """vsg::new_points_loop on a scene (triangulation_scenes).  store: dict of the WHOLE store's arrays (world_pos, normal,
    min_dist, max_dist, desc, observed), copied; None = geometry only.  Returns dict(reason, source, x3d, new_slot, n_created,
    store = the arrays after the loop or None)."""
    n1, n2 = len(s["k1"]), len(s["k2"])
    t1, o1, d1, keep1 = _frame(s, "1")
    t2, o2, d2, keep2 = _frame(s, "2")
    m = np.ascontiguousarray(matches12, I32)
    pb = params_blob(s["P"])
    fs = np.ascontiguousarray(free_slots if free_slots is not None else [], I32)
    after, sf_tab, sb_tab = None, None, None
    if store is not None:
        after = {k: np.array(store[k], copy=True) for k in ("world_pos", "normal", "min_dist", "max_dist", "desc", "observed")}
        sf_tab = (_vp * 4)(*[after[k].ctypes.data for k in ("world_pos", "normal", "min_dist", "max_dist")])
        sb_tab = (_vp * 2)(after["desc"].ctypes.data, after["observed"].ctypes.data)
    n = max(n1, 1)
    out = dict(reason=np.zeros(n, U8), source=np.zeros(n, U8), x3d=np.zeros((n, 3), F32), new_slot=np.zeros(n, I32))
    created = lib().tc_loop(_p(pb), n1, t1, _p(o1), _p(d1), n2, t2, _p(o2), _p(d2), _p(m), s["nlevels"], sf_tab, sb_tab,
                            _p(fs) if len(fs) else None, len(fs), _p(out["reason"]), _p(out["source"]), _p(out["x3d"]),
                            _p(out["new_slot"]))
    return dict({k: v[:n1] for k, v in out.items()}, n_created=created, store=after)
