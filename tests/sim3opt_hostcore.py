"""The host build of csrc/vsg_sim3_opt.h (tests/_sim3optcore) through ctypes: what the Sim3-optimisation tests compare the
restatement and the device against.  run(scene) returns the fields of sim3opt_reference.optimize_sim3 with state / chi2 as
full per-feature arrays over sentinels (state 9, chi2 -1: chi2 entries without an edge must keep them)."""
import ctypes as C
import functools
import subprocess
from pathlib import Path

import numpy as np

F32, I32, U8 = np.float32, np.int32, np.uint8
DIR = Path(__file__).resolve().parent / "_sim3optcore"
SENTINEL_STATE, SENTINEL_CHI2 = 9, -1.0


class FramePose(C.Structure):  # include/vsg_orb.h vsg_frame_pose
    _fields_ = [("Rcw", C.c_float * 9), ("tcw", C.c_float * 3), ("Ow", C.c_float * 3), ("fx", C.c_float), ("fy", C.c_float),
                ("cx", C.c_float), ("cy", C.c_float), ("mbf", C.c_float), ("log_scale_factor", C.c_float),
                ("n_levels", C.c_int32)]


class Sim3d(C.Structure):  # vsg_sim3d
    _fields_ = [("q", C.c_double * 4), ("t", C.c_double * 3), ("s", C.c_double)]


class Sim3OptResult(C.Structure):  # vsg_sim3_opt_result
    _fields_ = [("S12", Sim3d)] + [(k, C.c_int32) for k in ("n_correspondences", "n_bad", "n_in", "n_in_kf2", "n_out_kf2",
                                                             "more_iterations", "updated")]


COUNTERS = ("n_correspondences", "n_bad", "n_in", "n_in_kf2", "n_out_kf2", "more_iterations", "updated")


@functools.lru_cache(maxsize=None)
def lib():
    subprocess.check_call(["make", "-C", str(DIR)], stdout=subprocess.DEVNULL)
    L = C.CDLL(str(DIR / "libvsg_sim3optcore.so"))
    vp = C.c_void_p
    L.sim3optcore_run.restype = C.c_int
    L.sim3optcore_run.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, C.c_int, C.c_int] + [vp] * 12 + \
        [C.c_int, vp, C.c_float, C.c_int, C.c_int, vp, vp, vp]
    L.sim3optcore_exp.argtypes = [C.c_int, vp, vp]
    L.sim3optcore_exp7.argtypes = [vp, vp]
    L.sim3optcore_mul.argtypes = [vp, vp, vp]
    L.sim3optcore_inverse.argtypes = [vp, vp]
    L.sim3optcore_map.argtypes = [vp, vp, vp]
    L.sim3optcore_oplus.argtypes = [vp, vp, C.c_int, vp]
    return L


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def frame_pose(p, cls=FramePose):
    o = cls()
    o.Rcw[:] = [float(v) for v in np.asarray(p["Rcw"], F32).reshape(9)]
    o.tcw[:] = [float(v) for v in np.asarray(p["tcw"], F32)]
    o.fx, o.fy, o.cx, o.cy = float(p["fx"]), float(p["fy"]), float(p["cx"]), float(p["cy"])
    return o


def sim3d(S, cls=Sim3d):
    o = cls()
    o.q[:], o.t[:], o.s = [float(v) for v in S[0]], [float(v) for v in S[1]], float(S[2])
    return o


def result(ret, res, state, chi2):
    out = dict(ret=ret, state=state, chi2=chi2, S12_bytes=bytes(res.S12),
               S12=(np.array(res.S12.q[:]), np.array(res.S12.t[:]), float(res.S12.s)))
    out.update({k: int(getattr(res, k)) for k in COUNTERS})
    return out


def run(s, first_fresh=False, **over):
    """One call of the host core on a scene; over: fields of the scene to replace.  first_fresh: the test-only variant
    that recomputes the errors at the first check (NOT the reference)."""
    s = dict(s, **over)
    n = s["n1"]
    a = dict(s1=np.ascontiguousarray(s["slots1"], I32), s2=np.ascontiguousarray(s["slots2"], I32),
             i2=np.ascontiguousarray(s["idx2"], I32), l2=np.ascontiguousarray(s["level2"], I32),
             p1=np.ascontiguousarray(s["pos1"], F32), p2=np.ascontiguousarray(s["pos2"], F32),
             k1x=np.ascontiguousarray(s["kps1"]["x"], F32), k1y=np.ascontiguousarray(s["kps1"]["y"], F32),
             o1=np.ascontiguousarray(s["kps1"]["octave"], I32), k2x=np.ascontiguousarray(s["kps2"]["x"], F32),
             k2y=np.ascontiguousarray(s["kps2"]["y"], F32), o2=np.ascontiguousarray(s["kps2"]["octave"], I32),
             g1=np.ascontiguousarray(s["sig1"], F32), g2=np.ascontiguousarray(s["sig2"], F32))
    state, chi2 = np.full(max(n, 1), SENTINEL_STATE, U8), np.full(2 * max(n, 1), SENTINEL_CHI2, np.float64)
    pose1, pose2, S12, res = frame_pose(s["pose1"]), frame_pose(s["pose2"]), sim3d(s["S12"]), Sim3OptResult()
    rc = lib().sim3optcore_run(n, s["n2"], _p(a["s1"]), _p(a["s2"]), _p(a["i2"]), _p(a["l2"]), s["cap1"], s["cap2"], _p(a["p1"]),
                               _p(a["p2"]), _p(a["k1x"]), _p(a["k1y"]), _p(a["o1"]), _p(a["k2x"]), _p(a["k2y"]), _p(a["o2"]),
                               C.addressof(pose1), C.addressof(pose2), _p(a["g1"]), _p(a["g2"]), s["nlevels"],
                               C.addressof(S12), float(s["th2"]), int(s["fix_scale"]) | (2 if first_fresh else 0), s["all_points"], _p(state), _p(chi2),
                               C.addressof(res))
    out = result(rc, res, state[:n], chi2[:2 * n].reshape(n, 2))
    out["input_bytes"] = bytes(S12)
    return out


def exp(x):
    x = np.ascontiguousarray(x, np.float64)
    y = np.zeros_like(x)
    lib().sim3optcore_exp(len(x), _p(x), _p(y))
    return y


def _s8(S):
    return np.concatenate([S[0], S[1], [S[2]]]).astype(np.float64)


def _s3(a):
    return a[:4].copy(), a[4:7].copy(), float(a[7])


def sim3_exp(u):
    u, o = np.ascontiguousarray(u, np.float64), np.zeros(8)
    lib().sim3optcore_exp7(_p(u), _p(o))
    return _s3(o)


def sim3_mul(a, b):
    a, b, o = _s8(a), _s8(b), np.zeros(8)
    lib().sim3optcore_mul(_p(a), _p(b), _p(o))
    return _s3(o)


def sim3_inverse(a):
    a, o = _s8(a), np.zeros(8)
    lib().sim3optcore_inverse(_p(a), _p(o))
    return _s3(o)


def sim3_map(a, x):
    a, x, o = _s8(a), np.ascontiguousarray(x, np.float64), np.zeros(3)
    lib().sim3optcore_map(_p(a), _p(x), _p(o))
    return o


def oplus(S, update, fix_scale):
    """-> (the new estimate, the update array as oplusImpl left it)."""
    a, u, o = _s8(S), np.array(update, np.float64), np.zeros(8)
    lib().sim3optcore_oplus(_p(a), _p(u), int(fix_scale), _p(o))
    return _s3(o), u
