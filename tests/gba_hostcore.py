"""The host build of csrc/vsg_global_ba.h (tests/_gbacore) through ctypes: what the global-BA tests compare the restatement
and the device against.  run(scene) returns the fields of gba_reference.global_ba plus the return code, `res` bytes and the
store's positions after the call; every out starts as a sentinel so that "nothing written" is visible.  solve() runs the two
host forms of the reduced solve, geometry() returns the solver's constants."""
import ctypes as C
import functools
import subprocess
from pathlib import Path

import numpy as np

from lba_hostcore import BaCamera, PoseSE3, PoseSE3d, _p, marshal as lba_marshal  # noqa: F401  (the shared layouts)

F32, I32, U8 = np.float32, np.int32, np.uint8
DIR = Path(__file__).resolve().parent / "_gbacore"
SENTINEL_F, SENTINEL_INCLUDED = -7.0, 9

RES_INTS = ("ran", "n_opt_kf", "n_fixed_kf", "n_points", "n_edges", "n_mono", "n_stereo", "iterations_run", "trials_run",
            "stop_reason")
RES_DOUBLES = ("lambda", "chi2_initial", "chi2_final")


class GlobalBaResult(C.Structure):  # vsg_global_ba_result
    _fields_ = [(k, C.c_int32) for k in RES_INTS] + [(k, C.c_double) for k in RES_DOUBLES]


@functools.lru_cache(maxsize=None)
def lib():
    subprocess.check_call(["make", "-C", str(DIR)], stdout=subprocess.DEVNULL)
    L = C.CDLL(str(DIR / "libvsg_gbacore.so"))
    vp = C.c_void_p
    L.gbacore_run.restype = C.c_int
    L.gbacore_run.argtypes = [C.c_int, vp, C.c_int, vp, vp, vp, vp, C.c_int] + [vp] * 10 + [C.c_int] * 4 + [vp] * 6
    L.gbacore_solve.restype = C.c_int
    L.gbacore_solve.argtypes = [C.c_int, C.c_int, vp, vp, vp]
    L.gbacore_stop_after.restype = None
    L.gbacore_stop_after.argtypes = [C.c_int]
    L.gbacore_geometry.restype = None
    L.gbacore_geometry.argtypes = [vp, vp, vp]
    return L


def geometry():
    """-> (columns per panel, rows per tile, the cap on optimised keyframes)."""
    v = np.zeros(3, I32)
    lib().gbacore_geometry(v[0:].ctypes.data, v[1:].ctypes.data, v[2:].ctypes.data)
    return int(v[0]), int(v[1]), int(v[2])


def solve(M, b, blocked):
    """-> (ok, x): lba::solve_reduced_host (blocked = False) or gba::solve_reduced_blocked_host on the lower triangle of M."""
    M, b = np.ascontiguousarray(M, np.float64), np.ascontiguousarray(b, np.float64)
    x = np.zeros(len(b), np.float64)
    ok = lib().gbacore_solve(int(bool(blocked)), len(b), _p(M), _p(b), _p(x))
    return ok, x


def marshal(s):
    a = lba_marshal(s)
    a["included"] = np.full(max(a["P"], 1), SENTINEL_INCLUDED, U8)
    return a


def result(rc, res, a, store_pos):
    out = dict(ret=rc, res_bytes=bytes(res), kf_out=a["kf_out"][:a["K"]], pos_out=a["pos_out"][:a["P"]],
               included=a["included"][:a["P"]], chi2=a["chi2"][:a["E"]], store_pos=store_pos)
    out.update({k: int(getattr(res, k)) for k in RES_INTS})
    out.update({k: float(getattr(res, k)) for k in RES_DOUBLES})
    return out


def flat_features(s):
    K = len(s["kfs"])
    kf_off = np.zeros(K + 1, I32)
    kf_off[1:] = np.cumsum([len(f["x"]) for f in s["kfs"]])
    cat = lambda k, t: np.ascontiguousarray(np.concatenate([np.asarray(f[k], t) for f in s["kfs"]]) if K else np.zeros(0, t))
    ur = np.ascontiguousarray(np.concatenate([np.full(len(f["x"]), -1, F32) if f["ur"] is None else np.asarray(f["ur"], F32)
                                              for f in s["kfs"]]) if K else np.zeros(0, F32))
    return kf_off, cat("x", F32), cat("y", F32), cat("octave", I32), ur


def run(s, stop_flag=None, nleft=None, null=(), stop_after=0, **over):
    """One call of the host core on a scene (its robust / write_store / iterations are fields of the scene).  over: fields
    of the scene to replace; null: names of arguments passed as NULL; stop_flag: None or 0 / 1; stop_after = n > 0 (with a
    stop_flag of 0): the flag is set at the look behind iteration n, as a second thread's store landing there."""
    s = dict(s, **over)
    a = marshal(s)
    K = a["K"]
    kf_off, kx, ky, oc, ur = flat_features(s)
    nl = np.ascontiguousarray(np.full(K, -1, I32) if nleft is None else nleft, I32)
    store_pos = np.ascontiguousarray(s["store_pos"], F32).copy()
    flag = None if stop_flag is None else np.array([stop_flag], U8)
    res = GlobalBaResult()
    C.memset(C.addressof(res), 0x5A, C.sizeof(res))
    arg = lambda name, v: None if name in null else v
    lib().gbacore_stop_after(int(stop_after))
    rc = lib().gbacore_run(s["capacity"], _p(store_pos), a["P"], _p(arg("slots", a["slots"])), _p(arg("obs_off", a["off"])),
                           _p(arg("obs_kf", a["kf"])), _p(arg("obs_idx", a["idx"])), K, _p(kf_off), _p(kx), _p(ky), _p(oc), _p(ur),
                           _p(nl), _p(arg("kf_Tcw", a["Tcw"])), _p(arg("kf_fixed", a["fixed"])), _p(arg("kf_cam", a["cam"])),
                           _p(arg("inv_level_sigma2", a["sig"])), s["nlevels"], s["iterations"], int(s["robust"]),
                           int(s["write_store"]), _p(flag), _p(arg("kf_Tcw_out", a["kf_out"])),
                           _p(arg("world_pos_out", a["pos_out"])), _p(arg("included", a["included"])), _p(arg("chi2", a["chi2"])),
                           None if "res" in null else C.addressof(res))
    return result(rc, res, a, store_pos)
