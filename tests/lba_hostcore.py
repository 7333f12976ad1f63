"""The host build of csrc/vsg_local_ba.h (tests/_localbacore) through ctypes: what the local-BA tests compare the
restatement and the device against.  run(scene) returns the fields of lba_reference.local_ba plus the return code, `res`
bytes and the store's positions after the call; every out starts as a sentinel so that "nothing written" is visible."""
import ctypes as C
import functools
import subprocess
from pathlib import Path

import numpy as np

F32, I32, U8 = np.float32, np.int32, np.uint8
DIR = Path(__file__).resolve().parent / "_localbacore"
SENTINEL_F, SENTINEL_ERASE = -7.0, 9


class PoseSE3(C.Structure):  # include/vsg_orb.h vsg_pose_se3
    _fields_ = [("q", C.c_float * 4), ("t", C.c_float * 3)]


class PoseSE3d(C.Structure):  # vsg_pose_se3d
    _fields_ = [("q", C.c_double * 4), ("t", C.c_double * 3)]


class BaCamera(C.Structure):  # vsg_ba_camera
    _fields_ = [(k, C.c_float) for k in ("fx", "fy", "cx", "cy", "bf")]


RES_INTS = ("ran", "n_opt_kf", "n_fixed_kf", "n_points", "n_edges", "n_mono", "n_stereo", "n_erase", "iterations_run",
            "trials_run", "stop_reason")
RES_DOUBLES = ("lambda", "chi2_initial", "chi2_final")


class LocalBaResult(C.Structure):  # vsg_local_ba_result
    _fields_ = [(k, C.c_int32) for k in RES_INTS] + [(k, C.c_double) for k in RES_DOUBLES]


@functools.lru_cache(maxsize=None)
def lib():
    subprocess.check_call(["make", "-C", str(DIR)], stdout=subprocess.DEVNULL)
    L = C.CDLL(str(DIR / "libvsg_localbacore.so"))
    vp = C.c_void_p
    L.lbacore_run.restype = C.c_int
    L.lbacore_run.argtypes = [C.c_int, vp, C.c_int, vp, vp, vp, vp, C.c_int] + [vp] * 10 + [C.c_int, C.c_int] + [vp] * 6
    return L


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def marshal(s):
    """The scene's arrays as the C interfaces take them (contiguous, typed); kept alive by the returned dict."""
    K = len(s["kfs"])
    a = dict(slots=np.ascontiguousarray(s["slots"], I32), off=np.ascontiguousarray(s["obs_off"], I32),
             kf=np.ascontiguousarray(s["obs_kf"], I32), idx=np.ascontiguousarray(s["obs_idx"], I32),
             Tcw=np.ascontiguousarray(s["Tcw"], F32).reshape(K, 7), fixed=np.ascontiguousarray(s["fixed"], U8),
             cam=np.ascontiguousarray(s["cam"], F32).reshape(K, 5), sig=np.ascontiguousarray(s["sig"], F32))
    E, P = int(a["off"][-1]) if len(a["off"]) else 0, len(a["slots"])
    a.update(kf_out=np.full((max(K, 1), 7), SENTINEL_F, np.float64), pos_out=np.full((max(P, 1), 3), SENTINEL_F, F32),
             erase=np.full(max(E, 1), SENTINEL_ERASE, U8), chi2=np.full(max(E, 1), SENTINEL_F, np.float64), E=E, P=P, K=K)
    return a


def result(rc, res, a, store_pos):
    out = dict(ret=rc, res_bytes=bytes(res), kf_out=a["kf_out"][:a["K"]], pos_out=a["pos_out"][:a["P"]], erase=a["erase"][:a["E"]],
               chi2=a["chi2"][:a["E"]], store_pos=store_pos)
    out.update({k: int(getattr(res, k)) for k in RES_INTS})
    out.update({k: float(getattr(res, k)) for k in RES_DOUBLES})
    return out


def run(s, stop_flag=None, nleft=None, null=(), **over):
    """One call of the host core on a scene.  over: fields of the scene to replace; null: names of arguments passed as
    NULL; stop_flag: None or 0 / 1 (the byte the flag points to)."""
    s = dict(s, **over)
    a = marshal(s)
    K = a["K"]
    kf_off = np.zeros(K + 1, I32)
    kf_off[1:] = np.cumsum([len(f["x"]) for f in s["kfs"]])
    cat = lambda k, t: np.ascontiguousarray(np.concatenate([np.asarray(f[k], t) for f in s["kfs"]]) if K else np.zeros(0, t))
    kx, ky, oc = cat("x", F32), cat("y", F32), cat("octave", I32)
    ur = np.ascontiguousarray(np.concatenate([np.full(len(f["x"]), -1, F32) if f["ur"] is None else np.asarray(f["ur"], F32)
                                              for f in s["kfs"]]) if K else np.zeros(0, F32))
    nl = np.ascontiguousarray(np.full(K, -1, I32) if nleft is None else nleft, I32)
    store_pos = np.ascontiguousarray(s["store_pos"], F32).copy()
    flag = None if stop_flag is None else np.array([stop_flag], U8)
    res = LocalBaResult()
    C.memset(C.addressof(res), 0x5A, C.sizeof(res))
    arg = lambda name, v: None if name in null else v
    rc = lib().lbacore_run(s["capacity"], _p(store_pos), a["P"], _p(arg("slots", a["slots"])), _p(arg("obs_off", a["off"])),
                           _p(arg("obs_kf", a["kf"])), _p(arg("obs_idx", a["idx"])), K, _p(kf_off), _p(kx), _p(ky), _p(oc), _p(ur),
                           _p(nl), _p(arg("kf_Tcw", a["Tcw"])), _p(arg("kf_fixed", a["fixed"])), _p(arg("kf_cam", a["cam"])),
                           _p(arg("inv_level_sigma2", a["sig"])), s["nlevels"], s["iterations"], _p(flag),
                           _p(arg("kf_Tcw_out", a["kf_out"])), _p(arg("world_pos_out", a["pos_out"])), _p(arg("erase", a["erase"])),
                           _p(arg("chi2", a["chi2"])), None if "res" in null else C.addressof(res))
    return result(rc, res, a, store_pos)
