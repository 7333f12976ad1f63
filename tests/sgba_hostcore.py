"""The host build of csrc/vsg_sgraph_ba.h (tests/_sgbacore) through ctypes: what the tests of
vsg_mappoints_local_bundle_adjustment_sgraph compare the restatement and the device against.  run(scene) returns the fields
of sgba_reference.local_ba_sgraph plus the return code, `res` bytes and the store's positions after the call; every out starts
as a sentinel so that "nothing written" is visible.  The visual arguments are marshalled by lba_hostcore."""
import ctypes as C
import functools
import subprocess
from pathlib import Path

import numpy as np

import lba_hostcore as hc

F32, I32, U8, F64 = np.float32, np.int32, np.uint8, np.float64
DIR = Path(__file__).resolve().parent / "_sgbacore"
SENTINEL_F, SENTINEL_ERASE = hc.SENTINEL_F, hc.SENTINEL_ERASE
SEM_INTS = ("n_planes_active", "n_rooms_active", "n_plane_kf", "n_plane_point", "n_room_edges", "n_rows", "n_erase_plane", "reserved")
SEM_IN = ("plane_eq", "pl_obs_off", "pl_obs_kf", "pl_obs_local", "pl_obs_G", "w_plane_kf", "w_plane_point", "room_center",
          "room_n_walls", "room_wall")
SEM_OUT = ("plane_eq_out", "room_center_out", "erase_plane", "chi2_plane_kf", "chi2_plane_point")


class SGraphLocalBaResult(C.Structure):  # include/vsg_orb.h vsg_sgraph_local_ba_result
    _fields_ = [("local", hc.LocalBaResult)] + [(k, C.c_int32) for k in SEM_INTS]


@functools.lru_cache(maxsize=None)
def lib():
    subprocess.check_call(["make", "-C", str(DIR)], stdout=subprocess.DEVNULL)
    L = C.CDLL(str(DIR / "libvsg_sgbacore.so"))
    vp, ci, d = C.c_void_p, C.c_int, C.c_double
    L.sgbacore_run.restype = ci
    L.sgbacore_run.argtypes = [ci, vp, ci, vp, vp, vp, vp, ci] + [vp] * 10 + [ci, ci] + [vp] * 5 + [ci] + [vp] * 7 + [ci] + [vp] * 9
    L.sgbacore_atan2.restype = d
    L.sgbacore_atan2.argtypes = [d, d]
    L.sgbacore_sincos.argtypes = [d, vp, vp]
    L.sgbacore_point_plane_error.restype = d
    for name in ("plane_oplus", "plane_ominus", "wall_pair"):
        getattr(L, "sgbacore_" + name).argtypes = [vp] * 3
    L.sgbacore_plane_transform.argtypes = [vp] * 4
    L.sgbacore_point_plane_error.argtypes = [vp] * 4
    return L


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def marshal_sem(q):
    """The semantic arrays as the C interfaces take them, and their outs filled with sentinels."""
    Pl, R = len(np.asarray(q["plane_eq"]).reshape(-1, 4)), len(np.asarray(q["room_center"]).reshape(-1, 3))
    pad = lambda a, t, n: (lambda v: v if v.size else np.zeros(n, t))(np.ascontiguousarray(a, t).reshape(-1))
    a = dict(plane_eq=pad(q["plane_eq"], F64, 4), pl_obs_off=pad(q["pl_obs_off"], I32, 1), pl_obs_kf=pad(q["pl_obs_kf"], I32, 1),
             pl_obs_local=pad(q["pl_obs_local"], F64, 4), pl_obs_G=pad(q["pl_obs_G"], F64, 16), w_plane_kf=pad(q["w_plane_kf"], F64, 1),
             w_plane_point=pad(q["w_plane_point"], F64, 1), room_center=pad(q["room_center"], F64, 3),
             room_n_walls=pad(q["room_n_walls"], I32, 1), room_wall=pad(q["room_wall"], I32, 4))
    NO = int(np.asarray(q["pl_obs_off"]).reshape(-1)[-1])
    a.update(Pl=Pl, R=R, NO=NO, plane_eq_out=np.full((max(Pl, 1), 4), SENTINEL_F, F64), room_center_out=np.full((max(R, 1), 3), SENTINEL_F, F64),
             erase_plane=np.full(max(NO, 1), SENTINEL_ERASE, U8), chi2_plane_kf=np.full(max(NO, 1), SENTINEL_F, F64),
             chi2_plane_point=np.full(max(NO, 1), SENTINEL_F, F64))
    return a


def result(rc, res, a, b, store_pos):
    out = hc.result(rc, res.local, a, store_pos)
    out.update(res_bytes=bytes(res), plane_out=b["plane_eq_out"][:b["Pl"]], room_out=b["room_center_out"][:b["R"]],
               erase_plane=b["erase_plane"][:b["NO"]], chi2_pk=b["chi2_plane_kf"][:b["NO"]], chi2_pp=b["chi2_plane_point"][:b["NO"]])
    out.update({k: int(getattr(res, k)) for k in SEM_INTS})
    return out


def sem_args(b, null=()):
    """The entry's arguments from n_planes on, res excluded."""
    g = lambda k: None if k in null else _p(b[k])
    return [b["Pl"], g("plane_eq"), g("pl_obs_off"), g("pl_obs_kf"), g("pl_obs_local"), g("pl_obs_G"), g("w_plane_kf"), g("w_plane_point"),
            b["R"], g("room_center"), g("room_n_walls"), g("room_wall")] + [g(k) for k in SEM_OUT]


def run(s, stop_flag=None, nleft=None, null=(), sem=None, **over):
    """One call of the host core on a scene.  over: fields of the scene to replace; sem: fields of scene["sem"] to replace;
    null: names of arguments passed as NULL; stop_flag: None or 0 / 1."""
    s = dict(s, **over)
    q = dict(s["sem"], **(sem or {}))
    a, b = hc.marshal(s), marshal_sem(q)
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
    res = SGraphLocalBaResult()
    C.memset(C.addressof(res), 0x5A, C.sizeof(res))
    arg = lambda name, v: None if name in null else v
    rc = lib().sgbacore_run(s["capacity"], _p(store_pos), a["P"], _p(arg("slots", a["slots"])), _p(arg("obs_off", a["off"])),
                            _p(arg("obs_kf", a["kf"])), _p(arg("obs_idx", a["idx"])), K, _p(kf_off), _p(kx), _p(ky), _p(oc), _p(ur),
                            _p(nl), _p(arg("kf_Tcw", a["Tcw"])), _p(arg("kf_fixed", a["fixed"])), _p(arg("kf_cam", a["cam"])),
                            _p(arg("inv_level_sigma2", a["sig"])), s["nlevels"], s["iterations"], _p(flag),
                            _p(arg("kf_Tcw_out", a["kf_out"])), _p(arg("world_pos_out", a["pos_out"])), _p(arg("erase", a["erase"])),
                            _p(arg("chi2", a["chi2"])), *sem_args(b, null), None if "res" in null else C.addressof(res))
    return result(rc, res, a, b, store_pos)
