"""The host build of csrc/vsg_pose_opt.h (tests/_posecore) through ctypes: what the pose tests compare the restatement
and the device against.  run(scene) returns the same fields as pose_reference.pose_optimization, chi2 / outlier as full
per-feature arrays over sentinels (outlier 7, chi2 -1: entries of features without a slot must keep them)."""
import ctypes as C
import functools
import subprocess
from pathlib import Path

import numpy as np

F32, I32, U8 = np.float32, np.int32, np.uint8
DIR = Path(__file__).resolve().parent / "_posecore"
SENTINEL_FLAG, SENTINEL_CHI2 = 7, -1.0


@functools.lru_cache(maxsize=None)
def lib():
    subprocess.check_call(["make", "-C", str(DIR)], stdout=subprocess.DEVNULL)
    L = C.CDLL(str(DIR / "libvsg_posecore.so"))
    L.posecore_run.restype = C.c_int
    L.posecore_run.argtypes = [C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 8 + [C.c_int, C.c_int] + [C.c_void_p] * 6
    L.posecore_sincos.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.posecore_oplus.argtypes = [C.c_void_p] * 3
    return L


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def run(s, hold=None, removed="scene"):
    """One call of the host core on a scene.  hold: None = hold when the scene has a removed set."""
    removed = s["removed"] if isinstance(removed, str) else removed
    hold = (s["removed"] is not None) if hold is None else hold
    n = s["n"]
    arr = dict(slots=np.ascontiguousarray(s["feat_slots"], I32), pos=np.ascontiguousarray(s["world_pos"], F32),
               kx=np.ascontiguousarray(s["kx"], F32), ky=np.ascontiguousarray(s["ky"], F32),
               oct=np.ascontiguousarray(s["octave"], I32),
               ur=None if s["u_right"] is None else np.ascontiguousarray(s["u_right"], F32),
               pose=np.concatenate([s["q"], s["t"]]).astype(F32), cam=np.array(s["cam"], F32),
               sig=np.ascontiguousarray(s["inv_sigma2"], F32),
               rem=None if removed is None or not hold else np.ascontiguousarray(removed, U8))
    outlier, chi2 = np.full(max(n, 1), SENTINEL_FLAG, U8), np.full(max(n, 1), SENTINEL_CHI2, F32)
    qt, ri, held = np.zeros(7), np.zeros(4, I32), np.zeros(7)
    rc = lib().posecore_run(n, _p(arr["slots"]), s["capacity"], _p(arr["pos"]), _p(arr["kx"]), _p(arr["ky"]), _p(arr["oct"]),
                            _p(arr["ur"]), _p(arr["pose"]), _p(arr["cam"]), _p(arr["sig"]), s["nlevels"], 2 if hold else -1,
                            _p(arr["rem"]), _p(outlier), _p(chi2), _p(qt), _p(ri), _p(held))
    return dict(ret=rc, outlier=outlier[:n], chi2=chi2[:n], q=qt[:4].copy(), t=qt[4:].copy(), n_initial=int(ri[0]),
                n_bad=int(ri[1]), rounds_run=int(ri[2]), held=int(ri[3]), held_q=held[:4].copy(), held_t=held[4:].copy())


def sincos(x):
    x = np.ascontiguousarray(x, np.float64)
    s, c = np.zeros_like(x), np.zeros_like(x)
    lib().posecore_sincos(len(x), _p(x), _p(s), _p(c))
    return s, c


def oplus(q, t, update):
    e, u, o = np.concatenate([q, t]).astype(np.float64), np.ascontiguousarray(update, np.float64), np.zeros(7)
    lib().posecore_oplus(_p(e), _p(u), _p(o))
    return o[:4], o[4:]
