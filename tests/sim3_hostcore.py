"""The host build of csrc/vsg_sim3.h (tests/_sim3core) through ctypes: what the Sim3 tests compare the restatement and the
device against."""
import ctypes as C
import functools
import subprocess
from pathlib import Path

import numpy as np

F32, F64, I32, U8 = np.float32, np.float64, np.int32, np.uint8
DIR = Path(__file__).resolve().parent / "_sim3core"
_vp = C.c_void_p
RESULT_BYTES = 136  # vsg_sim3_result: 29 floats + 5 int32


@functools.lru_cache(maxsize=None)
def lib():
    subprocess.check_call(["make", "-C", str(DIR)], stdout=subprocess.DEVNULL)
    L = C.CDLL(str(DIR / "libvsg_sim3core.so"))
    L.sc_sizes.argtypes = [_vp, _vp]
    L.sc_eigenvectors.argtypes = [C.c_int, _vp, _vp]
    L.sc_rotations.argtypes = [C.c_int, _vp, _vp]
    L.sc_points.argtypes = [C.c_int] + [_vp] * 7
    L.sc_hypotheses.argtypes = [C.c_int, _vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp]
    L.sc_select.argtypes = [_vp, C.c_int, C.c_int, _vp]
    L.sc_args_ok.argtypes = [C.c_int, _vp, _vp, C.c_int, C.c_int, _vp, _vp, C.c_int, C.c_int, _vp, _vp]
    L.sc_ransac.argtypes = [C.c_int] + [_vp] * 6 + [C.c_int] * 3 + [_vp, C.c_int] + [_vp] * 4
    sizes = np.zeros(2, I32)
    L.sc_sizes(_p(sizes[:1]), _p(sizes[1:]))
    assert tuple(sizes) == (48, RESULT_BYTES)
    return L


def _p(a):
    return None if a is None else a.ctypes.data_as(_vp)


def sweeps():
    z = np.zeros(2, I32)
    return lib().sc_sizes(_p(z[:1]), _p(z[1:]))


def pose_blob(kf):
    """A scene's keyframe as the bytes of vsg_frame_pose (Ow, mbf, log_scale_factor, n_levels are not read: zeros)."""
    b = np.concatenate([np.asarray(kf["Rcw"], F32).reshape(9), np.asarray(kf["tcw"], F32), np.zeros(3, F32),
                        np.array([kf["fx"], kf["fy"], kf["cx"], kf["cy"], 0.0, 0.0], F32)]).tobytes() + I32(0).tobytes()
    assert len(b) == 88
    return np.frombuffer(b, U8).copy()


def eigenvectors(N):
    N = np.ascontiguousarray(N, F32).reshape(-1, 16)
    q = np.zeros((len(N), 4), F64)
    lib().sc_eigenvectors(len(N), _p(N), _p(q))
    return q


def rotations(q):
    q = np.ascontiguousarray(q, F64).reshape(-1, 4)
    R = np.zeros((len(q), 3, 3), F32)
    lib().sc_rotations(len(q), _p(q), _p(R))
    return R


def points(s, pose2=None):
    """n x 12 float32: X1, X2, p1, p2, max_err1, max_err2 of every correspondence of a scene."""
    n = len(s["Xw1"])
    a, b = pose_blob(s["kf1"]), pose_blob(s["kf2"] if pose2 is None else pose2)
    X1, X2 = np.ascontiguousarray(s["Xw1"], F32), np.ascontiguousarray(s["Xw2"], F32)
    e1, e2 = np.ascontiguousarray(s["max_err1"], F32), np.ascontiguousarray(s["max_err2"], F32)
    pts = np.zeros((max(n, 1), 12), F32)
    lib().sc_points(n, _p(a), _p(b), _p(X1), _p(X2), _p(e1), _p(e2), _p(pts))
    return pts[:n]


def hypotheses(s, pts, samples, fix_scale=False):
    """Every hypothesis of `samples` on the points: dict(R, t, s, T12, T21, N, err [n_hyp, n, 2], inlier [n_hyp, n])."""
    pts, sm = np.ascontiguousarray(pts, F32), np.ascontiguousarray(samples, I32).reshape(-1, 3)
    n, nh = len(pts), len(sm)
    a, b = pose_blob(s["kf1"]), pose_blob(s["kf2"])
    hyp, N = np.zeros((nh, 45), F32), np.zeros((nh, 4, 4), F32)
    err, fl = np.zeros((nh, max(n, 1), 2), F32), np.zeros((nh, max(n, 1)), U8)
    lib().sc_hypotheses(n, _p(pts), _p(a), _p(b), int(fix_scale), nh, _p(sm), _p(hyp), _p(N), _p(err), _p(fl))
    return dict(R=hyp[:, :9].reshape(nh, 3, 3), t=hyp[:, 9:12], s=hyp[:, 12], T12=hyp[:, 13:29].reshape(nh, 4, 4),
                T21=hyp[:, 29:45].reshape(nh, 4, 4), N=N, err=err[:, :n], inlier=fl[:, :n].astype(bool))


def select(counts, min_inliers):
    c, out = np.ascontiguousarray(counts, I32), np.zeros(3, I32)
    lib().sc_select(_p(c), len(c), int(min_inliers), _p(out))
    return dict(best=int(out[0]), converged=bool(out[1]), iterations=int(out[2]))


def args_ok(n, slots1, slots2, cap1, cap2, max_err1, max_err2, min_inliers, n_hyp, samples, inlier=True):
    opt = lambda a, t: None if a is None else np.ascontiguousarray(a, t)  # noqa: E731
    s1, s2, e1, e2, sm = opt(slots1, I32), opt(slots2, I32), opt(max_err1, F32), opt(max_err2, F32), opt(samples, I32)
    fl = np.zeros(max(n, 1), U8) if inlier else None
    return bool(lib().sc_args_ok(n, _p(s1), _p(s2), cap1, cap2, _p(e1), _p(e2), min_inliers, n_hyp, _p(sm), _p(fl)))


def parse_result(raw):
    raw = bytes(raw)
    f, i = np.frombuffer(raw[:116], F32), np.frombuffer(raw[116:RESULT_BYTES], I32)
    return dict(R12=f[:9].reshape(3, 3).copy(), t12=f[9:12].copy(), s12=F32(f[12]), T12=f[13:29].reshape(4, 4).copy(),
                converged=int(i[0]), no_more=int(i[1]), n_inliers=int(i[2]), best_hypothesis=int(i[3]), iterations=int(i[4]), raw=raw)


def ransac(s, min_inliers=15, fix_scale=False, samples=None, early_exit=False, want_hyp=True):
    """sim3::ransac_host on a scene: dict(inlier, res (parse_result), hyp_inliers, hyp_T12)."""
    n = len(s["Xw1"])
    sm = np.ascontiguousarray(s["samples"] if samples is None else samples, I32).reshape(-1, 3)
    nh = len(sm)
    a, b = pose_blob(s["kf1"]), pose_blob(s["kf2"])
    X1, X2 = np.ascontiguousarray(s["Xw1"], F32), np.ascontiguousarray(s["Xw2"], F32)
    e1, e2 = np.ascontiguousarray(s["max_err1"], F32), np.ascontiguousarray(s["max_err2"], F32)
    inl, res = np.full(max(n, 1), 0xAA, U8), np.zeros(RESULT_BYTES, U8)
    hc, hT = (np.zeros(nh, I32), np.zeros((nh, 4, 4), F32)) if want_hyp else (None, None)
    lib().sc_ransac(n, _p(X1), _p(X2), _p(e1), _p(e2), _p(a), _p(b), int(fix_scale), int(min_inliers), nh, _p(sm), int(early_exit),
                    _p(inl), _p(res), _p(hc), _p(hT))
    return dict(inlier=inl[:n], res=parse_result(res), hyp_inliers=hc, hyp_T12=hT)
