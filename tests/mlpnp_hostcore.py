"""The host build of csrc/vsg_mlpnp.h (tests/_mlpnpcore) through ctypes: what the MLPnP tests compare the restatement and the
device against."""
import ctypes as C
import functools
import subprocess
from pathlib import Path

import numpy as np

F32, F64, I32, U8 = np.float32, np.float64, np.int32, np.uint8
DIR = Path(__file__).resolve().parent / "_mlpnpcore"
_vp = C.c_void_p
POINT_BYTES, POSE_BYTES, RESULT_BYTES = 32, 96, 96  # vsg_mlpnp_result: 16 floats + 8 int32


@functools.lru_cache(maxsize=None)
def lib():
    subprocess.check_call(["make", "-C", str(DIR)], stdout=subprocess.DEVNULL)
    L = C.CDLL(str(DIR / "libvsg_mlpnpcore.so"))
    ci, cf = C.c_int, C.c_float
    L.mc_sizes.argtypes = [_vp] * 3
    L.mc_acos.argtypes = L.mc_cbrt.argtypes = [ci, _vp, _vp]
    L.mc_rot2rodrigues.argtypes = [_vp, _vp]
    L.mc_points.argtypes = [ci] + [_vp] * 7 + [cf, _vp]
    L.mc_hypotheses.argtypes = [ci, _vp, _vp, ci] + [_vp] * 5
    L.mc_refine.argtypes = [ci] + [_vp] * 7
    L.mc_select.argtypes = [_vp, ci, ci, ci, ci, _vp]
    L.mc_args_ok.argtypes = [ci, _vp, ci, _vp, ci, _vp, cf, ci, ci, ci, ci, ci, _vp, _vp, _vp, _vp]
    L.mc_ransac.argtypes = [ci] + [_vp] * 7 + [cf] + [ci] * 5 + [_vp, ci] + [_vp] * 4
    L.mc_parameters.argtypes = [C.c_double, ci, ci, ci, cf, ci, _vp, _vp]
    sizes = np.zeros(3, I32)
    L.mc_sizes(_p(sizes[:1]), _p(sizes[1:2]), _p(sizes[2:]))
    assert tuple(sizes) == (POINT_BYTES, POSE_BYTES, RESULT_BYTES)
    return L


def _p(a):
    return None if a is None else a.ctypes.data_as(_vp)


def _c(a, t):
    return None if a is None else np.ascontiguousarray(a, t)


def sweeps():
    z = np.zeros(3, I32)
    return lib().mc_sizes(_p(z[:1]), _p(z[1:2]), _p(z[2:]))


def acos(x):
    x = _c(x, F64)
    y = np.zeros_like(x)
    lib().mc_acos(len(x), _p(x), _p(y))
    return y


def cbrt(x):
    x = _c(x, F64)
    y = np.zeros_like(x)
    lib().mc_cbrt(len(x), _p(x), _p(y))
    return y


def rot2rodrigues(R):
    R, w = _c(R, F64).reshape(9), np.zeros(3, F64)
    lib().mc_rot2rodrigues(_p(R), _p(w))
    return w


def _scene_arrays(s, cam, sigma2):
    return (_c(s["slots"], I32), _c(s["world_pos"], F32), _c(s["kx"], F32), _c(s["ky"], F32), _c(s["octave"], I32),
            np.asarray(cam, F32), _c(sigma2, F32))


def points(s, cam, sigma2, th2):
    """The correspondences of a scene as the solver keeps them: raw [n, 32] bytes."""
    sl, wp, kx, ky, oc, cm, sg = _scene_arrays(s, cam, sigma2)
    pts = np.zeros((max(s["n"], 1), POINT_BYTES), U8)
    n = lib().mc_points(len(sl), _p(sl), _p(wp), _p(kx), _p(ky), _p(oc), _p(cm), _p(sg), th2, _p(pts))
    assert n == s["n"]
    return pts[:n]


INFO = ("planar", "err_lo", "err_hi", "gn_rounds", "gn_aborted", "gn_max_dx", "gn_min_dx", "gn_max_dl")


def hypotheses(pts, cam, sets):
    """Every hypothesis: dict(T [n_hyp, 3, 4], info [n_hyp, 8] (INFO), counts, flags [n_hyp, n])."""
    pts, sets, cm = np.ascontiguousarray(pts), _c(sets, I32).reshape(-1, 6), np.asarray(cam, F32)
    n, nh = len(pts), len(sets)
    T, info = np.zeros((nh, 3, 4), F64), np.zeros((nh, 8), F64)
    counts, flags = np.zeros(nh, I32), np.zeros((nh, max(n, 1)), U8)
    lib().mc_hypotheses(n, _p(pts), _p(cm), nh, _p(sets), _p(T), _p(info), _p(counts), _p(flags))
    return dict(T=T, info=info, counts=counts, flags=flags[:, :n].astype(bool))


def refine(pts, cam, member):
    """computePose over the set `member` (the solve Refine() runs over the best set and discards)."""
    pts, cm, mb = np.ascontiguousarray(pts), np.asarray(cam, F32), _c(member, U8)
    n = len(pts)
    T, info, count, flags = np.zeros((3, 4), F64), np.zeros(8, F64), np.zeros(1, I32), np.zeros(max(n, 1), U8)
    lib().mc_refine(n, _p(pts), _p(cm), _p(mb), _p(T), _p(info), _p(count), _p(flags))
    return dict(T=T, info=info, count=int(count[0]), flags=flags[:n].astype(bool))


def select(counts, first, n_iterations, max_its, min_inliers):
    c, out = _c(counts, I32), np.zeros(7, I32)
    lib().mc_select(_p(c), first, n_iterations, max_its, min_inliers, _p(out))
    return dict(found=int(out[0]), no_more=int(out[1]), refined=int(out[2]), best=int(out[3]), iterations=int(out[4]),
                pose=int(out[5]), records=int(out[6]))


def args_ok(s, cam, sigma2, nlevels, th2, min_inliers, max_its, first, n_iterations, sets, n_hyp=None, capacity=None,
            slots="scene", octave="scene", inlier=True, res=True, level_sigma2="given"):
    """(ok, n) of mlpnp::args_ok on a scene with single arguments replaced."""
    sl = _c(s["slots"] if isinstance(slots, str) else slots, I32)
    oc = _c(s["octave"] if isinstance(octave, str) else octave, I32)
    sg = _c(sigma2, F32) if isinstance(level_sigma2, str) else level_sigma2
    sm = None if sets is None else _c(sets, I32).reshape(-1)
    nh = (len(sm) // 6 if sm is not None else 0) if n_hyp is None else n_hyp
    fl = np.zeros(max(s["n_feat"], 1), U8) if inlier else None
    rs = np.zeros(RESULT_BYTES, U8) if res else None
    n = np.zeros(1, I32)
    ok = lib().mc_args_ok(s["n_feat"], _p(sl), s["capacity"] if capacity is None else capacity, _p(sg), nlevels, _p(oc), th2,
                          min_inliers, max_its, first, n_iterations, nh, _p(sm), _p(fl), _p(rs), _p(n))
    return bool(ok), int(n[0])


def parse_result(raw):
    raw = bytes(raw)
    f, i = np.frombuffer(raw[:64], F32), np.frombuffer(raw[64:RESULT_BYTES], I32)
    return dict(Tcw=f.reshape(4, 4).copy(), found=int(i[0]), no_more=int(i[1]), n_inliers=int(i[2]), refined=int(i[3]),
                best_hypothesis=int(i[4]), iterations=int(i[5]), n_correspondences=int(i[6]), n_records=int(i[7]), raw=raw)


def ransac(s, cam, sigma2, th2, min_inliers, max_its, first, n_iterations, sets=None, want_hyp=True):
    """mlpnp::ransac_host on a scene: dict(inlier, res (parse_result), hyp_inliers, hyp_T)."""
    sl, wp, kx, ky, oc, cm, sg = _scene_arrays(s, cam, sigma2)
    sm = _c(s["sets"] if sets is None else sets, I32).reshape(-1, 6)
    nh, nf = len(sm), s["n_feat"]
    n = int((sl >= 0).sum())
    inl, res = np.full(max(nf, 1), 0xAA, U8), np.zeros(RESULT_BYTES, U8)
    hcnt, hT = (np.zeros(nh, I32), np.zeros((nh, 3, 4), F64)) if want_hyp else (None, None)
    lib().mc_ransac(nf, _p(sl), _p(wp), _p(kx), _p(ky), _p(oc), _p(cm), _p(sg), th2, min_inliers, max_its, first, n_iterations, nh,
                    _p(sm), n, _p(inl), _p(res), _p(hcnt), _p(hT))
    return dict(inlier=inl[:nf], res=parse_result(res), hyp_inliers=hcnt, hyp_T=hT)


def parameters(probability, min_inliers, max_iterations, min_set, epsilon, n):
    o = np.zeros(2, I32)
    lib().mc_parameters(probability, min_inliers, max_iterations, min_set, epsilon, n, _p(o[:1]), _p(o[1:]))
    return int(o[0]), int(o[1])
