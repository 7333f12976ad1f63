"""The host build of csrc/vsg_two_view.h (tests/_twoviewcore) through ctypes: what the TwoViewReconstruction tests compare the
restatement and the device against."""
import ctypes as C
import functools
import subprocess
from pathlib import Path

import numpy as np

F32, F64, I32, U8 = np.float32, np.float64, np.int32, np.uint8
DIR = Path(__file__).resolve().parent / "_twoviewcore"
_vp = C.c_void_p
RESULT_BYTES = 188  # vsg_two_view_result: 47 words
X3D_SENTINEL = F32(-12345.0)
REASONS = ("ok", "no_score", "singular_values", "no_winner", "low_parallax")


@functools.lru_cache(maxsize=None)
def lib():
    subprocess.check_call(["make", "-C", str(DIR)], stdout=subprocess.DEVNULL)
    L = C.CDLL(str(DIR / "libvsg_twoviewcore.so"))
    L.tv_sizes.argtypes = [_vp] * 4
    L.tv_normalize.argtypes = [C.c_int, _vp, _vp, _vp]
    L.tv_null_vectors.argtypes = [C.c_int, C.c_int, _vp, C.c_int, _vp]
    L.tv_svd3.argtypes = [C.c_int] + [_vp] * 4
    L.tv_hypotheses.argtypes = [C.c_int, C.c_int, _vp, C.c_int, _vp, _vp, _vp, C.c_float] + [_vp] * 4
    L.tv_first_maximum.argtypes = [_vp, C.c_int]
    L.tv_motions.argtypes = [C.c_int, _vp, _vp, _vp]
    L.tv_check_rt.argtypes = [_vp, _vp, C.c_float, C.c_int] + [_vp] * 6
    L.tv_ranked_cosine.argtypes = [_vp, _vp, C.c_int, C.c_int]
    L.tv_ranked_cosine.restype = C.c_float
    L.tv_choose.argtypes = [C.c_int, _vp, C.c_int, C.c_int, _vp]
    L.tv_args_ok.argtypes = [_vp, C.c_int, _vp, C.c_int, _vp, _vp, _vp, C.c_int, _vp]
    L.tv_reconstruct.argtypes = [_vp, C.c_int, _vp, C.c_int, _vp, _vp, _vp, C.c_int, _vp, C.c_int] + [_vp] * 7
    z = np.zeros(4, I32)
    L.tv_sizes(*[_p(z[k:k + 1]) for k in range(4)])
    assert tuple(z[:3]) == (32, RESULT_BYTES, 16)
    return L


def _p(a):
    return None if a is None else a.ctypes.data_as(_vp)


def sweeps():
    """(sweeps of the 9-column systems, sweeps of the 3 x 3 decompositions)"""
    z = np.zeros(4, I32)
    s9 = lib().tv_sizes(*[_p(z[k:k + 1]) for k in range(4)])
    return s9, int(z[3])


def params_blob(sigma=1.0, rh_threshold=0.5, min_parallax=1.0, min_triangulated=50):
    return np.frombuffer(np.array([sigma, rh_threshold, min_parallax], F32).tobytes() + I32(min_triangulated).tobytes(), U8).copy()


def normalize(xy):
    xy = np.ascontiguousarray(xy, F32).reshape(-1, 2)
    out, T = np.zeros(4, F32), np.zeros((3, 3), F32)
    lib().tv_normalize(len(xy), _p(xy), _p(out), _p(T))
    return out, T


def null_vectors(A, sweeps=0):
    """The double null vector of every (16 | 8) x 9 float system of A [n, rows, 9]."""
    A = np.ascontiguousarray(A, F32)
    n, rows = A.shape[0], A.shape[1]
    v = np.zeros((n, 9), F64)
    lib().tv_null_vectors(n, rows, _p(A), int(sweeps), _p(v))
    return v


def svd3(A):
    A = np.ascontiguousarray(A, F32).reshape(-1, 3, 3)
    U, w, V = np.zeros_like(A), np.zeros((len(A), 3), F32), np.zeros_like(A)
    lib().tv_svd3(len(A), _p(A), _p(U), _p(w), _p(V))
    return U, w, V


def matches_of(s):
    """The compacted matches of a scene as the header holds them: pairs [N, 2] and N x 8 float32 {u1 v1 u2 v2 x1 y1 x2 y2}."""
    i1 = np.nonzero(s["matches12"] >= 0)[0]
    i2 = s["matches12"][i1]
    n1, _ = normalize(s["xy1"])
    n2, _ = normalize(s["xy2"])
    a, b = s["xy1"][i1].astype(F32), s["xy2"][i2].astype(F32)
    m = np.zeros((len(i1), 8), F32)
    m[:, 0:2], m[:, 2:4] = a, b
    m[:, 4:6] = (a - n1[:2]) * n1[2:]
    m[:, 6:8] = (b - n2[:2]) * n2[2:]
    return np.stack([i1, i2], 1).astype(I32), m


def hypotheses(model, s, sets=None, sigma=1.0):
    """Every hypothesis of one model (0 H, 1 F) on a scene: dict(M21, M12, terms [n_iter, N, 2], inlier, score)."""
    _, m = matches_of(s)
    nm1, _ = normalize(s["xy1"])
    nm2, _ = normalize(s["xy2"])
    sets = s["sets"] if sets is None else sets
    m, sets = np.ascontiguousarray(m, F32), np.ascontiguousarray(sets, I32).reshape(-1, 8)
    N, ni = len(m), len(sets)
    mo, terms = np.zeros((ni, 18), F32), np.zeros((ni, N, 2), F32)
    fl, sc = np.zeros((ni, N), U8), np.zeros(ni, F32)
    lib().tv_hypotheses(int(model), N, _p(m), ni, _p(sets), _p(nm1), _p(nm2), float(sigma), _p(mo), _p(terms), _p(fl), _p(sc))
    return dict(M21=mo[:, :9].reshape(ni, 3, 3), M12=mo[:, 9:].reshape(ni, 3, 3), terms=terms, inlier=fl.astype(bool), score=sc)


def first_maximum(scores):
    sc = np.ascontiguousarray(scores, F32)
    return int(lib().tv_first_maximum(_p(sc), len(sc)))


def motions(model, M21, K):
    M21, K = np.ascontiguousarray(M21, F32), np.ascontiguousarray(K, F32)
    out = np.zeros((8, 12), F32)
    n = lib().tv_motions(int(model), _p(M21), _p(K), _p(out))
    return out[:n, :9].reshape(n, 3, 3), out[:n, 9:]


def check_rt(R, t, K, m, inlier, sigma=1.0):
    Rt = np.concatenate([np.asarray(R, F32).reshape(9), np.asarray(t, F32).reshape(3)])
    m, K, fl = np.ascontiguousarray(m, F32), np.ascontiguousarray(K, F32), np.ascontiguousarray(inlier, U8)
    N = len(m)
    st, cv, pos, c = np.zeros(N, U8), np.zeros(N, F32), np.zeros((N, 3), F32), np.zeros(1, F32)
    ng = lib().tv_check_rt(_p(Rt), _p(K), float(sigma), N, _p(m), _p(fl), _p(st), _p(cv), _p(pos), _p(c))
    return dict(n_good=ng, state=st, cos=cv, pos=pos, cosine=c[0])


def ranked_cosine(cosv, state):
    cv, st = np.ascontiguousarray(cosv, F32), np.ascontiguousarray(state, U8)
    return F32(lib().tv_ranked_cosine(_p(cv), _p(st), len(cv), int((st != 0).sum())))


def choose(model, n_good, N, min_triangulated):
    g, out = np.ascontiguousarray(n_good, I32), np.zeros(2, I32)
    lib().tv_choose(int(model), _p(g), int(N), int(min_triangulated), _p(out))
    return int(out[0]), int(out[1])


def args_ok(s, params=None, sets=None, matches12=None, K=None, n_iter=None):
    """The number of matches when vsg_two_view_reconstruct would take the call, -1 when it refuses."""
    xy1, xy2 = np.ascontiguousarray(s["xy1"], F32), np.ascontiguousarray(s["xy2"], F32)
    m12 = np.ascontiguousarray(s["matches12"] if matches12 is None else matches12, I32)
    st = np.ascontiguousarray(s["sets"] if sets is None else sets, I32).reshape(-1, 8)
    k = np.ascontiguousarray(s["K"] if K is None else K, F32)
    pb = params_blob() if params is None else params
    return lib().tv_args_ok(_p(xy1), len(xy1), _p(xy2), len(xy2), _p(m12), _p(k), _p(pb), len(st) if n_iter is None else n_iter, _p(st))


def parse_result(raw):
    raw = bytes(raw)
    w = np.frombuffer(raw, I32)
    f = np.frombuffer(raw, F32)
    return dict(ok=int(w[0]), reason=int(w[1]), model=int(w[2]), SH=F32(f[3]), SF=F32(f[4]), best_it_h=int(w[5]), best_it_f=int(w[6]),
                H21=f[7:16].reshape(3, 3).copy(), F21=f[16:25].reshape(3, 3).copy(), R21=f[25:34].reshape(3, 3).copy(),
                t21=f[34:37].copy(), n_good=w[37:45].copy(), parallax=F32(f[45]), n_inliers=int(w[46]), raw=raw)


def reconstruct(s, params=None, sets=None, optional=True, two_threads=False, x3d_init=None):
    """two_view::reconstruct_host on a scene: dict(res (parse_result), triangulated, x3d, inlier_h, inlier_f, score_h, score_f);
    triangulated starts as 0xAA and x3d as X3D_SENTINEL (or x3d_init), so what the routine leaves alone shows."""
    xy1, xy2 = np.ascontiguousarray(s["xy1"], F32), np.ascontiguousarray(s["xy2"], F32)
    m12, k = np.ascontiguousarray(s["matches12"], I32), np.ascontiguousarray(s["K"], F32)
    st = np.ascontiguousarray(s["sets"] if sets is None else sets, I32).reshape(-1, 8)
    pb = params_blob() if params is None else params
    n1, N, ni = len(xy1), int((m12 >= 0).sum()), len(st)
    res, tri = np.zeros(RESULT_BYTES, U8), np.full(n1, 0xAA, U8)
    x3d = np.full((n1, 3), X3D_SENTINEL, F32) if x3d_init is None else np.array(x3d_init, F32).reshape(n1, 3)
    ih, jf, sh, sf = (np.zeros(N, U8), np.zeros(N, U8), np.zeros(ni, F32), np.zeros(ni, F32)) if optional else (None,) * 4
    lib().tv_reconstruct(_p(xy1), n1, _p(xy2), len(xy2), _p(m12), _p(k), _p(pb), ni, _p(st), int(two_threads), _p(res), _p(tri),
                         _p(x3d), _p(ih), _p(jf), _p(sh), _p(sf))
    return dict(res=parse_result(res), triangulated=tri, x3d=x3d, inlier_h=ih, inlier_f=jf, score_h=sh, score_f=sf)
