"""The host build of csrc/vsg_essential_graph.h (tests/_egcore) through ctypes: what the essential-graph tests compare the
restatement and the device against.  run(scene) returns the outs of vsg_mappoints_optimize_essential_graph over sentinels
(every out the call does not write must keep them), the store's bytes after the call, and the trials' accept flags."""
import ctypes as C
import functools
import subprocess
from pathlib import Path

import numpy as np

F32, F64, I32, U8 = np.float32, np.float64, np.int32, np.uint8
DIR = Path(__file__).resolve().parent / "_egcore"
SENT = -3.0
RESULT_INTS = ("ran", "n_opt_kf", "n_fixed_kf", "n_kf", "n_edges", "n_points", "iterations_run", "trials_run", "stop_reason", "pad")
RESULT_DOUBLES = ("lambda", "chi2_initial", "chi2_final")


class Result(C.Structure):  # include/vsg_orb.h vsg_essential_graph_result
    _fields_ = [(k, C.c_int32) for k in RESULT_INTS] + [(k, C.c_double) for k in RESULT_DOUBLES]


@functools.lru_cache(maxsize=None)
def lib():
    subprocess.check_call(["make", "-C", str(DIR)], stdout=subprocess.DEVNULL)
    L = C.CDLL(str(DIR / "libvsg_egcore.so"))
    vp, ci = C.c_void_p, C.c_int
    L.egcore_run.restype = ci
    L.egcore_run.argtypes = [vp, ci, ci, vp, vp, vp, vp, ci, vp, vp, vp, ci, ci, ci, vp, vp, vp, vp, vp, vp]
    L.egcore_correct.restype = ci
    L.egcore_correct.argtypes = [vp, ci, ci, vp, vp, ci, vp, vp, vp]
    L.egcore_last_trials.argtypes = [vp, ci]
    L.egcore_log.argtypes = [ci, vp, vp]
    L.egcore_lu3.argtypes = [vp, vp, vp]
    L.egcore_sim3_log.argtypes = [vp, vp]
    L.egcore_edge_error.argtypes = [vp, vp, vp, vp]
    L.egcore_edges.restype = ci
    L.egcore_edges.argtypes = [ci] + [vp] * 7 + [ci] + [vp] * 4 + [ci, ci, ci, vp, vp, vp]
    return L


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def marshal(s):
    """The arrays of a scene as the C ABI takes them."""
    return dict(Scw=np.ascontiguousarray(s["Scw"], F64).reshape(-1, 8), nonc=np.ascontiguousarray(s["nonc"], F64).reshape(-1, 8),
                has=np.ascontiguousarray(s["has"], U8), fixed=np.ascontiguousarray(s["fixed"], U8),
                ei=np.ascontiguousarray(s["ei"], I32), ej=np.ascontiguousarray(s["ej"], I32), el=np.ascontiguousarray(s["eloop"], U8),
                slots=np.ascontiguousarray(s["slots"], I32), ref=np.ascontiguousarray(s["point_ref"], I32))


def run(s, null=(), n_kf=None, n_edges=None, n_points=None):
    """null: names of pointers passed as NULL; n_kf / n_edges / n_points override the counts (argument-error cases)."""
    L, a = lib(), marshal(s)
    K, E, P = a["Scw"].shape[0], a["ei"].size, a["slots"].size
    store = None if s.get("store_pos") is None else np.array(s["store_pos"], F32).reshape(-1, 3)
    kf_out, pos_out, chi2 = np.full((max(K, 1), 8), SENT), np.full((max(P, 1), 3), SENT, F32), np.full(max(E, 1), SENT)
    res = Result()
    C.memset(C.byref(res), 0x5a, C.sizeof(res))
    before = bytes(res)
    arg = lambda name, arr: None if name in null else _p(arr)
    rc = L.egcore_run(arg("store", store) if store is not None else None, 0 if store is None else store.shape[0],
                      K if n_kf is None else n_kf, arg("Scw", a["Scw"]), arg("nonc", a["nonc"]), arg("has", a["has"]),
                      arg("fixed", a["fixed"]), E if n_edges is None else n_edges, arg("ei", a["ei"]), arg("ej", a["ej"]),
                      arg("el", a["el"]), int(s["fix_scale"]), int(s["iterations"]), P if n_points is None else n_points,
                      arg("slots", a["slots"]), arg("ref", a["ref"]), arg("kf_out", kf_out), arg("pos_out", pos_out),
                      arg("chi2", chi2), None if "res" in null else C.byref(res))
    acc = np.zeros(1000, U8)
    nt = L.egcore_last_trials(_p(acc), acc.size)
    out = dict(ret=rc, kf_Scw=kf_out[:K], world_pos=pos_out[:P], chi2=chi2[:E], store_pos=store, accepted=[bool(v) for v in acc[:nt]],
               res_bytes=bytes(res), res_untouched=bytes(res) == before)
    out.update({k: int(getattr(res, k)) for k in RESULT_INTS})
    out.update({k: float(getattr(res, k)) for k in RESULT_DOUBLES})
    return out


def correct(store_pos, slots, point_ref, S_from, S_to_inv, null=()):
    store = np.array(store_pos, F32).reshape(-1, 3)
    sl, ref = np.ascontiguousarray(slots, I32), np.ascontiguousarray(point_ref, I32)
    a, b = np.ascontiguousarray(S_from, F64).reshape(-1, 8), np.ascontiguousarray(S_to_inv, F64).reshape(-1, 8)
    out = np.full((max(sl.size, 1), 3), SENT, F32)
    rc = lib().egcore_correct(_p(store), store.shape[0], sl.size, None if "slots" in null else _p(sl), None if "ref" in null else _p(ref),
                              a.shape[0], None if "from" in null else _p(a), None if "to" in null else _p(b), _p(out))
    return dict(ret=rc, store_pos=store, world_pos=out[:sl.size])


def dlog(x):
    x = np.ascontiguousarray(x, F64)
    y = np.zeros_like(x)
    lib().egcore_log(x.size, _p(x), _p(y))
    return y


def lu3(W, t):
    W, t, x = np.ascontiguousarray(W, F64), np.ascontiguousarray(t, F64), np.zeros(3)
    lib().egcore_lu3(_p(W), _p(t), _p(x))
    return x


def sim3_log(S):
    S, o = np.ascontiguousarray(S, F64), np.zeros(7)
    lib().egcore_sim3_log(_p(S), _p(o))
    return o


def edge_error(Cm, v1, v2):
    a, b, c, o = (np.ascontiguousarray(v, F64) for v in (Cm, v1, v2)) + (np.zeros(7),)
    lib().egcore_edge_error(_p(a), _p(b), _p(c), _p(o))
    return o


def _csr(lists):
    off = np.zeros(len(lists) + 1, I32)
    off[1:] = np.cumsum([len(l) for l in lists])
    flat = np.array([v for l in lists for v in l], I32)
    return off, flat if flat.size else np.zeros(1, I32)


def edges(g):
    """vsg::essential_graph_edges on a keyframe graph of eg_scenes (parent, loops, children, covisibles, loop_connections)."""
    K = len(g["parent"])
    parent = np.ascontiguousarray(g["parent"], I32)
    lo, li = _csr(g["loops"])
    co, cidx = _csr([sorted(c) for c in g["children"]])
    vo, vi = _csr(g["covisibles"])
    lc = g["loop_connections"]
    lckf = np.array([k for k, _ in lc], I32) if lc else np.zeros(1, I32)
    lco, lci = _csr([[j for j, _ in conns] for _, conns in lc])
    _, lcw = _csr([[w for _, w in conns] for _, conns in lc])
    cap = 16 * K + 64
    ei, ej, el = np.zeros(cap, I32), np.zeros(cap, I32), np.zeros(cap, U8)
    n = lib().egcore_edges(K, _p(parent), _p(lo), _p(li), _p(co), _p(cidx), _p(vo), _p(vi), len(lc), _p(lckf), _p(lco), _p(lci),
                           _p(lcw), int(g["cur"]), int(g["loop_kf"]), cap, _p(ei), _p(ej), _p(el))
    assert 0 <= n <= cap
    return ei[:n], ej[:n], el[:n]
