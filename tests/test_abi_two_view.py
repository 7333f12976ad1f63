"""The C ABI of TwoViewReconstruction (include/vsg_orb.h: vsg_frame_two_view_reconstruct, vsg_two_view_reconstruct,
vsg_two_view_default_params, vsg_two_view_draw_sets) without a device: the symbols, the layout of the two structs as the header
declares them, the draw of the minimal sets against the transcribed loop, and every refusal with its sentinels intact.  The
host-array form checks its arguments before it asks for a device, so the library itself refuses here; the resident form needs
frames, which cannot exist without a device: tests/test_gpu_two_view.py repeats each refusal on real frames."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import two_view_hostcore as hc
import two_view_scenes as ts
from visual_sgraphs_amd import orb

ROOT = Path(__file__).resolve().parent.parent
INVALID = -6
F32, I32, U8 = np.float32, np.int32, np.uint8


def test_symbols_are_exported_declared_and_bound():
    L = orb.load_library()
    header = (ROOT / "include" / "vsg_orb.h").read_text()
    for name, nargs in (("vsg_frame_two_view_reconstruct", 14), ("vsg_two_view_reconstruct", 17), ("vsg_two_view_draw_sets", 5)):
        assert hasattr(L, name) and re.search(r"\bint %s\(" % name, header) and name in orb.EXPORTS, name
        assert len(getattr(L, name).argtypes) == nargs
        decl = header[header.index("int %s(" % name):]
        decl = decl[:decl.index(";")].replace("int (*random_int)(int lo, int hi, void *ctx)", "random_int")  # one argument
        assert decl.count(",") + 1 == nargs, name
    assert "void vsg_two_view_default_params(" in header and "vsg_two_view_default_params" in orb.EXPORTS
    for cite in ("TwoViewReconstruction.cc:40-129", "Tracking.cc:2568", "Pinhole.cpp:91-101", "KannalaBrandt8.cpp:181-211", ":82-97",
                 ":724-730", ":879-884", "ONE enqueue", "Random.cpp:47-50"):
        assert cite in header, cite
    assert callable(orb.TwoViewReconstruction.Reconstruct) and callable(orb.two_view_draw_sets)
    # both entry points check before the thread's context is asked for and before anything is launched
    src = (ROOT / "visual_sgraphs_amd" / "csrc" / "vsg_two_view.hip").read_text()
    for name in ("int vsg_frame_two_view_reconstruct(", "int vsg_two_view_reconstruct("):
        body = src[src.rindex(name):]
        assert body.index("tv_check(") < body.index("tv_run(")
    run = src[src.index("int tv_run("):src.index("int tv_check(")]
    assert run.index("thread_ctx(") < run.index("hipLaunchKernelGGL(") and "tv_check(" not in run


def test_struct_layouts_match_the_header_and_the_defaults_are_the_references(tmp_path):
    fields = ("ok", "reason", "model", "SH", "SF", "best_it_h", "best_it_f", "H21", "F21", "R21", "t21", "n_good", "parallax", "n_inliers")
    pfields = ("sigma", "rh_threshold", "min_parallax", "min_triangulated")
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vsg_orb.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(vsg_two_view_result));\n' +
                   "".join('  printf(" %%zu", offsetof(vsg_two_view_result, %s));\n' % f for f in fields) +
                   '  printf(" %zu", sizeof(vsg_two_view_params));\n' +
                   "".join('  printf(" %%zu", offsetof(vsg_two_view_params, %s));\n' % f for f in pfields) + '  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", str(ROOT / "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    T, P = orb.TwoViewResult, orb.TwoViewParams
    assert got == [C.sizeof(T)] + [getattr(T, f).offset for f in fields] + [C.sizeof(P)] + [getattr(P, f).offset for f in pfields]
    assert got[0] == hc.RESULT_BYTES and got[15] == 16
    p = orb.TwoViewParams()
    orb.load_library().vsg_two_view_default_params(C.byref(p))
    assert (p.sigma, p.rh_threshold, p.min_parallax, p.min_triangulated) == (1.0, 0.5, 1.0, 50)
    assert bytes(p) == hc.params_blob().tobytes()


def test_draw_sets_is_the_transcribed_loop_and_refuses():
    calls = []

    def counting(lo, hi):
        calls.append((lo, hi))
        return (7 * len(calls)) % (hi - lo + 1) + lo
    got = orb.two_view_draw_sets(23, 9, counting)
    seen = list(calls)
    calls.clear()
    want = ts.draw_sets(23, 9, counting)
    assert np.array_equal(got, want) and seen == calls and len(calls) == 72
    assert all(lo == 0 for lo, _ in calls) and [hi for _, hi in calls[:8]] == list(range(22, 14, -1))
    assert all(len(set(row)) == 8 for row in got.tolist())
    assert orb.two_view_draw_sets(8, 3, lambda lo, hi: hi).tolist() == [[7, 6, 5, 4, 3, 2, 1, 0]] * 3
    # RandomInt's formula over rand(): in range, without replacement
    d = orb.two_view_draw_sets(40, 50)
    assert d.min() >= 0 and d.max() < 40 and all(len(set(r)) == 8 for r in d.tolist())
    L = orb.load_library()
    out = np.full(16, -9, I32)
    cb = orb._RANDOM_INT(lambda lo, hi, _c: hi + 1)
    for args in ((7, 2, orb._RANDOM_INT(), None, out.ctypes.data_as(C.POINTER(C.c_int32))), (8, -1, orb._RANDOM_INT(), None, out.ctypes.data_as(C.POINTER(C.c_int32))),
                 (8, 2, orb._RANDOM_INT(), None, None), (8, 2, cb, None, out.ctypes.data_as(C.POINTER(C.c_int32)))):
        assert L.vsg_two_view_draw_sets(*args) == INVALID
    assert (out == -9).all()


def _scene():
    return ts.make(3, n=40, n_iter=6)


def _refusals(s):
    m12, sets, N, n2 = s["matches12"], s["sets"], s["n"], s["n2"]
    first = int(np.nonzero(m12 >= 0)[0][0])

    def edit(a, i, v):
        a = np.array(a, copy=True)
        a.reshape(-1)[i] = v
        return a
    few = np.full_like(m12, -1)
    keep = np.nonzero(m12 >= 0)[0][:7]
    few[keep] = m12[keep]
    Kn, Ki = s["K"].copy(), s["K"].copy()
    Kn[0, 2], Ki[1, 1] = np.nan, np.inf
    return {
        "match == n2": dict(matches12=edit(m12, first, n2)), "match < -1": dict(matches12=edit(m12, first, -2)),
        "7 matches": dict(matches12=few), "n_iter 0": dict(n_iter=0), "n_iter 1025": dict(sets=np.resize(sets, (1025, 8))),
        "set entry == N": dict(sets=edit(sets, 5, N)), "set entry < 0": dict(sets=edit(sets, 9, -1)),
        "two equal entries in one set": dict(sets=edit(sets, 3, sets[0, 0])), "two equal entries, last set": dict(sets=edit(sets, 47, sets[5, 0])),
        "K NaN": dict(K=Kn), "K inf": dict(K=Ki), "sigma inf": dict(params=hc.params_blob(sigma=np.inf)),
        "sigma NaN": dict(params=hc.params_blob(sigma=np.nan)), "sigma 0": dict(params=hc.params_blob(sigma=0.0)),
        "sigma < 0": dict(params=hc.params_blob(sigma=-1.0)),
    }


def test_the_good_call_passes_the_checks():
    s = _scene()
    assert hc.args_ok(s) == 40
    assert hc.args_ok(s, sets=np.resize(s["sets"], (1024, 8))) == 40 and hc.args_ok(s, sets=s["sets"][:1]) == 40
    eight = ts.make(4, n=8, n_iter=3, outliers=0.0)
    assert hc.args_ok(eight) == 8 and all(sorted(r) == list(range(8)) for r in eight["sets"].tolist())


@pytest.mark.parametrize("what", list(_refusals(_scene())))
def test_every_check_refuses_in_the_header_and_in_the_library_with_sentinels_intact(what):
    s = _scene()
    kw = _refusals(s)[what]
    assert hc.args_ok(s, **kw) == -1, what
    # the library's host-array form: refused before a device is asked for, nothing written
    L = orb.load_library()
    a = dict(matches12=s["matches12"], sets=s["sets"], K=s["K"], params=hc.params_blob())
    a.update({k: v for k, v in kw.items() if k != "n_iter"})
    st = np.ascontiguousarray(a["sets"], I32).reshape(-1, 8)
    n_iter = kw.get("n_iter", len(st))
    rc, bufs = _library_call(L, s, a["matches12"], a["K"], a["params"], n_iter, st)
    assert rc == INVALID and _untouched(bufs), what


def _library_call(L, s, m12, K, params, n_iter, sets, null=()):
    p = lambda a, t: None if a is None else a.ctypes.data_as(C.POINTER(t))  # noqa: E731
    n1, N = len(s["xy1"]), 64
    bufs = dict(res=np.full(hc.RESULT_BYTES, 0xC3, U8), tri=np.full(n1, 0xAA, U8), x3d=np.full(3 * n1, -7.5, F32),
                in_h=np.full(N, 0xC3, U8), in_f=np.full(N, 0xC3, U8), sc_h=np.full(1100, -5.5, F32), sc_f=np.full(1100, -5.5, F32))
    keep = dict(xy1=np.ascontiguousarray(s["xy1"], F32), xy2=np.ascontiguousarray(s["xy2"], F32), m12=np.ascontiguousarray(m12, I32),
                K=np.ascontiguousarray(K, F32), sets=np.ascontiguousarray(sets, I32), params=params)
    for k in null:
        keep[k] = None
    rc = L.vsg_two_view_reconstruct(
        0, p(keep["xy1"], C.c_float), n1, p(keep["xy2"], C.c_float), len(s["xy2"]), p(keep["m12"], C.c_int32), p(keep["K"], C.c_float),
        None if keep["params"] is None else C.cast(keep["params"].ctypes.data, C.POINTER(orb.TwoViewParams)), n_iter,
        p(keep["sets"], C.c_int32), None if "res" in null else C.cast(bufs["res"].ctypes.data, C.POINTER(orb.TwoViewResult)),
        None if "tri" in null else p(bufs["tri"], C.c_uint8), None if "x3d" in null else p(bufs["x3d"], C.c_float),
        p(bufs["in_h"], C.c_uint8), p(bufs["in_f"], C.c_uint8), p(bufs["sc_h"], C.c_float), p(bufs["sc_f"], C.c_float))
    return rc, bufs


def _untouched(b):
    return (b["res"] == 0xC3).all() and (b["tri"] == 0xAA).all() and (b["x3d"] == F32(-7.5)).all() and (b["in_h"] == 0xC3).all() and \
        (b["in_f"] == 0xC3).all() and (b["sc_h"] == F32(-5.5)).all() and (b["sc_f"] == F32(-5.5)).all()


@pytest.mark.parametrize("null", ["xy1", "xy2", "m12", "K", "params", "sets", "res", "tri", "x3d"])
def test_null_arguments_are_refused_without_a_device_and_write_nothing(null):
    s = _scene()
    rc, bufs = _library_call(orb.load_library(), s, s["matches12"], s["K"], hc.params_blob(), len(s["sets"]), s["sets"], null=(null,))
    assert rc == INVALID and _untouched(bufs)


def test_null_frames_are_refused_without_a_device_and_write_nothing():
    L, s = orb.load_library(), _scene()
    res, tri, x3d = np.full(hc.RESULT_BYTES, 0xC3, U8), np.full(len(s["xy1"]), 0xAA, U8), np.full(3 * len(s["xy1"]), -7.5, F32)
    m12, K, st, pb = np.ascontiguousarray(s["matches12"], I32), np.ascontiguousarray(s["K"], F32), np.ascontiguousarray(s["sets"], I32), hc.params_blob()
    rc = L.vsg_frame_two_view_reconstruct(None, None, m12.ctypes.data_as(C.POINTER(C.c_int32)), K.ctypes.data_as(C.POINTER(C.c_float)),
                                          C.cast(pb.ctypes.data, C.POINTER(orb.TwoViewParams)), len(st), st.ctypes.data_as(C.POINTER(C.c_int32)),
                                          C.cast(res.ctypes.data, C.POINTER(orb.TwoViewResult)), tri.ctypes.data_as(C.POINTER(C.c_uint8)),
                                          x3d.ctypes.data_as(C.POINTER(C.c_float)), None, None, None, None)
    assert rc == INVALID and (res == 0xC3).all() and (tri == 0xAA).all() and (x3d == F32(-7.5)).all()
