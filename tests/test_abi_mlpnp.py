"""The C ABI of MLPnPsolver on a resident frame (include/vsg_orb.h: vsg_frame_mlpnp_ransac, vsg_mlpnp_ransac_parameters,
vsg_mlpnp_draw_sets) without a device: the symbols, the layout of vsg_mlpnp_result as the header declares it, and the
refusals.  A frame cannot exist without a device, so the library itself is asked only what it decides on the handles; every
other check is mlpnp::args_ok of csrc/vsg_mlpnp.h -- the function the entry point calls before it touches a device -- through
the host build.  tests/test_gpu_mlpnp.py repeats each refusal on a real frame and store."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import mlpnp_hostcore as hc
import mlpnp_scenes as ms
from visual_sgraphs_amd import orb

ROOT = Path(__file__).resolve().parent.parent
INVALID = -6
F32, F64, I32, U8 = np.float32, np.float64, np.int32, np.uint8


def test_symbols_are_exported_declared_and_bound():
    L = orb.load_library()
    header = (ROOT / "include" / "vsg_orb.h").read_text()
    for name, nargs in (("vsg_frame_mlpnp_ransac", 20), ("vsg_mlpnp_ransac_parameters", 8), ("vsg_mlpnp_draw_sets", 5)):
        assert hasattr(L, name) and re.search(r"\bint %s\(" % name, header) and name in orb.EXPORTS, name
        assert len(getattr(L, name).argtypes) == nargs
        decl = header[header.index("int %s(" % name):]
        decl = decl[:decl.index(";")].replace("int (*random_int)(int lo, int hi, void *ctx)", "random_int")  # one argument
        assert decl.count(",") + 1 == nargs, name
    for cite in ("MLPnPsolver.cpp", "Tracking.cc:3735", ":231-267", ":125-145", "One enqueue", "VSG_ERR_UNSUPPORTED"):
        assert cite in header, cite
    assert callable(orb.Frame.mlpnp_ransac) and callable(orb.mlpnp_ransac_parameters) and callable(orb.mlpnp_draw_sets)
    # the entry point's checks come before the thread's context is asked for, and that before any launch
    src = (ROOT / "visual_sgraphs_amd" / "csrc" / "vsg_mlpnp.hip").read_text()
    body = src[src.index("int vsg_frame_mlpnp_ransac("):]
    assert body.index("mlpnp::args_ok(") < body.index("thread_ctx(") < body.index("hipLaunchKernelGGL(")


def test_result_layout_matches_the_header(tmp_path):
    fields = ("Tcw", "found", "no_more", "n_inliers", "refined", "best_hypothesis", "iterations", "n_correspondences", "n_records")
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vsg_orb.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(vsg_mlpnp_result));\n' +
                   "".join('  printf(" %%zu", offsetof(vsg_mlpnp_result, %s));\n' % f for f in fields) + '  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", str(ROOT / "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    T = orb.MlpnpResult
    assert got == [C.sizeof(T)] + [getattr(T, f).offset for f in fields]
    assert got == [hc.RESULT_BYTES, 0, 64, 68, 72, 76, 80, 84, 88, 92]


def test_null_handles_are_refused_without_a_device_and_write_nothing():
    L = orb.load_library()
    nf, nh = 8, 2
    sl, sg = np.arange(nf, dtype=I32), np.ones(8, F32)
    sm = np.array([0, 1, 2, 3, 4, 5, 7, 6, 5, 4, 3, 2], I32)
    inl, res, hcnt, hT = np.full(nf, 7, U8), orb.MlpnpResult(), np.full(nh, -3, I32), np.full(12 * nh, -2.0, F64)
    res.iterations = -44
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))  # noqa: E731
    rc = L.vsg_frame_mlpnp_ransac(None, None, p(sl, C.c_int32), 500.0, 500.0, 320.0, 240.0, p(sg, C.c_float), 8, 5.991, 6, 2, 0, 2, nh,
                                  p(sm, C.c_int32), p(inl, C.c_uint8), C.byref(res), p(hcnt, C.c_int32), p(hT, C.c_double))
    assert rc == INVALID
    assert (inl == 7).all() and res.iterations == -44 and (hcnt == -3).all() and (hT == -2).all()


@pytest.fixture(scope="module")
def scene():
    return ms.make(3, n=40, n_hyp=9)


def call(s, **kw):
    a = dict(nlevels=ms.NLEVELS, th2=ms.TH2, min_inliers=10, max_its=9, first=0, n_iterations=5, sets=s["sets"])
    a.update(kw)
    return hc.args_ok(s, ms.CAM, ms.LEVEL_SIGMA2, a.pop("nlevels"), a.pop("th2"), a.pop("min_inliers"), a.pop("max_its"), a.pop("first"),
                      a.pop("n_iterations"), a.pop("sets"), **a)


def edit(a, i, v):
    a = np.array(a, copy=True)
    a.reshape(-1)[i] = v
    return a


def test_the_argument_check(scene):
    s = scene
    used = np.flatnonzero(s["slots"] >= 0)
    assert call(s) == (True, 40)
    refused = {
        "slots NULL": dict(slots=None), "level_sigma2 NULL": dict(level_sigma2=None), "sets NULL": dict(sets=None, n_hyp=9),
        "inlier NULL": dict(inlier=False), "res NULL": dict(res=False), "slot == capacity": dict(slots=edit(s["slots"], used[2], s["capacity"])),
        "nlevels 0": dict(nlevels=0), "nlevels 17": dict(nlevels=17), "an octave == nlevels": dict(nlevels=int(s["octave"][used].max())),
        "an octave < 0": dict(octave=edit(s["octave"], used[0], -1)), "th2 0": dict(th2=0.0), "th2 < 0": dict(th2=-2.0),
        "th2 nan": dict(th2=float("nan")), "th2 inf": dict(th2=float("inf")), "min_inliers 5": dict(min_inliers=5), "max_its 0": dict(max_its=0),
        "first < 0": dict(first=-1), "n_iterations < 0": dict(n_iterations=-1), "n_hyp 0": dict(n_hyp=0),
        "n_hyp 1025": dict(sets=np.tile(s["sets"][:1], (1025, 1))), "max_its > n_hyp": dict(max_its=10),
        "first + n_iterations > n_hyp": dict(first=5, n_iterations=5), "sample == n": dict(sets=edit(s["sets"], 4, 40)),
        "sample < 0": dict(sets=edit(s["sets"], 50, -1)), "equal samples": dict(sets=edit(s["sets"], 1, s["sets"][0, 0])),
    }
    for what, kw in refused.items():
        assert call(s, **kw)[0] is False, what
    # an unused feature's octave and slot < 0 are not looked at; n < min_inliers leaves the sets unread
    free = np.flatnonzero(s["slots"] < 0)
    assert call(s, octave=edit(s["octave"], free[0], 99), slots=edit(s["slots"], free[1], -7)) == (True, 40)
    assert call(s, min_inliers=41, sets=edit(s["sets"], 4, 40)) == (True, 40)
    assert call(s, n_hyp=1024, max_its=1024, sets=np.tile(s["sets"][:1], (1024, 1))) == (True, 40)
    assert call(s, first=9, n_iterations=0) == (True, 40) and call(s, first=4, n_iterations=5) == (True, 40)
