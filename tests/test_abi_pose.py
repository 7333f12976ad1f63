"""The C ABI of the pose optimisation (include/vsg_orb.h: vsg_frame_pose_optimization / _resume) without a device: the
symbols, the layout of vsg_pose_se3 / vsg_pose_result as the header declares them, and the argument errors that are
decided before a device is touched."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np

from visual_sgraphs_amd import orb

ROOT = Path(__file__).resolve().parent.parent
INVALID = -6


def test_symbols_are_exported_and_declared():
    L = orb.load_library()
    header = (ROOT / "include" / "vsg_orb.h").read_text()
    for name in ("vsg_frame_pose_optimization", "vsg_frame_pose_optimization_resume"):
        assert hasattr(L, name) and re.search(r"\bint %s\(" % name, header), name
    assert "Optimizer.cc:1063-1452" in header and "one enqueue" in header


def test_struct_layouts_match_the_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vsg_orb.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(vsg_pose_se3), offsetof(vsg_pose_se3, t),\n'
                   '         sizeof(vsg_pose_result), offsetof(vsg_pose_result, t), offsetof(vsg_pose_result, n_initial),\n'
                   '         offsetof(vsg_pose_result, n_bad), offsetof(vsg_pose_result, rounds_run),\n'
                   '         offsetof(vsg_pose_result, held), offsetof(vsg_pose_result, q));\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", str(ROOT / "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    P, R = orb.PoseSE3, orb.PoseResult
    assert got == [C.sizeof(P), P.t.offset, C.sizeof(R), R.t.offset, R.n_initial.offset, R.n_bad.offset,
                   R.rounds_run.offset, R.held.offset, R.q.offset]
    assert got == [28, 16, 72, 32, 56, 60, 64, 68, 0]


def test_argument_errors_need_no_device():
    L = orb.load_library()
    out, chi2, res, pose = np.full(4, 9, np.uint8), np.full(4, -3, np.float32), orb.PoseResult(), orb.PoseSE3()
    slots, sig = np.zeros(4, np.int32), np.ones(8, np.float32)
    res.n_initial = -77
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    rc = L.vsg_frame_pose_optimization(None, None, p(slots, C.c_int32), C.byref(pose), 500.0, 500.0, 320.0, 240.0, 40.0,
                                       p(sig, C.c_float), 8, -1, p(out, C.c_uint8), p(chi2, C.c_float), C.byref(res))
    assert rc == INVALID
    assert L.vsg_frame_pose_optimization_resume(None, None, p(out, C.c_uint8), p(chi2, C.c_float), C.byref(res)) == INVALID
    assert (out == 9).all() and (chi2 == -3).all() and res.n_initial == -77
