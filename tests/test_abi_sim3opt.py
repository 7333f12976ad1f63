"""The C ABI of the Sim3 optimisation (include/vsg_orb.h: vsg_frame_optimize_sim3) without a device: the symbol, the
layout of vsg_sim3d / vsg_sim3_opt_result as the header declares them, the binding, and the argument errors that are
decided before a device is touched."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np

from visual_sgraphs_amd import orb

ROOT = Path(__file__).resolve().parent.parent
INVALID = -6


def test_symbol_is_exported_declared_and_bound():
    L = orb.load_library()
    header = (ROOT / "include" / "vsg_orb.h").read_text()
    assert hasattr(L, "vsg_frame_optimize_sim3") and re.search(r"\bint vsg_frame_optimize_sim3\(", header)
    assert "Optimizer.cc:3261-3529" in header and "one enqueue" in header and "base_binary_edge.hpp:131-205" in header
    assert hasattr(orb.Frame, "OptimizeSim3") and len(orb.SIM3_OPT_STATES) == 6
    adaptor = (ROOT / "include" / "vsg_orb_adaptor.hpp").read_text()
    assert "class ResidentSim3Optimizer" in adaptor and "vsg_frame_optimize_sim3(" in adaptor


def test_struct_layouts_match_the_header(tmp_path):
    src = tmp_path / "layout.c"
    fields = ("n_correspondences", "n_bad", "n_in", "n_in_kf2", "n_out_kf2", "more_iterations", "updated")
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vsg_orb.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu", sizeof(vsg_sim3d), offsetof(vsg_sim3d, t), offsetof(vsg_sim3d, s),\n'
                   '         sizeof(vsg_sim3_opt_result));\n' +
                   "".join('  printf(" %%zu", offsetof(vsg_sim3_opt_result, %s));\n' % f for f in fields) +
                   '  printf("\\n");\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", str(ROOT / "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    S, R = orb.Sim3d, orb.Sim3OptResult
    assert got == [C.sizeof(S), S.t.offset, S.s.offset, C.sizeof(R)] + [getattr(R, f).offset for f in fields]
    assert got == [64, 32, 56, 96, 64, 68, 72, 76, 80, 84, 88]


def test_argument_errors_need_no_device():
    L = orb.load_library()
    n = 4
    state, chi2, res = np.full(n, 9, np.uint8), np.full(2 * n, -3.0), orb.Sim3OptResult()
    slots, sig = np.zeros(n, np.int32), np.ones(8, np.float32)
    pose, S12 = orb.FramePose(), orb.Sim3d.make([0, 0, 0, 1], [0, 0, 0], 1.0)
    res.n_correspondences = -77
    ip, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    p = lambda a, t: a.ctypes.data_as(t)
    rc = L.vsg_frame_optimize_sim3(None, None, None, None, p(slots, ip), p(slots, ip), p(slots, ip), p(slots, ip),
                                   C.byref(pose), C.byref(pose), p(sig, fp), p(sig, fp), 8, C.byref(S12), 10.0, 0, 0,
                                   p(state, C.POINTER(C.c_uint8)), p(chi2, C.POINTER(C.c_double)), C.byref(res))
    assert rc == INVALID
    assert (state == 9).all() and (chi2 == -3).all() and res.n_correspondences == -77
