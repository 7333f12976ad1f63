"""The C ABI of the local-map chain call (include/vsg_orb.h: vsg_frame_track_local_map) without a device: the symbol, its
prototype, the layout of vsg_track_local_result as the header declares it, the reference lines and deviations its comment
states, and the refusals that are decided before a device is touched (those that need handles:
tests/test_gpu_track_local_map.py)."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np

from visual_sgraphs_amd import orb

ROOT = Path(__file__).resolve().parent.parent
INVALID = -6
NAME = "vsg_frame_track_local_map"


def test_symbol_is_declared_exported_and_bound():
    L = orb.load_library()
    header = (ROOT / "include" / "vsg_orb.h").read_text()
    assert hasattr(L, NAME) and re.search(r"\bint %s\(" % NAME, header) and NAME in orb.EXPORTS
    assert len(getattr(L, NAME).argtypes) == 27 and callable(orb.Frame.TrackLocalMap)
    comment = header[:header.index("typedef struct vsg_track_local_result")].rsplit("/*", 1)[1]
    for cited in ("Tracking.cc:3019-3131", ":3446-3466", "ORBmatcher.cc:42-143", ":3041", ":3074-3095", ":3426-3443",
                  "ORBmatcher.cc:86-88", ":3093", "Optimizer.cc:1251", "ONE enqueue", "DEVIATIONS", "EVERY feature",
                  "VSG_ERR_CAPACITY", "WHAT STAYS WITH THE CALLER", "UpdateLocalMap", "IncreaseVisible", "IncreaseFound"):
        assert cited in comment, cited
    # the calls it chains keep their signatures
    assert len(L.vsg_frame_search_local_points.argtypes) == 19 and len(L.vsg_frame_pose_optimization.argtypes) == 15
    assert len(L.vsg_frame_track_with_motion_model.argtypes) == 20


def test_struct_layout_matches_the_header(tmp_path):
    fields = [k for k, _ in orb.TrackLocalResult._fields_]
    assert fields == ["pose", "n_to_match", "n_matches_searched", "n_matches_inliers", "walk_rounds"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vsg_orb.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(vsg_track_local_result));\n' +
                   "".join('  printf(" %%zu", offsetof(vsg_track_local_result, %s));\n' % k for k in fields) +
                   '  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", str(ROOT / "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [C.sizeof(orb.TrackLocalResult)] + [getattr(orb.TrackLocalResult, k).offset for k in fields]
    assert got == [88, 0, 72, 76, 80, 84]


def test_refusals_need_no_device():
    L = orb.load_library()
    n = 4
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    slots, fin, sf, sig = np.zeros(n, np.int32), np.full(n, -1, np.int32), np.ones(8, np.float32), np.ones(8, np.float32)
    cp, se3 = orb.FramePose(), orb.PoseSE3()

    def call(hold=-1, nlevels=8, tcw=True, sigma=True, fin_=True, fs=True, out=True, res=True):
        f, tm, o, c2, r = np.full(n, -5, np.int32), np.full(n, -5, np.int32), np.full(n, 9, np.uint8), \
            np.full(n, -3, np.float32), orb.TrackLocalResult()
        iv, px, py = np.full(n, 9, np.uint8), np.full(n, -3, np.float32), np.full(n, -3, np.float32)
        r.n_to_match = -77
        rc = L.vsg_frame_track_local_map(
            None, None, n, p(slots, C.c_int32), None, C.byref(cp), 0.5, 3.0, 0.8, 0, 0.0, p(sf, C.c_float), nlevels,
            p(fin, C.c_int32) if fin_ else None, C.byref(se3) if tcw else None, p(sig, C.c_float) if sigma else None, hold,
            0, 0, p(f, C.c_int32) if fs else None, p(tm, C.c_int32), p(o, C.c_uint8) if out else None, p(c2, C.c_float),
            p(iv, C.c_uint8), p(px, C.c_float), p(py, C.c_float), C.byref(r) if res else None)
        # nothing is written by a refused call
        assert (f == -5).all() and (tm == -5).all() and (o == 9).all() and (c2 == -3).all() and r.n_to_match == -77
        assert (iv == 9).all() and (px == -3).all() and (py == -3).all()
        return rc

    assert call() == INVALID  # NULL handles
    for kw in (dict(hold=0), dict(hold=1), dict(hold=3), dict(nlevels=0), dict(nlevels=17), dict(tcw=False),
               dict(sigma=False), dict(fin_=False), dict(fs=False), dict(out=False), dict(res=False)):
        assert call(**kw) == INVALID, kw
