"""The C ABI of the chain call (include/vsg_orb.h: vsg_frame_track_with_motion_model) without a device: the symbol, its
prototype, the layout of vsg_track_result as the header declares it, the reference lines its comment cites, and the
refusals that are decided before a device is touched (those that need handles: tests/test_gpu_track_motion_model.py)."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np

from visual_sgraphs_amd import orb

ROOT = Path(__file__).resolve().parent.parent
INVALID = -6
NAME = "vsg_frame_track_with_motion_model"


def test_symbol_is_declared_exported_and_bound():
    L = orb.load_library()
    header = (ROOT / "include" / "vsg_orb.h").read_text()
    assert hasattr(L, NAME) and re.search(r"\bint %s\(" % NAME, header) and NAME in orb.EXPORTS
    assert len(getattr(L, NAME).argtypes) == 20 and callable(orb.Frame.TrackWithMotionModel)
    comment = header[:header.index("typedef struct vsg_track_result")].rsplit("/*", 1)[1]
    for cited in ("Tracking.cc:2945-3005", ":2958-2963", ":2967", ":2980-3005", "Optimizer.cc:1109-1180", "ONE enqueue"):
        assert cited in comment, cited
    assert "Future work" not in header
    # the calls it chains keep their signatures
    assert len(L.vsg_frame_search_last_frame.argtypes) == 19 and len(L.vsg_frame_pose_optimization.argtypes) == 15


def test_struct_layout_matches_the_header(tmp_path):
    fields = [k for k, _ in orb.TrackResult._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vsg_orb.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(vsg_track_result));\n' +
                   "".join('  printf(" %%zu", offsetof(vsg_track_result, %s));\n' % k for k in fields) +
                   '  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", str(ROOT / "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [C.sizeof(orb.TrackResult)] + [getattr(orb.TrackResult, k).offset for k in fields]
    assert got == [104, 0, 72, 76, 80, 84, 88, 92, 96, 100]


def test_the_walk_hook_is_a_debug_symbol_and_refuses_without_a_device():
    """vsg_debug_track_walk (k_track_walk alone): declared in include/vsg_orb_debug.h, exported by the shipped library, no
    part of the boundary a maintainer binds; NULL, negative and out-of-range arguments and a shape over the LDS cap are
    refused before a device is touched, with nothing written."""
    import walk_cases as wc
    L, hook = orb.load_library(), "vsg_debug_track_walk"
    assert re.search(r"\bint %s\(" % hook, (ROOT / "include" / "vsg_orb_debug.h").read_text())
    assert hasattr(L, hook) and hook in orb.EXPORTS and len(getattr(L, hook).argtypes) == len(orb.WALK_ARGS) == 27
    assert hook not in (ROOT / "include" / "vsg_orb.h").read_text() and hook not in (ROOT / "INTEGRATION.md").read_text()
    assert "vsg_orb_debug.h" not in (ROOT / "INTEGRATION.md").read_text()
    c = wc.directed_high()["from_slots_50"]
    pos = {k: i for i, k in enumerate(orb.WALK_ARGS)}

    def raw(case=c, table=c["slot_observed"], **replace):
        args, out, keep = orb.debug_track_walk_args(case, slot_observed=table)
        for k, v in replace.items():
            args[pos[k]] = v
        rc = L.vsg_debug_track_walk(*args)
        if rc < 0:  # nothing is written by a refused call
            assert all((out[k] == orb.WALK_SENTINEL_I32).all() for k in ("tm", "feat_slots", "edges_feat", "edges_slot", "status"))
            assert all((out[k] == orb.WALK_SENTINEL_U8).all() for k in ("tb", "feat_observed"))
        return rc

    for k in ("ent", "off", "cnt", "q_angle", "t_angle", "train_match", "train_blocked", "feat_slots", "feat_observed",
              "edge_feat", "edge_slot", "status"):
        assert raw(**{k: None}) == INVALID, k
    for k in ("nq", "nf", "n_ent", "cap", "n_slots"):
        assert raw(**{k: -1}) == INVALID, k
    assert raw(nf=32769) == INVALID and raw(form=2) == INVALID and raw(form=-1) == INVALID
    bad = c["q_slot"].copy()
    bad[-1] = len(c["slot_observed"])
    assert raw(case=dict(c, q_slot=bad)) == INVALID
    bad = c["slots_in"].copy()
    bad[0] = -2
    assert raw(case=dict(c, slots_in=bad)) == INVALID
    for name in sorted(wc.OVER_CAP_SHAPES):  # VSG_ERR_CAPACITY, by the chain calls' expression
        assert raw(case=wc.cap_cases()[name], table=None) == -2, name
    if L.vsg_device_count() <= 0:  # the same call with valid arguments gets as far as the device
        assert raw() == -4 and raw(case=wc.cap_cases()["cap_queries"], table=None) == -4


def test_refusals_need_no_device():
    L = orb.load_library()
    n = 4
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    slots, sf, sig = np.zeros(n, np.int32), np.ones(8, np.float32), np.ones(8, np.float32)
    cp, lp, se3 = orb.FramePose(), orb.FramePose(), orb.PoseSE3()

    def call(hold=-1, tcw=True, sigma=True, fs=True, out=True, res=True):
        f, tm, o, c2, r = np.full(n, -5, np.int32), np.full(n, -5, np.int32), np.full(n, 9, np.uint8), \
            np.full(n, -3, np.float32), orb.TrackResult()
        r.n_search = -77
        rc = L.vsg_frame_track_with_motion_model(
            None, None, None, p(slots, C.c_int32), C.byref(cp), C.byref(lp), 0.08, 0, 15.0, p(sf, C.c_float), 8, 1,
            C.byref(se3) if tcw else None, p(sig, C.c_float) if sigma else None, hold, p(f, C.c_int32) if fs else None,
            p(tm, C.c_int32), p(o, C.c_uint8) if out else None, p(c2, C.c_float), C.byref(r) if res else None)
        # nothing is written by a refused call
        assert (f == -5).all() and (tm == -5).all() and (o == 9).all() and (c2 == -3).all() and r.n_search == -77
        return rc

    assert call() == INVALID  # NULL handles
    for kw in (dict(hold=0), dict(hold=1), dict(hold=3), dict(tcw=False), dict(sigma=False), dict(fs=False),
               dict(out=False), dict(res=False)):
        assert call(**kw) == INVALID, kw
