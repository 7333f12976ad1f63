"""The C ABI of global bundle adjustment (include/vsg_orb.h: vsg_mappoints_global_bundle_adjustment) without a device: the
symbol, the signature as the header, the kernel file, the binding and the adaptor have it, the layout of
vsg_global_ba_result, the refusals the header lists, the debug hooks, and the argument errors that are decided before a
device is touched."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np

import gba_hostcore as hc
from test_gba_hostmath import error_cases
from visual_sgraphs_amd import orb

ROOT = Path(__file__).resolve().parent.parent
ADAPTOR = ROOT / "tests" / "_adaptor_gba"
NAME = "vsg_mappoints_global_bundle_adjustment"
INVALID, UNSUPPORTED = -6, -3


def _declaration(text):
    m = re.search(r"\bint %s\((.*?)\);" % NAME, text, re.S)
    assert m
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    return [re.sub(r"\s+", " ", a).strip() for a in args.split(",")]


def _header_comment():
    header = (ROOT / "include" / "vsg_orb.h").read_text()
    end = header.index("typedef struct vsg_global_ba_result")
    return header[header.rindex("/*", 0, end):end]


def test_symbol_is_exported_declared_and_bound():
    L = orb.load_library()
    header = (ROOT / "include" / "vsg_orb.h").read_text()
    assert hasattr(L, NAME) and NAME in orb.EXPORTS
    args = _declaration(header)
    assert args == ["vsg_mappoints *mp", "int n_points", "const int32_t *slots", "const int32_t *obs_off", "const int32_t *obs_kf",
                    "const int32_t *obs_idx", "int n_kf", "vsg_frame *const *kfs", "const vsg_pose_se3 *kf_Tcw",
                    "const uint8_t *kf_fixed", "const vsg_ba_camera *kf_cam", "const float *inv_level_sigma2", "int nlevels",
                    "int iterations", "int robust", "int write_store", "const volatile uint8_t *stop_flag",
                    "vsg_pose_se3d *kf_Tcw_out", "float *world_pos_out", "uint8_t *included", "double *chi2",
                    "vsg_global_ba_result *res"]
    assert len(getattr(L, NAME).argtypes) == len(args) == 22
    assert _declaration((ROOT / "visual_sgraphs_amd" / "csrc" / "vsg_global_ba.hip").read_text().replace(") {", ");")) == args
    assert "vsg_global_ba.hip" in (ROOT / "visual_sgraphs_amd" / "build.py").read_text()
    assert hasattr(orb.MapPoints, "GlobalBundleAdjustment")


def test_header_comment_cites_the_reference_and_states_every_refusal():
    text = _header_comment()
    for ref in ("Optimizer.cc:60-287", ":500-610", ":45-58", "Tracking.cc:2652", "LoopClosing.cc:2157", ":126", ":166-169", ":174", ":204",
                ":189", ":221", "5.99", ":278-286", ":516", ":600", ":529-584", ":289-498", ":612-640", "INTEGRATION.md"):
        assert ref in text, ref
    for refusal in ("robust or write_store outside {0, 1}", "write_store == 0 with", "NULL world_pos_out", "NULL included",
                    "VSG_ERR_UNSUPPORTED", "Nleft != -1", "no optimised keyframe", "more than 512 optimised keyframes",
                    "3072 rows", "75.5 MB", "waits for its stream"):
        assert refusal in re.sub(r"\s*\n \*\s*", " ", text), refusal
    cap = hc.geometry()[2]
    assert cap == 512  # the number the header states


def test_result_layout_matches_the_header(tmp_path):
    header = (ROOT / "include" / "vsg_orb.h").read_text()
    m = re.search(r"typedef struct vsg_global_ba_result \{(.*?)\} vsg_global_ba_result;", header, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = [n.strip() for part in re.findall(r"(?:int32_t|double)\s+([^;]+);", body) for n in part.split(",")]
    assert tuple(names) == hc.RES_INTS + hc.RES_DOUBLES == orb.GLOBAL_BA_RESULT_INTS + orb.GLOBAL_BA_RESULT_DOUBLES
    assert "n_erase" not in names and set(names) | {"n_erase"} == set(orb.LOCAL_BA_RESULT_INTS + orb.LOCAL_BA_RESULT_DOUBLES)
    src = tmp_path / "layout.c"
    fields = hc.RES_INTS + hc.RES_DOUBLES
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vsg_orb.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(vsg_global_ba_result));\n' +
                   "".join('  printf(" %%zu", offsetof(vsg_global_ba_result, %s));\n' % f for f in fields) +
                   '  printf("\\n");\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", str(ROOT / "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    for R in (orb.GlobalBaResult, hc.GlobalBaResult):
        assert got == [C.sizeof(R)] + [getattr(R, f).offset for f in fields]
    assert got == [64] + [4 * i for i in range(10)] + [40, 48, 56]


def test_debug_hooks_are_declared_exported_and_refuse_without_a_device():
    L = orb.load_library()
    text = (ROOT / "include" / "vsg_orb_debug_global_ba.h").read_text()
    assert "int vsg_debug_ba_reduced_solve(int n, const double *M, const double *b, double *x, int *ok);" in text
    assert "int vsg_debug_ba_solver_geometry(int *panel, int *tile);" in text
    assert "vsg_debug_ba_" not in (ROOT / "include" / "vsg_orb.h").read_text()
    assert "vsg_orb_debug_global_ba.h" not in (ROOT / "INTEGRATION.md").read_text()
    assert orb.debug_ba_solver_geometry() == hc.geometry()[:2]
    assert L.vsg_debug_ba_solver_geometry(None, None) == INVALID
    x, ok = np.full(4, -3.0), C.c_int32(7)
    p = x.ctypes.data_as(C.POINTER(C.c_double))
    for n, M, b, xo, o in ((0, p, p, p, C.byref(ok)), (6 * 512 + 1, p, p, p, C.byref(ok)), (2, None, p, p, C.byref(ok)),
                           (2, p, None, p, C.byref(ok)), (2, p, p, None, C.byref(ok)), (2, p, p, p, None)):
        assert L.vsg_debug_ba_reduced_solve(n, M, b, xo, o) == INVALID
    assert ok.value == 7 and (x == -3.0).all()


def test_cpp_adaptor_compiles_and_fails_loudly_without_device():
    L = orb.load_library()
    subprocess.check_call(["make", "-C", str(ADAPTOR)], stdout=subprocess.DEVNULL)
    adaptor = (ROOT / "include" / "vsg_orb_adaptor.hpp").read_text()
    for name in ("GlobalBAResult GlobalBundleAdjustment(", "struct GlobalBAResult", NAME + "(", "nIterations", "pbStopFlag", "bRobust"):
        assert name in adaptor, name
    m = re.search(r"check\(%s\((.*?)\),\s*\"%s\"\)" % (NAME, NAME), adaptor, re.S)
    assert m and len(m.group(1).split(",")) == 22  # the adaptor passes the header's twenty-two arguments
    if L.vsg_device_count() <= 0:
        r = subprocess.run([str(ADAPTOR / "gba_check"), "/dev/null", "/dev/null"], capture_output=True, text=True)
        assert r.returncode == 3 and "no CPU fallback" in r.stdout


def test_every_refusal_of_the_header_is_a_case_of_the_tests():
    """The refusals the header lists are the cases test_gba_hostmath.py runs on the host build (which shares the check with
    the library) and test_gpu_global_bundle_adjustment.py runs on the device; each returns its code and writes nothing."""
    _, cases = error_cases()
    for case in ("null_slots", "null_obs_off", "null_obs_kf", "null_obs_idx", "null_Tcw", "null_fixed", "null_cam", "null_sigma",
                 "null_kf_out", "null_included", "null_res", "null_pos_out_without_write_store", "off_not_from_zero", "off_descends",
                 "kf_negative", "kf_past_end", "idx_negative", "idx_past_end", "slot_negative", "slot_past_end", "slot_twice",
                 "nlevels_0", "nlevels_17", "octave_past_nlevels", "iterations_0", "iterations_101", "robust_2", "robust_negative",
                 "write_store_2", "write_store_negative", "nleft", "edges_on_fixed_alone"):
        assert case in cases, case
    assert {c for _, c in cases.values()} == {INVALID, UNSUPPORTED}


def test_argument_errors_need_no_device():
    """What the library decides before it looks for a device: a NULL store and the NULL outs."""
    L = orb.load_library()
    res = orb.GlobalBaResult()
    res.ran = -77
    kf_out, inc, pos = np.full(7, -3.0), np.full(4, 9, np.uint8), np.full(12, -3.0, np.float32)
    slots, sig = np.zeros(4, np.int32), np.ones(8, np.float32)
    ip, fp, bp = C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_uint8)
    p = lambda a, t: a.ctypes.data_as(t)
    rc = L.vsg_mappoints_global_bundle_adjustment(None, 4, p(slots, ip), p(slots, ip), p(slots, ip), p(slots, ip), 0, None, None,
                                                  None, None, p(sig, fp), 8, 10, 0, 0, None,
                                                  C.cast(kf_out.ctypes.data, C.POINTER(orb.PoseSE3d)), p(pos, fp), p(inc, bp), None,
                                                  C.byref(res))
    assert rc == INVALID and (kf_out == -3).all() and (inc == 9).all() and (pos == -3).all() and res.ran == -77
