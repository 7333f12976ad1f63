"""The C ABI of the local bundle adjustment with planes and rooms (include/vsg_orb.h:
vsg_mappoints_local_bundle_adjustment_sgraph) without a device: the symbol, the signature as the header, the kernel file, the
binding and the adaptor have it, the layout of vsg_sgraph_local_ba_result, and the argument errors that are decided before a
device is touched."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np

import sgba_hostcore as sh
from visual_sgraphs_amd import orb

ROOT = Path(__file__).resolve().parent.parent
ADAPTOR = ROOT / "tests" / "_adaptor_sgba"
NAME = "vsg_mappoints_local_bundle_adjustment_sgraph"
VISUAL = "vsg_mappoints_local_bundle_adjustment"
INVALID = -6


def _declaration(text, name):
    m = re.search(r"\bint %s\((.*?)\);" % name, text, re.S)
    assert m
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    return [re.sub(r"\s+", " ", a).strip() for a in args.split(",")]


def test_symbol_is_exported_declared_and_bound():
    L = orb.load_library()
    header = (ROOT / "include" / "vsg_orb.h").read_text()
    assert hasattr(L, NAME) and NAME in orb.EXPORTS
    args, visual = _declaration(header, NAME), _declaration(header, VISUAL)
    # the visual call's arguments in its order (its res excluded: the new struct holds it), then the new ones
    assert args[:19] == visual[:19]
    assert args[19:] == ["int n_planes", "const double *plane_eq", "const int32_t *pl_obs_off", "const int32_t *pl_obs_kf",
                         "const double *pl_obs_local", "const double *pl_obs_G", "const double *w_plane_kf",
                         "const double *w_plane_point", "int n_rooms", "const double *room_center", "const int32_t *room_n_walls",
                         "const int32_t *room_wall", "double *plane_eq_out", "double *room_center_out", "uint8_t *erase_plane",
                         "double *chi2_plane_kf", "double *chi2_plane_point", "vsg_sgraph_local_ba_result *res"]
    assert len(getattr(L, NAME).argtypes) == len(args) == 37
    for ref in ("Optimizer.cc:2018-2130", ":2155-2214", ":2342-2369", ":2426-2441", ":2277", ":2198", "768 rows", "marginalize_planes",
                "plane_map_point"):
        assert ref in header, ref
    assert hasattr(orb.MapPoints, "LocalBundleAdjustmentSGraph") and orb.SGRAPH_LOCAL_BA_MAX_ROWS == 768
    assert _declaration((ROOT / "visual_sgraphs_amd" / "csrc" / "vsg_sgraph_ba.hip").read_text().replace(") {", ");"), NAME) == args
    assert "vsg_sgraph_ba.hip" in (ROOT / "visual_sgraphs_amd" / "build.py").read_text()
    # the visual entry's comment points at the new one
    assert "vsg_mappoints_local_bundle_adjustment_sgraph below" in header


def test_struct_layout_matches_the_header(tmp_path):
    header = (ROOT / "include" / "vsg_orb.h").read_text()
    m = re.search(r"typedef struct vsg_sgraph_local_ba_result \{(.*?)\} vsg_sgraph_local_ba_result;", header, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = [n.strip() for part in re.findall(r"int32_t\s+([^;]+);", body) for n in part.split(",")]
    assert tuple(names) == sh.SEM_INTS == orb.SGRAPH_LOCAL_BA_RESULT_INTS and "vsg_local_ba_result local;" in body
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vsg_orb.h"\nint main(void) {\n'
                   '  printf("%zu %zu", sizeof(vsg_sgraph_local_ba_result), offsetof(vsg_sgraph_local_ba_result, local));\n' +
                   "".join('  printf(" %%zu", offsetof(vsg_sgraph_local_ba_result, %s));\n' % f for f in sh.SEM_INTS) +
                   '  printf("\\n");\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", str(ROOT / "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    for R in (orb.SGraphLocalBaResult, sh.SGraphLocalBaResult):
        assert got == [C.sizeof(R), R.local.offset] + [getattr(R, f).offset for f in sh.SEM_INTS]
    assert got == [104, 0] + [72 + 4 * i for i in range(8)]


def test_cpp_adaptor_compiles_and_fails_loudly_without_device():
    L = orb.load_library()
    subprocess.check_call(["make", "-C", str(ADAPTOR)], stdout=subprocess.DEVNULL)
    adaptor = (ROOT / "include" / "vsg_orb_adaptor.hpp").read_text()
    for name in ("SGraphLocalBAResult LocalBundleAdjustmentSGraph(", "struct SGraphLocalBAResult", "struct SGraphLists", NAME + "("):
        assert name in adaptor, name
    m = re.search(r"check\(%s\((.*?)\),\s*\"%s\"\)" % (NAME, NAME), adaptor, re.S)
    assert m and len(m.group(1).split(",")) == 37  # the adaptor passes the header's thirty-seven arguments
    if L.vsg_device_count() <= 0:
        r = subprocess.run([str(ADAPTOR / "sgba_check"), "/dev/null", "/dev/null"], capture_output=True, text=True)
        assert r.returncode == 3 and "no CPU fallback" in r.stdout


def test_argument_errors_need_no_device():
    L = orb.load_library()
    res = orb.SGraphLocalBaResult()
    res.n_rows = -77
    kf_out, erase, plane_out = np.full(7, -3.0), np.full(4, 9, np.uint8), np.full(4, -3.0)
    slots, sig, eq = np.zeros(4, np.int32), np.ones(8, np.float32), np.array([1.0, 0.0, 0.0, 2.0])
    ip, fp, dp = C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_double)
    p = lambda a, t: a.ctypes.data_as(t)
    rc = getattr(L, NAME)(None, 4, p(slots, ip), p(slots, ip), p(slots, ip), p(slots, ip), 0, None, None, None, None, p(sig, fp), 8,
                          10, None, C.cast(kf_out.ctypes.data, C.POINTER(orb.PoseSE3d)), None, p(erase, C.POINTER(C.c_uint8)), None,
                          1, p(eq, dp), p(slots, ip), None, None, None, None, None, 0, None, None, None, p(plane_out, dp), None, None,
                          None, None, C.byref(res))
    assert rc == INVALID and (kf_out == -3).all() and (erase == 9).all() and (plane_out == -3).all() and res.n_rows == -77
