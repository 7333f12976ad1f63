"""The C ABI of CreateNewMapPoints on resident keyframes (include/vsg_orb.h: vsg_frame_set_stereo_points,
vsg_frame_triangulate_matches, vsg_frame_create_new_map_points) without a device: the symbols, the layout of
vsg_triangulation_params as the header declares it, the codes shared with csrc/vsg_triangulate.h, and the argument errors that are
decided before a device is touched, with the outputs untouched."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np

import triangulation_reference as tr
from visual_sgraphs_amd import orb

ROOT = Path(__file__).resolve().parent.parent
INVALID = -6
NAMES = ("vsg_frame_set_stereo_points", "vsg_frame_triangulate_matches", "vsg_frame_create_new_map_points")


def test_symbols_are_exported_declared_and_bound():
    L = orb.load_library()
    header = (ROOT / "include" / "vsg_orb.h").read_text()
    for name, nargs in zip(NAMES, (3, 17, 32)):
        assert hasattr(L, name) and re.search(r"\bint %s\(" % name, header) and name in orb.EXPORTS, name
        assert len(getattr(L, name).argtypes) == nargs
        decl = header[header.index("int %s(" % name):]
        assert decl[:decl.index(";")].count(",") + 1 == nargs, name
    for cite in ("LocalMapping.cc:382-710", "GeometricTools.cc:47-66", "KeyFrame.cc:\n * 885-902", ":663", "kf2_first",
                 "VSG_ERR_UNSUPPORTED", "One enqueue", "drops it"):
        assert cite in header, cite
    assert callable(orb.Frame.SetStereoPoints) and callable(orb.Frame.TriangulateMatches) and callable(orb.Frame.CreateNewMapPoints)


def test_reason_and_source_codes_are_the_shared_sources():
    header = (ROOT / "include" / "vsg_orb.h").read_text()
    core = (ROOT / "visual_sgraphs_amd" / "csrc" / "vsg_triangulate.h").read_text()
    pub = {k: int(v) for k, v in re.findall(r"#define VSG_TRI_([A-Z0-9_]+) (\d+)", header)}
    src = {k: int(v) for k, v in re.findall(r"kTri([A-Za-z0-9]+) = (\d+)", core) if k != "Sweeps"}
    norm = lambda d: {k.replace("_", "").lower(): v for k, v in d.items()}  # noqa: E731
    assert norm(pub) == norm(src) and len(pub) == 16
    for i, name in enumerate(orb.TRI_REASONS):
        assert pub[name.upper()] == i == getattr(tr, name.upper())
    assert pub["NO_MATCH"] == orb.TRI_NO_MATCH == tr.NO_MATCH == 255
    assert (pub["FROM_TRIANGULATE"], pub["FROM_STEREO1"], pub["FROM_STEREO2"]) == (0, 1, 2)


def test_params_layout_matches_the_header(tmp_path):
    fields = ("kf1", "kf2", "ratio_factor", "th_far_points", "inertial", "far_points", "kf2_first")
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vsg_orb.h"\nint main(void) {\n'
                   '  printf("%zu %zu", sizeof(vsg_triangulation_params), sizeof(vsg_frame_pose));\n' +
                   "".join('  printf(" %%zu", offsetof(vsg_triangulation_params, %s));\n' % f for f in fields) +
                   '  printf(" %zu\\n", offsetof(vsg_frame_pose, mbf));\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", str(ROOT / "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    T = orb.TriangulationParams
    assert got == [C.sizeof(T), C.sizeof(orb.FramePose)] + [getattr(T, f).offset for f in fields] + [orb.FramePose.mbf.offset]
    assert got == [196, 88, 0, 88, 176, 180, 184, 188, 192, 76]


def test_argument_errors_need_no_device():
    L = orb.load_library()
    n = 4
    reason, source = np.full(n, 9, np.uint8), np.full(n, 8, np.uint8)
    x3d, slot, m12 = np.full(3 * n, -3, np.float32), np.full(n, -5, np.int32), np.full(n, 6, np.int32)
    created = C.c_int32(-77)
    tab, free, flags = np.ones(8, np.float32), np.zeros(2, np.int32), np.ones(n, np.uint8)
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))  # noqa: E731
    P = orb.TriangulationParams()
    tail = [C.byref(P)] + [p(tab, C.c_float)] * 4 + [8, None, p(free, C.c_int32), 0]
    outs = [p(reason, C.c_uint8), p(source, C.c_uint8), p(x3d, C.c_float), p(slot, C.c_int32), C.byref(created)]
    assert L.vsg_frame_set_stereo_points(None, p(x3d, C.c_float), p(x3d, C.c_float)) == INVALID
    assert L.vsg_frame_triangulate_matches(None, None, p(m12, C.c_int32), *tail, *outs) == INVALID
    F, ep = np.zeros(9, np.float32), np.zeros(2, np.float32)
    assert L.vsg_frame_create_new_map_points(None, p(flags, C.c_uint8), None, None, None, 0, None, p(flags, C.c_uint8), None, None,
                                             None, 0, p(F, C.c_float), p(ep, C.c_float), 0, 0, 1, *tail, p(m12, C.c_int32),
                                             *outs) == INVALID
    assert (reason == 9).all() and (source == 8).all() and (x3d == -3).all() and (slot == -5).all() and (m12 == 6).all()
    assert created.value == -77


ADAPTOR = ROOT / "tests" / "_adaptor_newpoints"


def test_cpp_adaptor_compiles_and_fails_loudly_without_device():
    L = orb.load_library()
    subprocess.check_call(["make", "-C", str(ADAPTOR)], stdout=subprocess.DEVNULL)
    adaptor = (ROOT / "include" / "vsg_orb_adaptor.hpp").read_text()
    for name in ("void SetStereoPoints(", "void TriangulateMatches(", "int CreateNewMapPoints(", "struct NewMapPointsResult"):
        assert name in adaptor, name
    if L.vsg_device_count() <= 0:
        r = subprocess.run([str(ADAPTOR / "newpoints_check"), "/dev/null", "/dev/null"], capture_output=True, text=True)
        assert r.returncode == 3 and "no CPU fallback" in r.stdout


def _blob(a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    return np.int32(a.size if a.dtype.names is None else a.nbytes).tobytes() + a.tobytes()


import pytest  # noqa: E402


@pytest.mark.gpu
def test_cpp_adaptor_equals_the_ctypes_path(tmp_path):
    import triangulation_hostcore as hc
    import triangulation_scenes as ts
    subprocess.check_call(["make", "-C", str(ADAPTOR)], stdout=subprocess.DEVNULL)
    s = ts.parity(kf2_first=True)
    cap = 512
    free = np.random.default_rng(4).permutation(cap)[:90].astype(np.int32)
    parts = []
    for t in ("1", "2"):
        parts += [_blob(s["k" + t].view(np.uint8), np.uint8), _blob(s["d" + t], np.uint8), _blob(s["ur" + t], np.float32),
                  _blob(s["stereo" + t][:, :3], np.float32), _blob(s["stereo" + t][:, 3], np.float32),
                  _blob(s["no_mp" + t], np.uint8)] + [_blob(a, np.int32) for a in s["fv" + t]]
    parts += [_blob(s["F12"], np.float32), _blob(s["ep"], np.float32), _blob(s["sf1"], np.float32), _blob(s["sigma2_1"], np.float32),
              _blob(hc.params_blob(s["P"]), np.uint8), _blob(free, np.int32), _blob([cap], np.int32)]
    src, out = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(b"".join(parts))
    r = subprocess.run([str(ADAPTOR / "newpoints_check"), str(src), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
    # the same through ctypes
    n1 = len(s["k1"])
    f = []
    for t in ("1", "2"):
        f.append(orb.Frame(n1 + 1).upload(s["k" + t], s["d" + t], ts.BOUNDS, u_right=s["ur" + t])
                 .SetStereoPoints(s["stereo" + t][:, :3], s["stereo" + t][:, 3]))
    mp = orb.MapPoints(cap)
    pose = lambda c: orb.FramePose.make(c["Rcw"], c["tcw"], c["Ow"], c["fx"], c["fy"], c["cx"], c["cy"], c["mbf"], 0.0, 0)  # noqa: E731
    P = orb.TriangulationParams.make(pose(s["P"]["kf1"]), pose(s["P"]["kf2"]), s["P"]["ratio_factor"], s["P"]["inertial"],
                                     s["P"]["far_points"], s["P"]["th_far_points"], s["P"]["kf2_first"])
    assert bytes(P) == hc.params_blob(s["P"]).tobytes()
    got = f[0].CreateNewMapPoints(s["no_mp1"], f[1], s["no_mp2"], s["F12"], s["ep"], False, False, True, P, s["sf1"], s["sigma2_1"],
                                  s["sf2"], s["sigma2_2"], mp=mp, free_slots=free, fv1=s["fv1"], fv2=s["fv2"])
    st = mp.read(np.arange(cap))
    pairs = np.array([(i, j) for i, j in enumerate(got["matches12"]) if j >= 0], np.int32).reshape(-1, 2)
    one = b"".join([np.array([got["nmatches"], got["n_created"], len(pairs)], np.int32).tobytes(), pairs.tobytes(),
                    got["reason"].tobytes(), got["source"].tobytes(), got["x3d"].tobytes(), got["new_slot"].tobytes()] +
                   [np.ascontiguousarray(st[k]).tobytes() for k in ("world_pos", "normal", "min_dist", "max_dist", "desc", "observed")])
    assert got["n_created"] == 90 and got["nmatches"] >= 150
    assert out.read_bytes() == one + one  # the fused call, then TriangulateMatches on its matches into a second store
