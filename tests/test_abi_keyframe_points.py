"""Fuse x2 and the Sim3 projection search on resident map points at the C-ABI boundary: declared in include/vsg_orb.h with
their reference lines and callers, exported by the library, bound by orb.py, and usable through the C++ adaptor
(tests/_adaptor_keyframe: the two vsg::ResidentMatcher::Fuse overloads and the SearchByProjection overload that take a
ResidentMapPoints store plus slots).  The GPU run of that program is in tests/test_gpu_keyframe_points.py."""
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("vsg_frame_fuse_points", "vsg_frame_fuse_points_sim3", "vsg_frame_search_sim3_points")
ADAPTOR = ROOT / "tests" / "_adaptor_keyframe"


@pytest.fixture(scope="module")
def lib():
    from visual_sgraphs_amd import build, orb
    build.build()
    return orb.load_library()


def test_entry_points_are_declared_exported_and_bound(lib):
    from visual_sgraphs_amd import orb
    header = (ROOT / "include" / "vsg_orb.h").read_text()
    declared = set(re.findall(r"\b(vsg_[a-z0-9_]+)\s*\(", header))
    for name in NAMES:
        assert name in declared and name in orb.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes, f"{name} has no ctypes prototype"
    assert [len(getattr(lib, n).argtypes) for n in NAMES] == [17, 15, 15]
    assert callable(orb.Frame.FusePoints) and callable(orb.Frame.FusePoints_Sim3) and callable(orb.Frame.SearchSim3Points)
    # every entry cites its reference lines and its caller
    cites = (("ORBmatcher.cc:1148-1335", "LocalMapping.cc:770"), ("ORBmatcher.cc:1337-1446", "LoopClosing.cc:2012"),
             ("ORBmatcher.cc:430-528", "LoopClosing.cc:735"))
    for name, (lines, caller) in zip(NAMES, cites):
        comment = header[:header.index(f"int {name}(")].rsplit("/*", 1)[1]
        assert lines in comment and caller in comment, name
    block = header[:header.index("int vsg_frame_fuse_points(")].rsplit("/*", 1)[1]
    assert "KeyFrame.cc:880-883" in block and "KeyFrame.cc:52" in block
    # the host-array entries keep their signatures
    assert len(lib.vsg_frame_fuse.argtypes) == 13
    assert len(lib.vsg_frame_fuse_sim3.argtypes) == 9
    assert len(lib.vsg_frame_search_by_projection_sim3.argtypes) == 9
    for name, nargs in (("vsg_frame_fuse", 13), ("vsg_frame_fuse_sim3", 9), ("vsg_frame_search_by_projection_sim3", 9)):
        decl = header[header.index(f"int {name}("):]
        assert decl[:decl.index(";")].count(",") + 1 == nargs, name
    adaptor = (ROOT / "include" / "vsg_orb_adaptor.hpp").read_text()
    assert "const vector<MapPoint *> &vpMapPoints, const float th = 3.0, const bool bRight = false" in adaptor
    assert "Sophus::Sim3f &Scw, const vector<MapPoint *> &vpPoints, float th" in adaptor
    for name in NAMES:
        assert f"{name}(" in adaptor, name


def test_null_handles_are_refused_without_a_device(lib):
    """-6 (VSG_ERR_INVALID) before any device is touched: no CPU fallback computes anything."""
    assert lib.vsg_frame_fuse_points(None, None, 0, None, None, None, 3.0, None, None, 8, None, None, None, None, None,
                                     None, None) == -6
    assert lib.vsg_frame_fuse_points_sim3(None, None, 0, None, None, None, 4.0, None, 8, None, None, None, None, None,
                                          None) == -6
    assert lib.vsg_frame_search_sim3_points(None, None, 0, None, None, None, 8.0, 1.5, None, 8, None, None, None, None,
                                            None) == -6


def test_cpp_adaptor_compiles_and_fails_loudly_without_device(lib):
    subprocess.check_call(["make", "-C", str(ADAPTOR)], stdout=subprocess.DEVNULL)
    if lib.vsg_device_count() == 0:
        r = subprocess.run([str(ADAPTOR / "keyframe_check"), "/dev/null", "/dev/null"], capture_output=True, text=True)
        assert r.returncode == 3 and "no CPU fallback" in r.stdout
