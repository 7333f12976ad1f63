"""SearchForTriangulation with the epipolar test on the device at the C-ABI boundary: declared in include/vsg_orb.h (its test
hook in include/vsg_orb_debug_epipolar.h), exported by the library, bound by orb.py, and used through the C++ adaptor
(tests/_adaptor_triangulation: the vsg::ResidentMatcher::SearchForTriangulation overload that takes F12 and the epipole,
against the predicate overload given the host build of csrc/vsg_epipolar.h).  The GPU test runs the C++ program on the parity
scene and compares the pairs it wrote with the CPU oracle fed the restatement's bits."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import epipolar_reference as er
import epipolar_scenes as es

ROOT = Path(__file__).resolve().parent.parent
NAME, HOOK = "vsg_frame_search_for_triangulation_epipolar", "vsg_debug_epipolar_pairs"
ADAPTOR = ROOT / "tests" / "_adaptor_triangulation"


@pytest.fixture(scope="module")
def lib():
    from visual_sgraphs_amd import build, orb
    build.build()
    return orb.load_library()


def test_entry_point_and_hook_are_declared_exported_and_bound(lib):
    from visual_sgraphs_amd import orb
    header = (ROOT / "include" / "vsg_orb.h").read_text()
    assert NAME in set(re.findall(r"\b(vsg_[a-z0-9_]+)\s*\(", header)) and NAME in orb.EXPORTS and hasattr(lib, NAME)
    assert len(getattr(lib, NAME).argtypes) == 21
    comment = header[:header.index(f"int {NAME}(")].rsplit("/*", 1)[1]
    for cite in ("ORBmatcher.cc:902-1146", "Pinhole.cpp:118-141", "LocalMapping.cc:389-460", "VSG_ERR_UNSUPPORTED"):
        assert cite in comment, cite
    hook = (ROOT / "include" / "vsg_orb_debug_epipolar.h").read_text()
    assert f"int {HOOK}(" in hook and hasattr(lib, HOOK) and len(getattr(lib, HOOK).argtypes) == 13
    assert HOOK not in header and "vsg_orb_debug_epipolar.h" not in (ROOT / "INTEGRATION.md").read_text()
    assert callable(orb.Frame.SearchForTriangulationEpipolar) and callable(orb.debug_epipolar_pairs)
    # the existing entry point keeps its signature, the adaptor its predicate overloads
    assert len(lib.vsg_frame_search_for_triangulation.argtypes) == 16
    adaptor = (ROOT / "include" / "vsg_orb_adaptor.hpp").read_text()
    assert adaptor.count("template <class Pred>\n  int SearchForTriangulation(") == 2
    assert "const float F12[9], const float ep[2], const std::vector<float> &mvScaleFactors2" in adaptor
    # the header's codes are the shared source's
    core = (ROOT / "visual_sgraphs_amd" / "csrc" / "vsg_epipolar.h").read_text()
    codes = dict(re.findall(r"(kEpi[A-Za-z]+) = (\d)", core))
    assert codes == {"kEpiPass": "0", "kEpiNotStereo": "1", "kEpiEpipoleGate": "2", "kEpiDenZero": "3", "kEpiChiSquare": "4"}
    assert re.findall(r"VSG_EPIPOLAR_[A-Z_]+ = (\d)", hook) == ["0", "1", "2", "3", "4"]


def test_null_handles_are_refused_without_a_device(lib):
    """-6 (VSG_ERR_INVALID) before any device is touched: no CPU fallback computes anything."""
    assert getattr(lib, NAME)(None, None, None, None, None, 0, None, None, None, None, None, 0, None, None, None, None, 8, 0, 0,
                              1, None) == -6
    assert getattr(lib, HOOK)(None, None, 0, None, None, None, None, None, None, 8, 0, 0, None) == -6


def test_cpp_adaptor_compiles_and_fails_loudly_without_device(lib):
    subprocess.check_call(["make", "-C", str(ADAPTOR)], stdout=subprocess.DEVNULL)
    if lib.vsg_device_count() == 0:
        r = subprocess.run([str(ADAPTOR / "triangulation_check"), "/dev/null", "/dev/null"], capture_output=True, text=True)
        assert r.returncode == 3 and "no CPU fallback" in r.stdout


def _blob(a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    return np.int32(a.size if a.dtype.names is None else len(a)).tobytes() + a.tobytes()


@pytest.mark.gpu
def test_cpp_adaptor_equals_the_predicate_overload_and_the_oracle(tmp_path):
    import oracle_lib as ol
    from visual_sgraphs_amd import orb
    subprocess.check_call(["make", "-C", str(ADAPTOR)], stdout=subprocess.DEVNULL)
    s = es.frames()
    parts = []
    for t in ("1", "2"):
        parts += [_blob(s["k" + t], orb.KP_DTYPE), _blob(s["d" + t], np.uint8), _blob(s["ur" + t], np.float32),
                  _blob(s["no_mp" + t], np.uint8)] + [_blob(a, np.int32) for a in s["fv" + t]]
    parts += [_blob(s["F12"], np.float32), _blob(s["ep"], np.float32), _blob(s["sf"], np.float32),
              _blob(s["sigma2"], np.float32), _blob(es.BOUNDS, np.float32)]
    src, out = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(b"".join(parts))
    r = subprocess.run([str(ADAPTOR / "triangulation_check"), str(src), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
    buf, pos = out.read_bytes(), 0
    for leg in range(8):
        n = int(np.frombuffer(buf, np.int32, 1, pos)[0])
        flat = np.frombuffer(buf, np.int32, n, pos + 4)
        pos += 4 + 4 * n
        ref = er.scene(s["k1"], s["ur1"], s["no_mp1"], s["fv1"], s["d1"], s["k2"], s["ur2"], s["no_mp2"], s["fv2"], s["d2"],
                       s["F12"], s["ep"], s["sf"], s["sigma2"], bool(leg & 1), bool(leg & 2))
        nm, m12 = ol.search_for_triangulation(s["d1"], s["k1"]["angle"], ref["eligible1"], s["fv1"], s["d2"], s["k2"]["angle"],
                                              ref["eligible2"], s["fv2"], ref["pair_ok"], ref["pair_off"], bool(leg & 4))
        want = np.array([(i, m12[i]) for i in range(len(m12)) if m12[i] >= 0], np.int32).reshape(-1, 2)
        assert flat[0] == nm and np.array_equal(flat[1:].reshape(-1, 2), want), leg
        if not leg & 1:
            assert nm >= 40
    assert pos == len(buf)
