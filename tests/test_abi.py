"""CPU tests of the C-ABI boundary: the library builds/loads, exports exactly what include/vsg_orb.h
declares, and refuses to compute without a GPU (no CPU fallback)."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def lib():
    from visual_sgraphs_amd import build, orb
    build.build()
    return orb.load_library()


def test_header_and_debug_hook_symbols_are_exported(lib):
    """Every symbol of include/vsg_orb.h and, listed exactly, every hook of include/vsg_orb_debug.h (now with
    vsg_debug_last_launch_forms) is exported, and orb.EXPORTS binds exactly those."""
    from visual_sgraphs_amd import orb
    header = (ROOT / "include" / "vsg_orb.h").read_text()
    declared = sorted(set(re.findall(r"\b(vsg_[a-z0-9_]+)\s*\(", header)))
    assert len(declared) >= 25
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/vsg_orb.h but not exported"
    # the test / measurement hooks live in a header of their own, outside the boundary a maintainer binds (VERDICT r5 #8b)
    assert not [n for n in declared if n.startswith("vsg_debug_")], "debug hooks belong in include/vsg_orb_debug.h"
    dbg = sorted(set(re.findall(r"\b(vsg_debug_[a-z0-9_]+)\s*\(", (ROOT / "include" / "vsg_orb_debug.h").read_text())))
    assert dbg == ["vsg_debug_call_profile", "vsg_debug_device_sort", "vsg_debug_kfdb_state", "vsg_debug_last_launch_forms",
                   "vsg_debug_track_walk"]
    for name in dbg:
        assert hasattr(lib, name), f"{name} declared in include/vsg_orb_debug.h but not exported"
    assert "vsg_orb_debug.h" not in (ROOT / "INTEGRATION.md").read_text()
    assert sorted(orb.EXPORTS) == sorted(declared + dbg)


def test_launch_forms_record_matches_the_header():
    """orb.debug_launch_forms reads vsg_launch_forms through ctypes: the same int fields in the same order, and the same
    VSG_OCT_* values."""
    from visual_sgraphs_amd import orb
    text = (ROOT / "include" / "vsg_orb_debug.h").read_text()
    body = re.search(r"typedef struct vsg_launch_forms \{(.*?)\} vsg_launch_forms;", text, re.S).group(1)
    assert re.findall(r"^\s*int (\w+);", body, re.M) == list(orb.LAUNCH_FORM_FIELDS)
    enum = dict((k, int(v)) for k, v in re.findall(r"(VSG_OCT_\w+) = (\d+)", text))
    assert enum == {"VSG_" + n: getattr(orb, n) for n in ("OCT_BLUR_MEMBATCH", "OCT_BLUR_MEMBATCH_FUSED",
                                                           "OCT_FEW_MEMBATCH", "OCT_FEW_MEMBATCH_FUSED", "OCT_STANDALONE")}


def test_keypoint_record_is_cv_keypoint_layout():
    from visual_sgraphs_amd import orb
    assert orb.KP_DTYPE.itemsize == 28
    assert [orb.KP_DTYPE.fields[n][1] for n in ("x", "y", "size", "angle", "response", "octave", "class_id")] == \
        [0, 4, 8, 12, 16, 20, 24]


def test_no_cpu_fallback_without_device(lib):
    from visual_sgraphs_amd import orb
    if lib.vsg_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(orb.VsgError) as ei:
        orb.ORBextractor(1000, 1.2, 8, 20, 7)
    assert ei.value.code == -4  # VSG_ERR_NO_DEVICE
    m = orb.ORBmatcher(0.7, True)
    with pytest.raises(orb.VsgError):
        m.block_best2(np.zeros((4, 32), np.uint8), np.zeros((4, 32), np.uint8))


def test_product_does_not_reference_the_oracle():
    """The shipped path must not import, link or call anything under oracle/."""
    pkg = ROOT / "visual_sgraphs_amd"
    for f in list(pkg.rglob("*.py")) + list(pkg.rglob("*.hip")) + list(pkg.rglob("*.h")) + [ROOT / "include/vsg_orb.h"]:
        txt = f.read_text()
        assert "orb_oracle" not in txt and "oracle_lib" not in txt and "liborb_oracle" not in txt, f


def test_cpp_adaptor_compiles_and_fails_loudly_without_device(lib, tmp_path):
    """include/vsg_orb_adaptor.hpp is plain C++ over the C ABI: compile it with g++, link the HIP library and
    check that constructing the extractor without a GPU throws (no silent fallback)."""
    import subprocess
    from visual_sgraphs_amd import orb
    src = tmp_path / "t.cpp"
    src.write_text('#include "vsg_orb_adaptor.hpp"\n#include <cstdio>\n'
                   'int main(){ try { vsg::ORBextractor e(1000,1.2f,8,20,7); std::vector<vsg_keypoint> k; '
                   'std::vector<uint8_t> d; std::vector<int> lap{0,0}; std::vector<uint8_t> img(640*480,128);'
                   'int m = e(img.data(),480,640,640,k,d,lap); printf("OK %d %zu\\n", m, k.size()); return 0; }'
                   ' catch (const std::exception& ex) { printf("THROW %s\\n", ex.what()); return 3; } }\n')
    exe = tmp_path / "t"
    subprocess.check_call(["g++", "-std=c++17", "-I", str(ROOT / "include"), str(src), "-o", str(exe),
                           str(orb.LIB_PATH), "-Wl,-rpath," + str(orb.LIB_PATH.parent), "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    if lib.vsg_device_count() > 0:
        assert r.returncode == 0 and r.stdout.startswith("OK 0 0")  # constant image: 0 keypoints
    else:
        assert r.returncode == 3 and "THROW" in r.stdout


def test_cpp_adaptor_full_surface_compiles(lib):
    """tests/_adaptor/adaptor_check.cpp uses every class of the C++ adaptor (extractor, grid, vocabulary, matcher);
    it must build with plain g++ and, without a GPU, refuse to run (the GPU run is tests/test_gpu_adaptor.py)."""
    import subprocess
    d = ROOT / "tests" / "_adaptor"
    subprocess.check_call(["make", "-C", str(d)], stdout=subprocess.DEVNULL)
    if lib.vsg_device_count() > 0:
        pytest.skip("a GPU is present")
    r = subprocess.run([str(d / "adaptor_check"), "/dev/null", "/dev/null"], capture_output=True, text=True)
    assert r.returncode == 3 and "no CPU fallback" in r.stdout


def test_adaptor_opencv_branch_compiles(tmp_path):
    """The VSG_WITH_OPENCV branch of the adaptor (the reference's exact operator() signature, mvImagePyramid,
    DownloadPyramid) is type-checked with the reference's language standard against a DECLARATION-ONLY header of the
    OpenCV names it touches (tests/_adaptor/cv_decl: not OpenCV, never linked or run).  OpenCV itself is absent from
    this image, so behaviour against a real cv::Mat stays unverified."""
    import subprocess
    src = tmp_path / "cvchk.cpp"
    src.write_text('#define VSG_WITH_OPENCV\n#include "vsg_orb_adaptor.hpp"\n'
                   'int use(vsg::ORBextractor &e, cv::InputArray img, std::vector<cv::KeyPoint> &k, cv::OutputArray d,'
                   ' std::vector<int> &lap) { int m = e(img, img, k, d, lap); e.DownloadPyramid(); '
                   'return m + (int)e.mvImagePyramid.size(); }\n')
    subprocess.check_call(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Werror", "-I", str(ROOT / "include"), "-I",
                           str(ROOT / "tests" / "_adaptor" / "cv_decl"), str(src)])


def test_stream_to_rank_honours_more_ranks_than_streams():
    from visual_sgraphs_amd import sharding
    # C5: 4 camera streams on 8 GPUs = 2 ranks per stream, alternating frames
    seen = {}
    for s in range(4):
        for f in range(6):
            r = sharding.stream_to_rank(s, 4, 8, f)
            assert 0 <= r < 8 and r % 4 == s
            seen.setdefault(r, []).append((s, f))
    assert sorted(seen) == list(range(8)) and all(len(v) == 3 for v in seen.values())
    # fewer or as many ranks as streams: stream s -> rank s % world, every frame
    assert [sharding.stream_to_rank(s, 4, 4, 9) for s in range(4)] == [0, 1, 2, 3]
    assert [sharding.stream_to_rank(s, 4, 2, 1) for s in range(4)] == [0, 1, 0, 1]
    # a world that is not a multiple of the stream count: the spare ranks share the first streams
    ranks = {sharding.stream_to_rank(s, 4, 6, f) for s in range(4) for f in range(4)}
    assert ranks == set(range(6))


def _bad_feature_vectors(n):
    """(name, FeatureVector) of a frame of n features: an idx that holds n, and offsets that descend."""
    ids, off = np.array([2, 5, 9], np.int32), np.array([0, 3, 6, 8], np.int32)
    idx = np.arange(8, dtype=np.int32)
    bad_idx = idx.copy()
    bad_idx[4] = n
    bad_off = off.copy()
    bad_off[1] = 7
    return (ids, off, idx), [("idx_holds_n", (ids, off, bad_idx)), ("offsets_descend", (ids, bad_off, idx))]


def test_bad_feature_vectors_are_refused_before_the_device_is_touched(lib):
    """VSG_ERR_INVALID (-6), not VSG_ERR_NO_DEVICE, on a machine without a device, and the output array as it was: the
    FeatureVector and predicate-bit checks of csrc/vsg_fv.h run before thread_ctx, before anything is enqueued and before the
    output is written.  With a device present the same calls are refused the same way."""
    from visual_sgraphs_amd import orb
    p, n = orb._p, 10
    desc, angle, flags = np.zeros((n, 32), np.uint8), np.zeros(n, np.float32), np.ones(n, np.uint8)
    good, bad = _bad_feature_vectors(n)
    side = lambda fv, with_flags=True: ([p(desc, orb._u8p), p(angle, orb._f32p)] + ([p(flags, orb._u8p)] if with_flags else []) +
                                        [n] + [p(a, orb._i32p) for a in fv] + [len(fv[0])])
    exact = np.array([0, 9, 18, 22], np.int32)      # the three shared nodes hold 3 x 3, 3 x 3 and 2 x 2 pairs
    short = exact - np.array([0, 0, 0, 1], np.int32)
    bits = np.full(2, 0xFFFFFFFF, np.uint32)
    calls = []
    for name, fv in bad:
        for where in (0, 1):
            a, b = (fv, good) if where == 0 else (good, fv)
            calls.append((name, "vsg_search_by_bow_kf_f_stereo",
                          lambda out, a=a, b=b: [0] + side(a) + side(b, False)[:3] + [-1] + side(b, False)[3:] + [0.7, 1, out]))
            calls.append((name, "vsg_search_by_bow_kf_kf", lambda out, a=a, b=b: [0] + side(a) + side(b) + [0.7, 1, out]))
            calls.append((name, "vsg_search_for_triangulation",
                          lambda out, a=a, b=b: [0] + side(a) + side(b) + [bits.ctypes.data, exact.ctypes.data, 1, out]))
    calls.append(("pair_off_one_bit_short", "vsg_search_for_triangulation",
                  lambda out: [0] + side(good) + side(good) + [bits.ctypes.data, short.ctypes.data, 1, out]))
    assert len(calls) == 13
    for name, fn, args in calls:
        out = np.full(n, 12345, np.int32)
        assert getattr(lib, fn)(*args(p(out, orb._i32p))) == -6, (fn, name)
        assert (out == 12345).all(), (fn, name)
    if lib.vsg_device_count() <= 0:   # the same calls with valid arguments get as far as the device
        for fn, args in (("vsg_search_by_bow_kf_kf", lambda out: [0] + side(good) + side(good) + [0.7, 1, out]),
                         ("vsg_search_for_triangulation",
                          lambda out: [0] + side(good) + side(good) + [bits.ctypes.data, exact.ctypes.data, 1, out])):
            out = np.full(n, 12345, np.int32)
            assert getattr(lib, fn)(*args(p(out, orb._i32p))) == -4 and (out == 12345).all(), fn
