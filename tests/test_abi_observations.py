"""vsg_mappoints_refresh_from_observations at the C-ABI boundary: declared in include/vsg_orb.h, exported by the library, bound
by orb.py with the header's signature, and reachable through the C++ adaptor (vsg::ResidentMapPoints::Refresh,
tests/_adaptor_refresh; the GPU run of that program is in tests/test_gpu_mappoints_refresh.py)."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
NAME = "vsg_mappoints_refresh_from_observations"
ADAPTOR = ROOT / "tests" / "_adaptor_refresh"
CTYPE = {"vsg_mappoints *": C.c_void_p, "int": C.c_int, "const int32_t *": C.POINTER(C.c_int32),
         "const uint8_t *": C.POINTER(C.c_uint8), "vsg_frame *const *": C.POINTER(C.c_void_p),
         "const float *": C.POINTER(C.c_float), "int32_t *": C.POINTER(C.c_int32), "float *": C.POINTER(C.c_float)}


@pytest.fixture(scope="module")
def lib():
    from visual_sgraphs_amd import build, orb
    build.build()
    return orb.load_library()


def header_parameters():
    text = (ROOT / "include" / "vsg_orb.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    args = re.search(r"\bint " + NAME + r"\s*\((.*?)\);", text, re.S).group(1)
    out = []
    for a in args.split(","):
        m = re.match(r"\s*(.*?)(\w+)\s*$", a, re.S)
        out.append((" ".join(m.group(1).split()), m.group(2)))
    return out


def test_entry_point_is_declared_exported_and_bound_with_the_headers_signature(lib):
    from visual_sgraphs_amd import orb
    params = header_parameters()
    assert [n for _, n in params] == ["mp", "n", "slots", "obs_off", "obs_kf", "obs_idx", "obs_bad", "ref_pos", "n_kf", "kfs",
                                      "kf_Ow", "scale_factors", "nlevels", "what", "best", "normal", "min_dist", "max_dist"]
    assert NAME in orb.EXPORTS and hasattr(lib, NAME)
    assert list(getattr(lib, NAME).argtypes) == [CTYPE[t] for t, _ in params]
    header = (ROOT / "include" / "vsg_orb.h").read_text()
    assert re.search(r"#define VSG_REFRESH_DESC\s+1\b", header) and re.search(r"#define VSG_REFRESH_NORMAL\s+2\b", header)
    assert (orb.REFRESH_DESC, orb.REFRESH_NORMAL) == (1, 2) and callable(orb.MapPoints.refresh)
    # the entry points beside it keep their signatures
    assert len(lib.vsg_mappoints_update.argtypes) == 9 and len(lib.vsg_distinctive_descriptors.argtypes) == 5


def test_adaptor_passes_the_headers_arguments_in_order():
    text = (ROOT / "include" / "vsg_orb_adaptor.hpp").read_text()
    assert "struct RefreshResult" in text and re.search(r"RefreshResult Refresh\(", text)
    body = re.search(NAME + r"\((.*?)\),\s*\"" + NAME + "\"", text, re.S).group(1)
    passed = [" ".join(a.split()) for a in re.split(r",(?![^()]*\))", body)]
    assert len(passed) == len(header_parameters()) == 18
    for arg, stem in zip(passed, ("mp_", "n", "slots", "obsOff", "obsKf", "obsIdx", "obsBad", "refPos", "keyFrames",
                                  "keyFrames", "kfOw", "mvScaleFactors", "mvScaleFactors", "what", "r.best", "r.normal",
                                  "r.minDist", "r.maxDist")):
        assert stem in arg, (arg, stem)


def test_refuses_before_it_looks_for_a_device(lib):
    from visual_sgraphs_amd import orb
    f = getattr(lib, NAME)
    assert f(None, 0, None, None, None, None, None, None, 0, None, None, None, 8, 3, None, None, None, None) == -6
    if lib.vsg_device_count() > 0:
        return
    with pytest.raises(orb.VsgError) as e:
        orb.MapPoints(100)
    assert e.value.code == -4  # VSG_ERR_NO_DEVICE: no CPU fallback


def test_python_binding_checks_its_array_lengths():
    from visual_sgraphs_amd import orb
    mp = orb.MapPoints.__new__(orb.MapPoints)  # no device needed: the length checks come first
    for kwargs in (dict(obs_off=[0, 1, 2]), dict(obs_idx=[0, 0]), dict(ref_pos=[0, 0]), dict(obs_bad=[0, 0]),
                   dict(kf_Ow=np.zeros(4)), dict(obs_off=[0, 5])):
        a = dict(slots=[3], obs_off=[0, 1], obs_kf=[0], obs_idx=[0], ref_pos=[0], keyframes=[], kf_Ow=np.zeros(0),
                 scale_factors=np.ones(8))
        a.update(kwargs)
        with pytest.raises(ValueError):
            mp.refresh(**a)
    mp._h = None


def test_cpp_adaptor_compiles_and_fails_loudly_without_device(lib):
    subprocess.check_call(["make", "-C", str(ADAPTOR)], stdout=subprocess.DEVNULL)
    if lib.vsg_device_count() > 0:
        return
    r = subprocess.run([str(ADAPTOR / "refresh_check"), "/dev/null", "/dev/null"], capture_output=True, text=True)
    assert r.returncode == 3 and "no CPU fallback" in r.stdout
