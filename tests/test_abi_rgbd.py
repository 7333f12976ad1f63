"""CPU tests of the RGB-D frame entry points at the C-ABI boundary: declared in include/vsg_orb.h, exported by the
library, bound by orb.py, and used through the C++ adaptor (tests/_adaptor_rgbd)."""
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("vsg_orb_extract_to_frame_rgbd", "vsg_depth_map_scale", "vsg_rgbd_depth_batch_device")


@pytest.fixture(scope="module")
def lib():
    from visual_sgraphs_amd import build, orb
    build.build()
    return orb.load_library()


def test_rgbd_entry_points_are_declared_exported_and_bound(lib):
    from visual_sgraphs_amd import orb
    header = (ROOT / "include" / "vsg_orb.h").read_text()
    declared = set(re.findall(r"\b(vsg_[a-z0-9_]+)\s*\(", header))
    for name in NAMES:
        assert name in declared and name in orb.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes, f"{name} has no ctypes prototype"
    consts = dict((k, int(v)) for k, v in re.findall(r"#define (VSG_DEPTH_\w+) (\d+)", header))
    assert consts == {"VSG_DEPTH_U16": orb.VSG_DEPTH_U16, "VSG_DEPTH_F32": orb.VSG_DEPTH_F32}
    assert callable(orb.Frame.extract_into_rgbd) and callable(orb.rgbd_depth_batch_device)
    assert callable(orb.depth_map_scale)
    # the existing one-frame entry keeps its signature
    assert len(lib.vsg_orb_extract_to_frame.argtypes) == 20


def test_rgbd_entry_points_refuse_without_device(lib):
    """Argument errors come first; with valid arguments and no device the batch entry reports VSG_ERR_NO_DEVICE."""
    import ctypes as C
    import numpy as np
    from visual_sgraphs_amd import orb
    if lib.vsg_device_count() > 0:
        pytest.skip("a GPU is present")
    K4 = np.array([500, 500, 320, 240], np.float32)
    fake = 1 << 20  # never dereferenced: no device, no launch
    args = dict(d_depth=fake, depth_type=orb.VSG_DEPTH_U16, nframes=2, frame_stride=640 * 480 * 2, depth_stride=1280,
                rows=480, cols=640, depth_scale=0.001, mbf=40.0, K4=K4, dist=None, d_kps=fake, d_counts=fake,
                capacity=1024, d_u_right=fake, d_depth_out=fake)
    with pytest.raises(orb.VsgError) as e:
        orb.rgbd_depth_batch_device(**args)
    assert e.value.code == -4  # VSG_ERR_NO_DEVICE
    for bad, code in ((dict(depth_type=7), -3), (dict(depth_stride=1000), -6), (dict(d_depth=0), -6),
                      (dict(frame_stride=1000), -6), (dict(rows=0), -6)):
        with pytest.raises(orb.VsgError) as e:
            orb.rgbd_depth_batch_device(**{**args, **bad})
        assert e.value.code == code, bad
    n = C.c_int32(0)
    rc = lib.vsg_orb_extract_to_frame_rgbd(None, None, 480, 640, 640, 0, 0, None, None, 0, C.byref(n), None, None, None,
                                           0, 0.0, 0.0, 640.0, 480.0, None, None, 0, 1280, 480, 640, 1.0, 40.0, None,
                                           None)
    assert rc == -6  # VSG_ERR_INVALID: no extractor, no frame


def test_cpp_adaptor_rgbd_compiles_and_fails_loudly_without_device(lib):
    """tests/_adaptor_rgbd/rgbd_check.cpp uses ResidentFrame::ExtractIntoRGBD and DepthMapScale: it builds with plain
    g++; DepthMapScale is host arithmetic and answers without a device, the extractor refuses to run."""
    d = ROOT / "tests" / "_adaptor_rgbd"
    subprocess.check_call(["make", "-C", str(d)], stdout=subprocess.DEVNULL)
    if lib.vsg_device_count() > 0:
        pytest.skip("a GPU is present")
    r = subprocess.run([str(d / "rgbd_check"), "/dev/null"], capture_output=True, text=True)
    assert r.stdout.startswith("DepthMapScale 0.00100000005 1\n")
    assert r.returncode == 3 and "no CPU fallback" in r.stdout


def test_python_depth_view_takes_host_planes_only():
    """Frame.extract_into_rgbd hands the library a HOST pointer: a tensor that lives elsewhere, or a plane that is not 2-D
    with contiguous rows, is refused before any call (no device needed)."""
    import numpy as np
    import torch
    from visual_sgraphs_amd import orb
    with pytest.raises(ValueError, match="host memory"):
        orb._depth_view(torch.empty((4, 6), dtype=torch.float32, device="meta"))
    with pytest.raises(ValueError, match="2-D"):
        orb._depth_view(torch.zeros((2, 4, 6), dtype=torch.float32))
    with pytest.raises(ValueError, match="2-D"):
        orb._depth_view(torch.zeros((6, 4), dtype=torch.float32).t())
    t = torch.zeros((4, 8), dtype=torch.float32)[:, :6]  # padded rows are fine
    ptr, typ, rows, cols, stride, _ = orb._depth_view(t)
    assert (ptr, typ, rows, cols, stride) == (t.data_ptr(), orb.VSG_DEPTH_F32, 4, 6, 32)
    a = np.zeros((4, 8), np.uint16)[:, :6]
    assert orb._depth_view(a)[1:5] == (orb.VSG_DEPTH_U16, 4, 6, 16)
    assert orb._depth_view(np.zeros((4, 6), np.int32))[1] == -1  # the library answers VSG_ERR_UNSUPPORTED
