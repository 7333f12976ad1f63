"""The resident map-point entry points at the C-ABI boundary: declared in include/vsg_orb.h, exported by the library, bound
by orb.py, and used through the C++ adaptor (tests/_adaptor_mappoints: vsg::ResidentMapPoints, vsg::FramePose,
vsg::ResidentFrame::isInFrustum / SearchLocalPoints).  The GPU test runs the C++ program on a scenario and compares what
it wrote with tests/frustum_reference.py and with the Python binding."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import frustum_reference as fr

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("vsg_mappoints_create", "vsg_mappoints_destroy", "vsg_mappoints_capacity", "vsg_mappoints_update",
         "vsg_mappoints_read", "vsg_frame_is_in_frustum", "vsg_frame_search_local_points")
ADAPTOR = ROOT / "tests" / "_adaptor_mappoints"


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
    assert callable(orb.MapPoints.update) and callable(orb.MapPoints.read) and callable(orb.MapPoints.close)
    assert callable(orb.Frame.isInFrustum) and callable(orb.Frame.SearchLocalPoints)
    # existing entry points keep their signatures
    assert len(lib.vsg_frame_search_by_projection.argtypes) == 23


def test_frame_pose_record_matches_the_header():
    from visual_sgraphs_amd import orb
    text = (ROOT / "include" / "vsg_orb.h").read_text()
    body = re.search(r"typedef struct vsg_frame_pose \{(.*?)\} vsg_frame_pose;", text, re.S).group(1)
    names = []
    for decl in re.findall(r"(?:float|int32_t) ([^;]+);", body):
        names += [re.sub(r"\[\d+\]", "", n.strip()) for n in decl.split(",")]
    assert names == [f[0] for f in orb.FramePose._fields_]
    assert C.sizeof(orb.FramePose) == 88


def test_refuses_without_device(lib):
    from visual_sgraphs_amd import orb
    h = C.c_void_p()
    assert lib.vsg_mappoints_create(0, 0, C.byref(h)) == -6 and lib.vsg_mappoints_create(0, 16, None) == -6
    assert lib.vsg_mappoints_capacity(None) == -6
    assert lib.vsg_mappoints_update(None, 1, None, None, None, None, None, None, None) == -6
    assert lib.vsg_frame_is_in_frustum(None, None, 0, None, None, 0.5, None, None, None, None, None, None, None) == -6
    if lib.vsg_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(orb.VsgError) as e:
        orb.MapPoints(100)
    assert e.value.code == -4  # VSG_ERR_NO_DEVICE: no CPU fallback


def test_cpp_adaptor_compiles_and_fails_loudly_without_device(lib):
    subprocess.check_call(["make", "-C", str(ADAPTOR)], stdout=subprocess.DEVNULL)
    if lib.vsg_device_count() > 0:
        pytest.skip("a GPU is present")
    r = subprocess.run([str(ADAPTOR / "mappoints_check"), "/dev/null", "/dev/null"], capture_output=True, text=True)
    assert r.returncode == 3 and "no CPU fallback" in r.stdout


def _blob(a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    return np.int32(a.size if a.dtype.names is None else len(a)).tobytes() + a.tobytes()


def _load(buf, pos, dtype):
    n = int(np.frombuffer(buf, np.int32, 1, pos)[0])
    a = np.frombuffer(buf, dtype, n, pos + 4)
    return a, pos + 4 + a.nbytes


@pytest.mark.gpu
@pytest.mark.parametrize("stereo", [False, True], ids=["mono", "uright"])
def test_cpp_adaptor_equals_reference_and_python_binding(tmp_path, stereo):
    from visual_sgraphs_amd import orb
    subprocess.check_call(["make", "-C", str(ADAPTOR)], stdout=subprocess.DEVNULL)
    rng = np.random.default_rng(17)
    pose, bounds, f = fr.scenario(5, "tum1", n=2500)
    ref0 = fr.is_in_frustum(pose, bounds, f["world_pos"], f["normal"], f["min_dist"], f["max_dist"])
    fr.check_scenario(ref0)
    # a frame whose features sit where the in-view points project, with their descriptors slightly changed
    iv = np.flatnonzero(ref0["in_view"])
    keys = np.zeros(len(iv), orb.KP_DTYPE)
    keys["x"] = ref0["proj_x"][iv] + rng.normal(0, 0.5, len(iv)).astype(np.float32)
    keys["y"] = ref0["proj_y"][iv] + rng.normal(0, 0.5, len(iv)).astype(np.float32)
    keys["octave"] = np.maximum(ref0["scale_level"][iv] - rng.integers(0, 2, len(iv)), 0)
    desc = f["desc"][iv].copy()
    desc[:, 0] ^= rng.integers(0, 256, len(iv), dtype=np.uint8)
    ur = (ref0["proj_xr"][iv] + np.where(rng.random(len(iv)) < 0.3, 40.0, 0.0)).astype(np.float32) if stereo else None
    skip = (rng.random(len(f["desc"])) < 0.2).astype(np.uint8)
    th, nnratio = 3.0, 0.8
    th_far = float(np.quantile(ref0["depth"][iv], 0.75))
    sf = (np.float32(1.2) ** np.arange(8, dtype=np.float32)).astype(np.float32)
    cam = np.concatenate([pose["Rcw"].reshape(9), pose["tcw"], pose["Ow"],
                          [pose[k] for k in ("fx", "fy", "cx", "cy", "mbf", "log_scale_factor")]]).astype(np.float32)
    src, out = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(b"".join([
        _blob(cam, np.float32), _blob([pose["n_levels"], 1], np.int32), _blob(list(bounds) + [th, nnratio, th_far], np.float32),
        _blob(sf, np.float32), _blob(keys, orb.KP_DTYPE), _blob(desc, np.uint8),
        _blob(ur if stereo else np.zeros(0), np.float32), _blob(f["world_pos"], np.float32), _blob(f["normal"], np.float32),
        _blob(f["min_dist"], np.float32), _blob(f["max_dist"], np.float32), _blob(f["desc"], np.uint8),
        _blob(f["observed"], np.uint8), _blob(skip, np.uint8)]))
    r = subprocess.run([str(ADAPTOR / "mappoints_check"), str(src), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    buf, pos = out.read_bytes(), 0
    got = {}
    for name, dt in (("head", np.int32), ("in_view", np.uint8), ("proj_x", np.float32), ("proj_y", np.float32),
                     ("proj_xr", np.float32), ("depth", np.float32), ("scale_level", np.int32), ("view_cos", np.float32),
                     ("train_match", np.int32), ("blocked", np.uint8), ("lp_in_view", np.uint8), ("lp_x", np.float32),
                     ("lp_y", np.float32)):
        got[name], pos = _load(buf, pos, dt)
    assert pos == len(buf)
    nm, n_to_match, cap, N = got["head"].tolist()
    assert cap == 2 * len(skip) + 1 and N == len(keys)
    # isInFrustum (no skip) against the reference
    assert np.array_equal(got["in_view"], ref0["in_view"])
    for k in ("proj_x", "proj_y"):
        assert got[k].tobytes() == ref0[k].tobytes(), k
    m = ref0["in_view"] != 0
    for k in ("proj_xr", "depth", "view_cos", "scale_level"):
        assert got[k][m].tobytes() == ref0[k][m].tobytes(), k
    # SearchLocalPoints against the existing search fed with the reference's fields, and against the Python binding
    ref = fr.is_in_frustum(pose, bounds, f["world_pos"], f["normal"], f["min_dist"], f["max_dist"], skip=skip)
    F = orb.Frame(len(keys) + 1)
    F.upload(keys, desc, bounds, u_right=ur)
    want = F.SearchByProjection(fr.search_fields(ref, f["desc"], f["observed"], th_far), th, nnratio, sf,
                                np.zeros(len(keys), np.uint8))
    assert want[0] >= 0.1 * ref["in_view"].sum()
    assert nm == want[0] and np.array_equal(got["train_match"], want[1]) and np.array_equal(got["blocked"], want[2])
    assert n_to_match == int(ref["in_view"].sum()) and np.array_equal(got["lp_in_view"], ref["in_view"])
    assert got["lp_x"].tobytes() == ref["proj_x"].tobytes() and got["lp_y"].tobytes() == ref["proj_y"].tobytes()
    mp = orb.MapPoints(len(skip))
    mp.update(np.arange(len(skip)), **{k: f[k] for k in ("world_pos", "normal", "min_dist", "max_dist", "desc", "observed")})
    py = F.SearchLocalPoints(mp, orb.FramePose.make(**pose), th, nnratio, sf, np.zeros(len(keys), np.uint8), skip=skip,
                             far_points=True, th_far_points=th_far)
    assert py[0] == nm and np.array_equal(py[1], got["train_match"]) and py[6] == n_to_match
