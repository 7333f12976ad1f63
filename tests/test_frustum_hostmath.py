"""CPU tests of the product's host-and-device arithmetic of the resident map-point path, compiled for the host by
tests/_frustumcore: vsg_math.h's logf against the host's libm over EVERY float of [2^-6, 2^8), and vsg_frustum.h's
isInFrustum against tests/frustum_reference.py bit for bit."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import frustum_reference as fr
from visual_sgraphs_amd import orb

FC_DIR = Path(__file__).resolve().parent / "_frustumcore"
_f32p, _u8p, _i32p, _u32p = (C.POINTER(t) for t in (C.c_float, C.c_uint8, C.c_int32, C.c_uint32))


@pytest.fixture(scope="module")
def fc():
    subprocess.check_call(["make", "-C", str(FC_DIR)], stdout=subprocess.DEVNULL)
    L = C.CDLL(str(FC_DIR / "libvsg_frustumcore.so"))
    L.fc_logf.restype = C.c_float
    L.fc_logf.argtypes = [C.c_float, C.c_int]
    L.fc_log_f32.restype = C.c_float
    L.fc_log_f32.argtypes = [C.c_float]
    L.fc_logf_sweep.restype = None
    L.fc_logf_sweep.argtypes = [C.c_uint32, C.c_uint32, _f32p, C.c_int, C.c_int, C.POINTER(C.c_longlong), _u32p, C.c_int]
    L.fc_frustum.restype = None
    L.fc_frustum.argtypes = [C.POINTER(orb.FramePose), _f32p, C.c_float, C.c_int, _f32p, _f32p, _f32p, _f32p, _u8p, _f32p,
                             _f32p, _f32p, _f32p, _i32p, _f32p]
    return L


def bits(x):
    return int(np.float32(x).view(np.uint32))


def test_logf_matches_libm_for_every_float_of_the_level_range(fc):
    """Every float of [2^-6, 2^8) (117 440 512 values): the predicted level clamp((int)ceilf(logf(r) / logf(s))) must be
    equal for every one of them and every scale factor (1.2: all 51 reference configs; 1.1, 1.5: guards).  Bit equality of
    logf itself is expected: the mismatches are counted and printed."""
    sf = np.array([1.2, 1.1, 1.5], np.float32)
    counts = (C.c_longlong * 8)()
    first = np.zeros(8, np.uint32)
    lo, hi = bits(2.0 ** -6), bits(2.0 ** 8)
    fc.fc_logf_sweep(lo, hi, sf.ctypes.data_as(_f32p), len(sf), 8, counts, first.ctypes.data_as(_u32p), len(first))
    n, mis_plain, mis_fma = counts[0], counts[1], counts[2]
    print(f"logf sweep: {n} values, bit mismatches against libm: uncontracted {mis_plain}, fma {mis_fma}; "
          f"level mismatches {[counts[3 + k] for k in range(len(sf))]}")
    for u in first[:min(len(first), mis_plain + mis_fma)]:
        x = np.uint32(u).view(np.float32)
        print("  first mismatches: x =", float(x).hex(), "libm", float(fr.logf(x)).hex(), "uncontracted",
              float(fc.fc_logf(x, 0)).hex(), "fma", float(fc.fc_logf(x, 1)).hex())
    assert n == hi - lo == 117440512
    assert [counts[3 + k] for k in range(len(sf))] == [0, 0, 0]
    assert mis_plain == 0 and mis_fma == 0


def test_logf_special_values_and_spot_checks(fc):
    rng = np.random.default_rng(5)
    xs = np.concatenate([rng.uniform(0, 1e-3, 2000), rng.uniform(1e3, 3e38, 2000), 2.0 ** rng.uniform(-149, 127, 4000),
                         [1.0, 1e-45, 1e-40, 3.4e38, np.float32(1.2), np.float32(1.1)]]).astype(np.float32)
    for x in xs:
        assert bits(fc.fc_log_f32(x)) == bits(fr.logf(x)), float(x).hex()
    assert fc.fc_log_f32(0.0) == -np.inf and fc.fc_log_f32(-0.0) == -np.inf and fc.fc_log_f32(np.inf) == np.inf
    assert np.isnan(fc.fc_log_f32(-1.0)) and np.isnan(fc.fc_log_f32(np.nan))


def host_frustum(fc, pose, bounds, f, limit=0.5):
    n = len(f["world_pos"])
    p = orb.FramePose.make(**pose)
    b = np.array(bounds, np.float32)
    out = dict(in_view=np.zeros(n, np.uint8), proj_x=np.zeros(n, np.float32), proj_y=np.zeros(n, np.float32),
               proj_xr=np.zeros(n, np.float32), depth=np.zeros(n, np.float32), scale_level=np.zeros(n, np.int32),
               view_cos=np.zeros(n, np.float32))
    a = {k: np.ascontiguousarray(f[k], np.float32) for k in ("world_pos", "normal", "min_dist", "max_dist")}
    fc.fc_frustum(C.byref(p), b.ctypes.data_as(_f32p), limit, n, a["world_pos"].ctypes.data_as(_f32p),
                  a["normal"].ctypes.data_as(_f32p), a["min_dist"].ctypes.data_as(_f32p),
                  a["max_dist"].ctypes.data_as(_f32p), out["in_view"].ctypes.data_as(_u8p),
                  out["proj_x"].ctypes.data_as(_f32p), out["proj_y"].ctypes.data_as(_f32p),
                  out["proj_xr"].ctypes.data_as(_f32p), out["depth"].ctypes.data_as(_f32p),
                  out["scale_level"].ctypes.data_as(_i32p), out["view_cos"].ctypes.data_as(_f32p))
    return out


def assert_frustum_equal(got, ref):
    """in_view for every point; the in-view points' fields as bit patterns; proj_x / proj_y of rejected points as the
    reference leaves them.  No tolerance, no point left out."""
    assert (got["in_view"] == ref["in_view"]).all()
    iv = ref["in_view"] != 0
    for k in ("proj_x", "proj_y", "proj_xr", "depth", "view_cos"):
        assert (got[k][iv].view(np.uint32) == ref[k][iv].view(np.uint32)).all(), k
    assert (got["scale_level"][iv] == ref["scale_level"][iv]).all()
    for k in ("proj_x", "proj_y"):
        assert (got[k][~iv].view(np.uint32) == ref[k][~iv].view(np.uint32)).all(), k


@pytest.mark.parametrize("camera", sorted(fr.CAMERAS))
def test_host_frustum_is_bit_equal_to_the_reference(fc, camera):
    for seed in range(8):
        pose, bounds, f = fr.scenario(seed, camera)
        ref = fr.is_in_frustum(pose, bounds, f["world_pos"], f["normal"], f["min_dist"], f["max_dist"])
        fr.check_scenario(ref)
        assert_frustum_equal(host_frustum(fc, pose, bounds, f), ref)


def test_host_frustum_edges(fc):
    """PcZ == 0, dist == 0, points on the bounds and the band's ends: decisions and levels as the reference (NaN fields
    compare as NaN)."""
    pose = fr.make_pose(np.eye(3), np.zeros(3), 512.0, 512.0, 320.0, 240.0, 40.0)
    P = np.array([(0, 0, 4), (-2.5, 0, 4), (2.5, 0, 4), (0, -1.875, 4), (0, 1.875, 4), (1, 0, 0), (0, 0, 0), (0, 0, -4),
                  (0, 0, 4), (0, 0, 4), (0, 0, 6)], np.float32)
    N = np.tile(np.array([0, 0, 1], np.float32), (len(P), 1))
    N[1:5] = P[1:5] / np.linalg.norm(P[1:5], axis=1, keepdims=True)
    N[9] = (0, np.sqrt(0.75), 0.5)
    f = dict(world_pos=P, normal=N, min_dist=np.array([.5, .5, .5, .5, .5, 0, 0, .5, 5, .5, .5], np.float32),
             max_dist=np.array([6, 6, 6, 6, 6, 6, 6, 6, 20, 6, 5], np.float32))
    ref = fr.is_in_frustum(pose, (0, 0, 640, 480), P, N, f["min_dist"], f["max_dist"])
    got = host_frustum(fc, pose, (0, 0, 640, 480), f)
    assert ref["in_view"].tolist() == [1, 1, 1, 1, 1, 0, 1, 0, 1, 1, 1]
    assert (got["in_view"] == ref["in_view"]).all()
    iv = ref["in_view"] != 0
    assert (got["scale_level"][iv] == ref["scale_level"][iv]).all()
    for k in ("proj_x", "proj_y", "proj_xr", "depth", "view_cos"):
        a, b = got[k][iv] if k not in ("proj_x", "proj_y") else got[k], ref[k][iv] if k not in ("proj_x", "proj_y") else ref[k]
        assert ((a == b) | (np.isnan(a) & np.isnan(b))).all(), k
