"""include/vsg_orb_adaptor.hpp's ResidentFrame::TrackWithMotionModel and ResidentFrame::TrackLocalMap from plain C++
(tests/_adaptor_track/track_check.cpp): the program builds against the header and the library without a device; under
`-m gpu` it runs both steps on a scene of tests/track_scenes.py, the motion-model step's slots feeding the local-map
step, and every output must equal the C ABI's through ctypes byte for byte."""
import copy
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
ADAPTOR = ROOT / "tests" / "_adaptor_track"
F32, I32, U8 = np.float32, np.int32, np.uint8


@pytest.fixture(scope="module")
def program():
    from visual_sgraphs_amd import orb
    orb.load_library()  # the library the program links against is built
    subprocess.check_call(["make", "-C", str(ADAPTOR)], stdout=subprocess.DEVNULL)
    return ADAPTOR / "track_check"


def test_the_check_program_builds_against_the_adaptor(program):
    assert program.exists()
    header = (ROOT / "include" / "vsg_orb_adaptor.hpp").read_text()
    for name in ("int TrackWithMotionModel(", "int TrackLocalMap(", "struct TrackMotionResult", "struct TrackLocalResult",
                 "vsg_frame_track_with_motion_model(", "vsg_frame_track_local_map("):
        assert name in header, name


@pytest.mark.gpu
@pytest.mark.parametrize("rgbd", [False, True], ids=["gray", "rgbd"])
def test_cpp_adaptor_gives_the_same_bytes(program, tmp_path, rgbd):
    import ctypes as C

    import projection_scenes as ps
    import test_gpu_track_local_map as tl
    import track_scenes as ts
    from visual_sgraphs_amd import orb

    ex = orb.ORBextractor(1000, 1.2, 8, 20, 7)
    loc = tl.Local(ex, 3, rgbd)
    s = loc.s
    # the C ABI's side runs on a frame uploaded from the same arrays the program uploads
    twin = copy.copy(loc)
    twin.s = copy.copy(s)
    twin.s.F = orb.Frame(s.n + 1).upload(s.F.kps, loc.desc, ts.BOUNDS, u_right=s.ur)
    want_m = twin.s.chain_motion(15)
    want_l = twin.chain(3, entry=want_m["feat_slots"], only_tracking=False, drop=True)
    assert want_m["optimized"] == 1 and want_l["n_matches_searched"] >= 100 and want_l["rounds_run"] == 4

    def block(a, t):
        a = np.ascontiguousarray(a, t)
        return np.array([a.size], I32).tobytes() + a.tobytes()
    per = ps.per_slot(s.fields, s.store_slots)
    pose_bytes = lambda p: np.frombuffer(bytes(memoryview(p)), U8)
    assert C.sizeof(orb.FramePose) == 88
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(
        block([s.mp.capacity, 0, 1, 0, 1], I32) + block([ps.MB, 15.0, 3.0, tl.NN], F32) +
        block(s.F.kps.view(U8), U8) + block(loc.desc, U8) + block(s.ur if s.ur is not None else np.zeros(0), F32) +
        block(s.lk.view(U8), U8) + block(np.zeros((len(s.lk), 32)), U8) + block(s.slots, I32) +
        block(per["world_pos"], F32) + block(per["normal"], F32) + block(per["min_dist"], F32) +
        block(per["max_dist"], F32) + block(per["desc"], U8) + block(per["observed"], U8) +
        block(pose_bytes(s.cp), U8) + block(pose_bytes(s.lp), U8) + block(np.concatenate([s.q, s.t]), F32) +
        block(s.sf, F32) + block(ts.SIG, F32) + block(loc.local, I32) + block(loc.seen, U8))
    subprocess.check_call([str(program), str(src), str(dst)], timeout=120)
    raw, at = dst.read_bytes(), 0

    def take(dtype, count):
        nonlocal at
        a = np.frombuffer(raw, dtype, count, at)
        at += a.nbytes
        return a
    n, nq = s.n, len(loc.local)
    head = take(I32, 12).tolist()
    assert head == [want_m[k] for k in ("ret", "n_search", "wide", "n_matches_searched", "optimized", "n_matches",
                                        "n_matches_map", "direction", "n_initial", "n_bad", "rounds_run", "held")]
    for k, t in (("feat_slots", I32), ("train_match", I32), ("outlier", U8), ("chi2", F32)):
        assert take(t, n).tobytes() == want_m[k].tobytes(), k
    assert take(np.float64, 4).tobytes() == want_m["q"].tobytes() and take(np.float64, 3).tobytes() == want_m["t"].tobytes()
    head = take(I32, 9).tolist()
    assert head == [want_l[k] for k in ("ret", "n_to_match", "n_matches_searched", "n_matches_inliers", "walk_rounds",
                                        "n_initial", "n_bad", "rounds_run", "held")]
    for k, t in (("feat_slots", I32), ("train_match", I32), ("outlier", U8), ("chi2", F32)):
        assert take(t, n).tobytes() == want_l[k].tobytes(), k
    for k, t in (("in_view", U8), ("proj_x", F32), ("proj_y", F32)):
        assert take(t, nq).tobytes() == want_l[k].tobytes(), k
    assert take(np.float64, 4).tobytes() == want_l["q"].tobytes() and take(np.float64, 3).tobytes() == want_l["t"].tobytes()
    assert at == len(raw)
