"""The resident-frame kernels (k_frame_grid_build: visual_sgraphs_amd/csrc/vsg_frame.hip, k_window_search:
csrc/vsg_window.hip) at their edges
instead of at their typical shape: device-built grids across kGridLdsMax, cells of more than 32 entries under every gate,
windows of more than 64 cells, candidate lists around the inline slot, the overflow retry from a fresh thread, the packed
candidate word at its field limits, degenerate stereo splits, query-count tails, one frame rewritten at changing sizes,
production geometries and a seeded sweep.  The reference is always the CPU oracle (oracle_lib.OracleFrame); integers and
indices equal, floats bit for bit.  Every case's reach condition lives beside its inputs in tests/scenarios.py and is
asserted here and, on the CPU alone, in tests/test_frame_edge_scenarios.py."""
import threading

import numpy as np
import pytest

import oracle_lib as ol
import scenarios as sc
from frame_edge_routines import (DENSE_FLOORS, DENSE_RIGHT_FLOORS, GEOMETRIES, PRODUCTION_FLOORS, S16, areas, levels_of, production_counts,
                                 resident, run_by_sim3, run_fuse, run_fuse_sim3, run_init, run_kf, run_last, run_local,
                                 run_sim3, same, TAIL_NQ, reach_split, reach_tail, rewrite_uploads, split_case, sweep_case,
                                 tail_case)
from visual_sgraphs_amd import orb

pytestmark = pytest.mark.gpu


def in_thread(fn):
    """run fn on a freshly started host thread (its own stream, arena and candidate-stride hint); re-raise what it raised"""
    box = []

    def run():
        try:
            box.append(("ok", fn()))
        except BaseException as e:  # noqa: BLE001
            box.append(("err", e))
        finally:
            orb.load_library().vsg_thread_release()
    t = threading.Thread(target=run)
    t.start()
    t.join()
    if box[0][0] == "err":
        raise box[0][1]
    return box[0][1]


# ---------------------------------------------------------------------------------------------- a. device-built grids
@pytest.fixture(scope="module")
def big_extraction():
    img, rk, rd = sc.device_image_features()
    assert len(rk) >= 4200
    ex = orb.ORBextractor(6000, 1.2, 8, 20, 7)
    _, k, d = ex(img)
    assert k.tobytes() == rk.tobytes() and np.array_equal(d, rd)
    # every test that uses from_extractor* re-runs ex(img) first: the fixture's extractor is shared, and from_extractor reads
    # the outputs of its LAST call
    return ex, img, k, d


@pytest.mark.parametrize("camera", sc.CAMERA_NAMES)
@pytest.mark.parametrize("n", sc.DEVICE_NS)
def test_device_built_grid_across_the_lds_limit(big_extraction, n, camera):
    """k_frame_grid_build for the first n records of a > 4200-keypoint extraction: up to kGridLdsMax = 4096 keypoints the
    cells are ordered in LDS, above it where they lie in global memory; n = 1023 / 1024 / 1025 walk its strided loops."""
    ex, img, k, d = big_extraction
    h, w = img.shape
    n = len(k) if n is None else n
    cam = None if camera == "image" else ol.scaled_camera(camera, w, h)
    bounds = (0.0, 0.0, float(w), float(h)) if cam is None else ol.image_bounds(cam)
    f = orb.Frame(ex.capacity(h, w))
    ex(img)
    if cam is None:
        f.from_extractor(ex, 0, k, bounds, n=n)
        kun = k[:n]
    else:
        assert orb.camera_image_bounds(w, h, cam["K4"], cam["dist"]) == bounds
        f.from_extractor_undistort(ex, 0, k, cam["K4"], cam["dist"], bounds, n=n)
        kun = ol.undistort_keypoints(k[:n], cam)
    o = ol.OracleFrame(kun, d[:n], bounds)
    sc.reach_device_grid(o, n)
    assert f.N == n and f.kps.tobytes() == kun.tobytes()
    cs, en = f.grid(False)
    ocs, oen = o.grid(False)
    assert np.array_equal(cs, ocs) and np.array_equal(en, oen)
    rcs, ren = f.grid(True)
    assert not rcs.any() and len(ren) == 0
    x, y, r = sc.densest_windows(o, bounds)
    lens = areas(f, o, x, y, r)
    assert max(lens) >= min(n, 8)
    rng = np.random.default_rng(n)
    src = rng.integers(0, n, len(x))
    q = dict(q_desc=sc.noisy_desc(rng, d[src], 6), u=x, v=y, radius=r, level=np.clip(kun["octave"][src], 0, 7).astype(np.int32))
    run_sim3(f, o, dict(keys=kun), q, ratio=2.0)


@pytest.mark.parametrize("camera", sc.CAMERA_NAMES)
def test_extract_into_above_the_lds_limit(big_extraction, camera):
    """the same grid launch riding behind operator()'s chain (the count is read on the device), gray and RGB-D"""
    import rgbd_reference as rr
    ex, img, k, d = big_extraction
    h, w = img.shape
    cam = None if camera == "image" else ol.scaled_camera(camera, w, h)
    bounds = (0.0, 0.0, float(w), float(h)) if cam is None else ol.image_bounds(cam)
    K4, dist = (cam["K4"], cam["dist"]) if cam else (None, None)
    kun = ol.undistort_keypoints(k, cam) if cam else k
    o = ol.OracleFrame(kun, d, bounds)
    sc.reach_device_grid(o, len(k))
    f = orb.Frame(ex.capacity(h, w))
    depth = (np.random.default_rng(5).integers(0, 9000, (h, w))).astype(np.uint16)
    depth[::7, ::5] = 0
    for rgbd in (False, True):
        if rgbd:
            mono, gk, gd, ur, dep = f.extract_into_rgbd(ex, img, depth, bounds, K4, dist, orb.depth_map_scale(5000.0), 40.0)
            want_ur, want_dep = rr.rgbd_frame(k, kun, depth, orb.depth_map_scale(5000.0), 40.0)
            assert ur.tobytes() == want_ur.tobytes() and dep.tobytes() == want_dep.tobytes()
            assert (want_ur > 0).sum() > 1000 and (want_ur < 0).sum() > 10
        else:
            mono, gk, gd = f.extract_into(ex, img, bounds, K4, dist)
        assert gk.tobytes() == k.tobytes() and np.array_equal(gd, d) and f.N == len(k)
        assert f.kps.tobytes() == kun.tobytes()
        assert all(np.array_equal(a, b) for a, b in zip(f.grid(), o.grid()))
        assert not f.grid(True)[0].any()
        x, y, r = sc.densest_windows(o, bounds)
        areas(f, o, x, y, r)


# ---------------------------------------------------------------------------------------------- b. dense cells
@pytest.mark.parametrize("routine", ["area", "local", "last", "sim3", "kf", "by_sim3", "fuse", "fuse_no_ur", "fuse_sim3",
                                     "init"])
def test_dense_cells_left_grid(routine):
    """cells of 33-200 entries (the kernel's two-pass filter) beside cells of 1-32 (its bit mask) on a frame with mvuRight:
    kGateUr in SearchByProjection (local map / last frame), kGateChi2 in Fuse, no gate elsewhere"""
    fr, q, _ = sc.dense_case(False)
    sc.reach_dense(fr, q, False)
    if routine == "fuse_no_ur":
        fr = dict(fr, u_right=None)
    f, o = resident(fr)
    if routine == "area":
        lens = areas(f, o, q["u"], q["v"], q["radius"], *levels_of(q))
        assert max(lens) >= 200
        return
    n = {"local": run_local, "last": run_last, "sim3": run_sim3, "kf": run_kf, "by_sim3": run_by_sim3, "fuse": run_fuse,
         "fuse_no_ur": run_fuse, "fuse_sim3": run_fuse_sim3}[routine](f, o, fr, q) if routine != "init" else run_init(f, o, fr)
    assert n >= DENSE_FLOORS[routine], n


@pytest.mark.parametrize("routine", ["area", "local", "last", "fuse"])
def test_dense_cells_right_grid(routine):
    """the same on a fisheye-stereo frame (Nleft != -1): mGridRight with cells of up to 200 entries, indices + Nleft"""
    fr, q, qr = sc.dense_case(True)
    sc.reach_dense(fr, q, False)
    sc.reach_dense(fr, qr, True)
    f, o = resident(fr)
    if routine == "area":
        assert max(areas(f, o, qr["u"], qr["v"], qr["radius"], *levels_of(qr), right=True)) >= 200
    elif routine == "fuse":
        assert run_fuse(f, o, fr, qr, right=True) >= DENSE_RIGHT_FLOORS["fuse_right"]
        assert run_fuse(f, o, fr, q, right=False) >= DENSE_RIGHT_FLOORS["fuse_left"]
    else:
        n = (run_local if routine == "local" else run_last)(f, o, fr, q, qr)
        assert n >= DENSE_RIGHT_FLOORS[routine], n


# ---------------------------------------------------------------------------------------------- c. large windows
@pytest.mark.parametrize("n", [1000, 20000])
def test_windows_of_65_to_3072_cells(n):
    """the c0 += 64 loop with its running count: windows of 65, 128, 129 and all 3072 cells between small ones, list mode
    (GetFeaturesInArea x2, SearchByProjection_Sim3 / _KF) and best mode (Fuse x2, SearchBySim3)"""
    fr, q = sc.large_window_case(n)
    sc.reach_large_windows(fr, q)
    f, o = resident(fr)
    lens = areas(f, o, q["u"], q["v"], q["radius"], *levels_of(q))
    assert max(lens) >= int(0.9 * n)   # the whole-grid window lists (nearly) every feature
    run_sim3(f, o, fr, q, ratio=1.5)
    run_kf(f, o, fr, q)
    assert run_fuse_sim3(f, o, fr, q) >= 5
    run_fuse(f, o, fr, q)
    run_by_sim3(f, o, fr, q)


# ---------------------------------------------------------------------------------------------- d / e. inline slot, retry
def inline_checks(f, o, fr, q):
    lens = areas(f, o, q["u"], q["v"], q["radius"], *levels_of(q))
    assert tuple(lens) == sc.INLINE_LENGTHS
    assert run_last(f, o, fr, dict(q, ur=None), th=3.0 / float(S16[3])) >= 10
    return lens


def test_candidate_lists_around_the_inline_slot():
    """lists of exactly 0, 1, 15, 16, 17, 18 and >= 200 entries in one call, short and long interleaved: the inline slot
    of kInline = 16 entries against the overflow segment"""
    fr, q = sc.inline_case()
    sc.reach_inline(fr, q)
    f, o = resident(fr)
    inline_checks(f, o, fr, q)


def test_overflow_retry_from_a_fresh_thread():
    """a new host thread starts with the smallest candidate stride: its first long-list call overflows and is re-run
    (WindowCall::finish -> with_retry); the second identical call is not; a small call after them shows the never-reset
    device counter's base is still right"""
    fr, q = sc.inline_case()
    sc.reach_inline(fr, q)
    fd, qd, _ = sc.dense_case(False)
    f, o = resident(fr)
    f2, o2 = resident(fd)

    def body():
        # 16 queries x the initial 4 entries = room for 64 < the 617 entries of the lists longer than the inline slot (the CPU
        # companion asserts that sum): the call is re-run with a larger stride.  The library exposes no retry counter (the
        # arena grows in 64 KiB steps, far above this call); what shows is the result after the re-run and the base of the
        # never-reset counter in the calls that follow
        inline_checks(f, o, fr, q)
        inline_checks(f, o, fr, q)        # fits now
        small = [0, 4, 1]                 # 17 + 1 + 0 entries: one overflow segment, no retry
        areas(f, o, q["u"][small], q["v"][small], q["radius"][small])
        n1 = run_local(f2, o2, fd, qd)    # dense lists under kGateUr: grows again
        n2 = run_local(f2, o2, fd, qd)
        areas(f, o, q["u"][small], q["v"][small], q["radius"][small])
        assert n1 == n2 >= 40
    in_thread(body)


# ---------------------------------------------------------------------------------------------- f. packed fields
@pytest.fixture(scope="module", params=[16385, 32767])
def packed(request):
    case = sc.packed_case(request.param)
    sc.reach_packed(*case)
    f, o = resident(case[0], cap=32767 if request.param == 32767 else 20000)
    return case, f, o


def test_packed_candidate_word_at_its_field_limits(packed):
    """index : 15 | distance : 9 | octave : 4 with index >= 16384 (and capacity - 1 = 32766), distances 255 / 256 and
    octave 15 in the same lists.  SearchByProjection(F, vpMapPoints) reads all three fields of every candidate: a distance of
    256 read through 8 bits is 0 and wins, an index read through 14 bits claims another feature."""
    (fr, mp, src, kinds, inside), f, o = packed
    n = len(fr["keys"])
    blocked = np.zeros(n, np.uint8)
    a = (mp, 3.0, 0.8, S16, blocked)
    got, ref = f.SearchByProjection(*a), o.search_by_projection(*a)
    assert same(got, ref) >= 25
    assert ref[1].max() >= len(mp["desc"]) // 2 and np.nonzero(ref[1] >= 0)[0].max() >= 16384
    assert not np.isin(ref[1][ref[1] >= 0], np.nonzero(kinds < 0)[0]).any()   # distances 255 / 256 never match
    q = dict(q_desc=mp["desc"], u=mp["proj_x"], v=mp["proj_y"], ur=mp["proj_x"] - np.float32(4),
             radius=(np.float32(12) * S16[mp["scale_level"]]).astype(np.float32), level=mp["scale_level"], src=src,
             angle=fr["keys"]["angle"][src].astype(np.float32), observed=mp["observed"])
    lens = areas(f, o, q["u"], q["v"], q["radius"], *levels_of(q))
    assert max(lens) >= 200
    assert run_last(f, o, fr, q, th=12.0) >= 25
    run_sim3(f, o, fr, q, ratio=2.5)      # 100 * 2.5 = 250: distances up to 250 match, 255 / 256 do not
    run_fuse(f, o, fr, q)                 # inv_sigma2[15]
    run_fuse_sim3(f, o, fr, q)            # best mode: the best distance may be 255 / 256
    run_by_sim3(f, o, fr, q)


def test_frame_capacity_limits():
    with pytest.raises(orb.VsgError) as e:
        orb.Frame(32768)
    assert e.value.code == -6   # VSG_ERR_INVALID
    fr = sc.synthetic_frame(72, 300, "uniform")
    f, o = resident(fr, cap=300)   # n == capacity
    assert f.N == 300 and all(np.array_equal(a, b) for a, b in zip(f.grid(), o.grid()))
    with pytest.raises(orb.VsgError):
        orb.Frame(299).upload(fr["keys"], fr["desc"], fr["bounds"])


# ---------------------------------------------------------------------------------------------- g. splits and tails
@pytest.mark.parametrize("split", ["0", "1", "n-1", "n"])
def test_degenerate_stereo_splits(split):
    fr, q, qr = split_case(split)
    n, nleft = len(fr["keys"]), fr["nleft"]
    f, o = resident(fr)
    for right in (False, True):
        cs, en = f.grid(right)
        ocs, oen = o.grid(right)
        assert np.array_equal(cs, ocs) and np.array_equal(en, oen)
    assert len(o.grid(False)[1]) <= nleft and len(o.grid(True)[1]) <= n - nleft
    ll = areas(f, o, q["u"], q["v"], q["radius"], *levels_of(q), right=False)
    lr = areas(f, o, qr["u"], qr["v"], qr["radius"], *levels_of(qr), right=True)
    reach_split(fr, q, qr, ll, lr)
    run_local(f, o, fr, q, qr)
    run_last(f, o, fr, q, qr)
    run_fuse(f, o, fr, qr, right=True)
    run_fuse(f, o, fr, q, right=False)


@pytest.mark.parametrize("nq", TAIL_NQ)
def test_query_count_tails(nq):
    """four queries per workgroup: the q < nq tail, with queries the host flags inactive between active ones"""
    fr, qq = tail_case(nq)
    f, o = resident(fr)
    reach_tail(fr, qq, areas(f, o, qq["u"], qq["v"], qq["radius"]))
    run_local(f, o, fr, qq)
    run_fuse(f, o, fr, qq)
    run_fuse_sim3(f, o, fr, qq)
    run_sim3(f, o, fr, qq)
    observed = dict(qq, observed=(np.arange(nq) % 2).astype(np.uint8), level=np.maximum(qq["level"], 0))
    run_last(f, o, fr, observed)


# ---------------------------------------------------------------------------------------------- h. one frame rewritten
def test_one_frame_rewritten_by_every_writer(big_extraction):
    """device-built 4500 -> upload 40 -> fisheye-stereo 1500 + 1500 -> extract_into (0 features) -> device-built 1000
    under a distorted camera -> upload with mvuRight -> extract_into: after every step both grids and a left and a right
    window search equal an oracle frame of exactly the current contents (no stale right grid, mvuRight or entry tail)"""
    ex, img, k, d = big_extraction
    h, w = img.shape
    b0 = (0.0, 0.0, float(w), float(h))
    cam = ol.scaled_camera("tum1", w, h)
    bc = ol.image_bounds(cam)
    f = orb.Frame(8192)
    uploads = rewrite_uploads()

    def step(i):
        if i == 0:
            ex(img)
            f.from_extractor(ex, 0, k, b0, n=4500)
            return dict(keys=k[:4500], desc=d[:4500], u_right=None, nleft=-1, bounds=b0)
        if i in (1, 2, 5):
            fr = uploads[i]
            f.upload(fr["keys"], fr["desc"], fr["bounds"], fr["u_right"], fr["nleft"])
            return fr
        if i == 3:
            _, gk, gd = f.extract_into(ex, np.full((h, w), 90, np.uint8), b0)
            assert len(gk) == 0
            return dict(keys=gk, desc=gd, u_right=None, nleft=-1, bounds=b0)
        if i == 4:
            ex(img)
            f.from_extractor_undistort(ex, 0, k, cam["K4"], cam["dist"], bc, n=1000)
            return dict(keys=ol.undistort_keypoints(k[:1000], cam), desc=d[:1000], u_right=None, nleft=-1, bounds=bc)
        _, gk, gd = f.extract_into(ex, img, b0)
        assert gk.tobytes() == k.tobytes()
        return dict(keys=gk, desc=gd, u_right=None, nleft=-1, bounds=b0)

    for i in range(7):
        fr = step(i)
        o = sc.oracle_of(fr)
        n = len(fr["keys"])
        assert f.N == n and f.kps.tobytes() == np.ascontiguousarray(fr["keys"], orb.KP_DTYPE).tobytes(), i
        for right in (False, True):
            cs, en = f.grid(right)
            ocs, oen = o.grid(right)
            assert np.array_equal(cs, ocs) and np.array_equal(en, oen), (i, right)
        q = sc.synthetic_queries(93 + i, fr, 120, max_level=7 if i in (0, 3, 4, 6) else 15)
        qr = sc.synthetic_queries(103 + i, fr, 120, right=True)
        q["level"] = np.maximum(q["level"], 0)
        # left: the last-frame search reads mvuRight where the frame has it (kGateUr); right: the right grid's lists
        if n:
            run_last(f, o, fr, q, qr)
        areas(f, o, q["u"], q["v"], q["radius"])
        in_thread(lambda: areas(f, o, qr["u"], qr["v"], qr["radius"], right=True))


# ---------------------------------------------------------------------------------------------- i. production geometries
@pytest.mark.parametrize("camera", sc.CAMERA_NAMES)
@pytest.mark.parametrize("geom", GEOMETRIES, ids=lambda g: "%dx%d_%d" % g)
def test_routines_at_production_geometries(geom, camera):
    """BASELINE configs C2-C5: 640x480 / 1000, 752x480 / 1200 (and its 2 x 1200 fisheye-stereo form), 1280x720 / 2000"""
    sc.use_camera(camera, geom[0], geom[1])
    try:
        counts = production_counts(True, geom)
    finally:
        sc.use_camera("image")
    for name, floor in PRODUCTION_FLOORS[geom].items():
        assert counts[name] >= floor, (name, counts[name], floor)


# ---------------------------------------------------------------------------------------------- j. seeded sweep
@pytest.mark.parametrize("seed", range(60))
def test_seeded_sweep(seed):
    fr, nq, rad, routine = sweep_case(seed)
    n, nleft = len(fr["keys"]), fr["nleft"]
    q = sc.synthetic_queries(7200 + seed, fr, nq, radius=rad)
    qr = sc.synthetic_queries(7300 + seed, fr, nq, radius=rad, right=True)
    f, o = resident(fr)
    what = "seed %d: n %d nleft %d nq %d %s radius %s" % (seed, n, nleft, nq, routine, rad)
    try:
        for right in (False, True):
            cs, en = f.grid(right)
            ocs, oen = o.grid(right)
            assert np.array_equal(cs, ocs) and np.array_equal(en, oen), "grid"
        if routine == "area":
            areas(f, o, q["u"], q["v"], q["radius"], *levels_of(q))
            areas(f, o, qr["u"], qr["v"], qr["radius"], *levels_of(qr), right=True)
        elif routine == "local":
            run_local(f, o, fr, q, qr)
        elif routine == "last":
            run_last(f, o, fr, q, qr, direction=seed % 3)
        elif routine == "fuse":
            run_fuse(f, o, fr, q)
            if nleft != -1:
                run_fuse(f, o, fr, qr, right=True)
        elif routine == "init":
            run_init(f, o, fr, window=int(rad[1]))
        else:
            {"sim3": run_sim3, "kf": run_kf, "by_sim3": run_by_sim3, "fuse_sim3": run_fuse_sim3}[routine](f, o, fr, q)
    except AssertionError as e:
        raise AssertionError("%s: %s" % (what, e)) from e
