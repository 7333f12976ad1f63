"""CPU companion of tests/test_gpu_frame_edges.py: the reach conditions of its cases, asserted with the oracle alone
(OracleFrame.grid() / features_in_area()), so that a generator change that silently stops reaching a kernel edge fails on
a machine without a GPU.  Also: the size-parametrised scenario builders keep today's inputs at their defaults."""
import numpy as np
import pytest

import frame_edge_routines as fe
import oracle_lib as ol
import scenarios as sc


def test_device_grid_image_reaches_the_global_memory_sort():
    img, k, d = sc.device_image_features()
    h, w = img.shape
    assert len(k) >= 4200
    for camera in sc.CAMERA_NAMES:
        cam = None if camera == "image" else ol.scaled_camera(camera, w, h)
        bounds = (0.0, 0.0, float(w), float(h)) if cam is None else ol.image_bounds(cam)
        for n in sc.DEVICE_NS:
            n = len(k) if n is None else n
            kun = ol.undistort_keypoints(k[:n], cam) if cam else k[:n]
            o = ol.OracleFrame(kun, d[:n], bounds)
            occ = sc.reach_device_grid(o, n)
            x, y, r = sc.densest_windows(o, bounds)
            lens = [len(o.features_in_area(x[i], y[i], r[i], kf_form=True)) for i in range(len(x))]
            assert max(lens) >= min(n, 8) and occ.sum() <= n


@pytest.mark.parametrize("stereo", [False, True])
def test_dense_case_reaches_big_and_mixed_chunks(stereo):
    fr, q, qr = sc.dense_case(stereo)
    nbig, nmix = sc.reach_dense(fr, q, False)
    assert nbig >= 20 and nmix >= 1
    if stereo:
        sc.reach_dense(fr, qr, True)
    else:
        ur = fr["u_right"]   # the uR > 0 / uR >= 0 gates differ at exactly 0.0
        assert (ur == 0.0).sum() > 100 and (ur == -1.0).sum() > 300 and (ur > 0).sum() > 1000


@pytest.mark.parametrize("n", [1000, 20000])
def test_large_window_case_hits_the_named_cell_counts(n):
    fr, q = sc.large_window_case(n)
    cells = sc.reach_large_windows(fr, q)
    o = sc.oracle_of(fr)
    i = cells.index(sc.GRID_COLS * sc.GRID_ROWS)
    assert len(o.features_in_area(q["u"][i], q["v"][i], q["radius"][i], kf_form=True)) >= int(0.9 * n)
    assert 0 < min(c for c in cells if c) < 64   # small windows between the large ones


def test_window_cells_is_the_oracles_window():
    """the helper's restatement of the window arithmetic agrees with the oracle: a feature is listed only inside it"""
    fr = sc.synthetic_frame(3, 4000, "uniform")
    o = sc.oracle_of(fr)
    cs, en = o.grid()
    cof = sc.cell_of_features(cs, en, 4000)
    q = sc.synthetic_queries(3, fr, 200, radius=(0.3, 400.0))
    for i in range(200):
        cnt, x0, x1, y0, y1 = sc.window_cells(fr["bounds"], q["u"][i], q["v"][i], q["radius"][i])
        lst = o.features_in_area(q["u"][i], q["v"][i], q["radius"][i], kf_form=True)
        assert cnt > 0 or len(lst) == 0
        cx, cy = cof[lst] // sc.GRID_ROWS, cof[lst] % sc.GRID_ROWS
        assert np.all((cx >= x0) & (cx <= x1) & (cy >= y0) & (cy <= y1))


def test_inline_case_has_the_lengths_around_the_slot():
    lens = sc.reach_inline(*sc.inline_case())
    long_ = [n > 16 for n in lens]
    assert sum(a != b for a, b in zip(long_, long_[1:])) >= 8   # short and long lists interleave
    assert sum(n for n in lens if n > 16) > 4 * len(lens)        # a thread's first call overflows its 4 entries per query


@pytest.mark.parametrize("n", [16385, 32767])
def test_packed_case_reaches_the_field_limits(n):
    case = sc.packed_case(n)
    assert sc.reach_packed(*case)
    assert len(case[0]["keys"]) == n and set(case[0]["keys"]["octave"]) == set(range(16))


def test_lattice_frames_sit_on_cell_boundaries_and_bounds():
    fr = sc.synthetic_frame(5, 3000, "lattice", bounds=sc.D435I_LIKE)
    b = fr["bounds"]
    k = fr["keys"]
    o = sc.oracle_of(fr)
    on_max = (k["x"] == np.float32(b[2])) | (k["y"] == np.float32(b[3]))
    assert on_max.sum() > 20 and ((k["x"] == np.float32(b[0])).sum() > 5)
    cs, en = o.grid()
    listed = np.zeros(len(k), bool)
    listed[en] = True
    assert not listed[on_max].any()                       # px == 64 / py == 48 are rejected
    assert listed[(k["x"] == np.float32(b[0])) & (k["y"] > b[1]) & (k["y"] < b[3])].all()


def test_size_parameters_scale_the_camera_and_the_frames():
    """(that the defaults still give the parent's inputs is shown by tests/test_gpu_frame.py passing unchanged)"""
    try:
        for cam in sc.CAMERA_NAMES:
            sc.use_camera(cam)
            assert sc.BOUNDS == ((0.0, 0.0, 320.0, 240.0) if cam == "image" else ol.image_bounds(ol.scaled_camera(cam, 320, 240)))
            sc.use_camera(cam, 752, 480)
            s = sc.local_map_scenario(1, True, 752, 480, 1200)
            assert len(s["keys"]) > 2000 and s["nleft"] > 1000 and sc.BOUNDS[2] > 700
    finally:
        sc.use_camera("image")


# ---------------------------------------------------------------------------------------------- floors, oracle alone
DENSE_RUNNERS = {"local": fe.run_local, "last": fe.run_last, "sim3": fe.run_sim3, "kf": fe.run_kf, "by_sim3": fe.run_by_sim3,
                 "fuse": fe.run_fuse, "fuse_no_ur": fe.run_fuse, "fuse_sim3": fe.run_fuse_sim3}


@pytest.mark.parametrize("routine", sorted(fe.DENSE_FLOORS))
def test_dense_case_match_count_floors(routine):
    fr, q, _ = sc.dense_case(False)
    if routine == "fuse_no_ur":
        fr = dict(fr, u_right=None)
    o = sc.oracle_of(fr)
    n = fe.run_init(None, o, fr) if routine == "init" else DENSE_RUNNERS[routine](None, o, fr, q)
    assert n >= fe.DENSE_FLOORS[routine], (routine, n)


def test_dense_case_right_grid_floors():
    fr, q, qr = sc.dense_case(True)
    o = sc.oracle_of(fr)
    assert max(fe.areas(None, o, qr["u"], qr["v"], qr["radius"], right=True)) >= 200
    assert fe.run_fuse(None, o, fr, qr, right=True) >= fe.DENSE_RIGHT_FLOORS["fuse_right"]
    assert fe.run_fuse(None, o, fr, q, right=False) >= fe.DENSE_RIGHT_FLOORS["fuse_left"]
    assert fe.run_local(None, o, fr, q, qr) >= fe.DENSE_RIGHT_FLOORS["local"]
    assert fe.run_last(None, o, fr, q, qr) >= fe.DENSE_RIGHT_FLOORS["last"]


@pytest.mark.parametrize("camera", sc.CAMERA_NAMES)
@pytest.mark.parametrize("geom", fe.GEOMETRIES, ids=lambda g: "%dx%d_%d" % g)
def test_production_geometry_floors(geom, camera):
    sc.use_camera(camera, geom[0], geom[1])
    try:
        counts = fe.production_counts(False, geom)
    finally:
        sc.use_camera("image")
    assert set(counts) == set(fe.PRODUCTION_FLOORS[geom])
    for name, floor in fe.PRODUCTION_FLOORS[geom].items():
        assert counts[name] >= floor, (name, counts[name], floor)


@pytest.mark.parametrize("split", ["0", "1", "n-1", "n"])
def test_stereo_split_cases_reach_both_sides(split):
    fr, q, qr = fe.split_case(split)
    o = sc.oracle_of(fr)
    ll = fe.areas(None, o, q["u"], q["v"], q["radius"], right=False)
    lr = fe.areas(None, o, qr["u"], qr["v"], qr["radius"], right=True)
    fe.reach_split(fr, q, qr, ll, lr)


@pytest.mark.parametrize("nq", fe.TAIL_NQ)
def test_query_tail_cases_mix_active_and_inactive(nq):
    fr, qq = fe.tail_case(nq)
    fe.reach_tail(fr, qq, fe.areas(None, sc.oracle_of(fr), qq["u"], qq["v"], qq["radius"]))


def test_rewrite_steps_change_size_and_side():
    """section h: the writers' frames differ in size by more than 10 x, cross kGridLdsMax twice, and the stereo / mvuRight
    steps have what a stale copy would show: a populated right grid, then none; mvuRight, then none"""
    _, k, d = sc.device_image_features()
    steps = fe.rewrite_uploads()
    sizes = [4500, len(steps[1]["keys"]), len(steps[2]["keys"]), 0, 1000, len(steps[5]["keys"]), len(k)]
    assert sizes == [4500, 40, 3000, 0, 1000, 2500, len(k)] and len(k) > 4096
    assert steps[2]["nleft"] == 1500 and len(sc.oracle_of(steps[2]).grid(True)[1]) > 1400
    assert steps[1]["u_right"] is not None and steps[5]["u_right"] is not None and steps[2]["u_right"] is None
    sc.reach_device_grid(ol.OracleFrame(k[:4500], d[:4500], (0.0, 0.0, 1280.0, 720.0)), 4500)


def test_sweep_seeds_cover_sizes_laws_splits_and_routines():
    """section j: over the 60 seeds every routine, law and bound is drawn, the sizes run from a handful to above 16384,
    stereo and mono frames both occur, and most seeds have candidates to compare"""
    cases = [fe.sweep_case(s) for s in range(60)]
    ns = [len(c[0]["keys"]) for c in cases]
    assert min(ns) <= 4 and max(ns) > 16384 and sum(4096 < n for n in ns) >= 5
    assert {c[3] for c in cases} == set(fe.SWEEP_ROUTINES)
    assert all(sum(c[3] == r for c in cases) >= 3 for r in fe.SWEEP_ROUTINES)
    assert {c[0]["bounds"] for c in cases} == {tuple(float(v) for v in b) for b in fe.SWEEP_BOUNDS}
    stereo = [c for c in cases if c[0]["nleft"] != -1]
    assert 8 <= len(stereo) <= 40 and any(c[0]["u_right"] is not None for c in cases)
    assert sum(np.diff(sc.oracle_of(c[0]).grid()[0]).max(initial=0) > 32 for c in cases) >= 8   # dense cells occur
    busy = 0
    for seed, (fr, nq, rad, routine) in enumerate(cases):
        q = sc.synthetic_queries(7200 + seed, fr, nq, radius=rad)
        busy += sum(fe.areas(None, sc.oracle_of(fr), q["u"], q["v"], q["radius"])) > 0
        assert not (routine == "by_sim3" and len(fr["keys"]) == 0)
    assert busy >= 40
