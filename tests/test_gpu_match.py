"""GPU parity tests of the Hamming searches (ORBmatcher) through the C ABI against the CPU oracle:
index pairs and distances identical, including tie-breaking and the greedy, order-dependent state."""
from pathlib import Path

import numpy as np
import pytest

import oracle_lib as ol
from visual_sgraphs_amd import orb, synth

pytestmark = pytest.mark.gpu

GOLDEN = np.load(Path(__file__).parent / "golden" / "orb_golden_v1.npz")


@pytest.fixture(scope="module")
def frames():
    """Two consecutive synthetic frames extracted by the oracle (matcher inputs)."""
    e = ol.OracleExtractor(1000, 1.2, 8, 20, 7)
    _, k0, d0 = e(synth.sequence_frame(640, 480, 3, 0))
    _, k1, d1 = e(synth.sequence_frame(640, 480, 3, 1))
    return (k0, d0), (k1, d1)


def make_fv(n, n_nodes, rng, drop=0.0):
    """Synthetic DBoW2 FeatureVector: node id per feature -> CSR with ascending node ids and, inside a node,
    ascending feature indices (FeatureVector::addFeature appends in feature order)."""
    node = rng.integers(0, n_nodes, n) * 7 + 3
    keep = rng.random(n) >= drop
    ids = np.unique(node[keep])
    off = [0]
    idx = []
    for i in ids:
        m = np.nonzero((node == i) & keep)[0]
        idx += m.tolist()
        off.append(len(idx))
    return ids.astype(np.int32), np.array(off, np.int32), np.array(idx, np.int32)


def near_duplicates(desc, rng, flips):
    """Descriptors at small Hamming distance from `desc` (so ratio tests and ties actually trigger)."""
    out = desc.copy()
    for r in range(len(out)):
        for b in rng.integers(0, 256, flips):
            out[r, b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def test_descriptor_distance_kats_and_random():
    m = orb.ORBmatcher()
    z = np.zeros(32, np.uint8)
    assert m.DescriptorDistance(z, z) == 0 and m.DescriptorDistance(z, ~z) == 256
    rng = np.random.default_rng(0)
    a, b = rng.integers(0, 256, (2, 500, 32), dtype=np.uint8)
    want = np.unpackbits(a ^ b, axis=1).sum(axis=1)
    assert np.array_equal(m.DescriptorDistance(a, b), want)
    ia, ib = rng.integers(0, 500, (2, 3000))
    got = m.hamming_pairs(a, b, ia, ib)
    assert np.array_equal(got, np.unpackbits(a[ia] ^ b[ib], axis=1).sum(axis=1))
    assert got.tolist()[:50] == [ol.descriptor_distance(a[i], b[j]) for i, j in zip(ia[:50], ib[:50])]


def test_block_best2_real_frames_and_golden(frames):
    (k0, d0), (k1, d1) = frames
    m = orb.ORBmatcher()
    got = m.block_best2(d0, d1)
    want = ol.block_best2(d0, d1)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    g = m.block_best2(GOLDEN["match/desc0"], GOLDEN["match/desc1"])
    assert np.array_equal(g[0], GOLDEN["match/best"]) and np.array_equal(g[1], GOLDEN["match/second"])
    assert np.array_equal(g[2], GOLDEN["match/arg"])


def test_block_best2_ties_and_ragged_sizes():
    rng = np.random.default_rng(1)
    m = orb.ORBmatcher()
    for na, nb in [(1, 1), (3, 700), (257, 256), (256, 257), (1000, 3), (513, 1025)]:
        # few distinct rows => many exact ties; first index must win
        base = rng.integers(0, 256, (5, 32), dtype=np.uint8)
        a = base[rng.integers(0, 5, na)]
        b = near_duplicates(base[rng.integers(0, 5, nb)], rng, 1)
        for g, w in zip(m.block_best2(a, b), ol.block_best2(a, b)):
            assert np.array_equal(g, w), (na, nb)
    best, second, arg = m.block_best2(np.zeros((4, 32), np.uint8), np.zeros((0, 32), np.uint8))
    assert best.tolist() == [256] * 4 and second.tolist() == [256] * 4 and arg.tolist() == [-1] * 4


@pytest.mark.parametrize("seed,n_nodes,ratio,ori", [(0, 60, 0.7, True), (1, 8, 0.75, True), (2, 300, 0.9, False),
                                                    (3, 1, 0.6, True)])
def test_search_by_bow_kf_f(frames, seed, n_nodes, ratio, ori):
    (k0, d0), (k1, d1) = frames
    rng = np.random.default_rng(seed)
    # F descriptors = KF descriptors with a few bit flips + shuffled, so many candidates pass TH_LOW / the ratio test
    perm = rng.permutation(len(d0))
    f_desc = near_duplicates(d0[perm], rng, 6)
    f_angle = (k0["angle"][perm] + rng.choice([0, 0, 0, 45, 200], len(perm))).astype(np.float32) % np.float32(360)
    kf_valid = (rng.random(len(d0)) > 0.2).astype(np.uint8)
    # same vocabulary node for a feature and its perturbed copy (most of the time)
    node_of_kf = rng.integers(0, n_nodes, len(d0))
    node_of_f = node_of_kf[perm].copy()
    flip = rng.random(len(perm)) < 0.1
    node_of_f[flip] = rng.integers(0, n_nodes, flip.sum())

    def csr(node):
        ids = np.unique(node)
        idx = np.concatenate([np.nonzero(node == i)[0] for i in ids])
        off = np.concatenate([[0], np.cumsum([np.sum(node == i) for i in ids])])
        return ids.astype(np.int32), off.astype(np.int32), idx.astype(np.int32)

    kf_fv, f_fv = csr(node_of_kf), csr(node_of_f)
    m = orb.ORBmatcher(ratio, ori)
    n_got, got = m.SearchByBoW_KF_F(d0, k0["angle"], kf_valid, kf_fv, f_desc, f_angle, f_fv)
    n_want, want = ol.search_by_bow_kf_f(d0, k0["angle"], kf_valid, kf_fv, f_desc, f_angle, f_fv, ratio, ori)
    assert n_got == n_want and np.array_equal(got, want)
    assert n_want > 50


@pytest.mark.parametrize("seed,n_nodes", [(0, 40), (1, 5), (2, 200)])
def test_search_by_bow_kf_kf(frames, seed, n_nodes):
    (k0, d0), (k1, d1) = frames
    rng = np.random.default_rng(100 + seed)
    perm = rng.permutation(len(d0))
    d2 = near_duplicates(d0[perm], rng, 5)
    a2 = k0["angle"][perm]
    v1 = (rng.random(len(d0)) > 0.15).astype(np.uint8)
    v2 = (rng.random(len(d2)) > 0.15).astype(np.uint8)
    fv1 = make_fv(len(d0), n_nodes, rng, drop=0.05)
    node2 = rng.integers(0, n_nodes, len(d2))
    fv2 = make_fv(len(d2), n_nodes, rng)
    m = orb.ORBmatcher(0.8, True)
    n_got, got = m.SearchByBoW_KF_KF(d0, k0["angle"], v1, fv1, d2, a2, v2, fv2)
    n_want, want = ol.search_by_bow_kf_kf(d0, k0["angle"], v1, fv1, d2, a2, v2, fv2, 0.8, True)
    assert n_got == n_want and np.array_equal(got, want)


def window_candidates(kps_q, kps_t, radius, rng, level_window=True):
    """Candidate lists exactly as the C++ adaptor would build them: Frame::GetFeaturesInArea on the grid."""
    grid = ol.OracleGrid(kps_t, 0.0, 0.0, 640.0, 480.0)
    off, idx = [0], []
    for kp in kps_q:
        lo, hi = (int(kp["octave"]) - 1, int(kp["octave"]) + 1) if level_window else (-1, -1)
        c = grid.query(kp["x"] + 3.0, kp["y"] + 2.0, radius * (1.2 ** int(kp["octave"])), lo, hi)
        idx += c.tolist()
        off.append(len(idx))
    return np.array(off, np.int32), np.array(idx, np.int32)


@pytest.mark.parametrize("seed,ori,th", [(0, True, 100), (1, False, 100), (2, True, 60)])
def test_search_by_projection_last(frames, seed, ori, th):
    (k0, d0), (k1, d1) = frames
    rng = np.random.default_rng(seed)
    nq = 700
    q = rng.choice(len(d0), nq, replace=False)
    q.sort()
    cand_off, cand_idx = window_candidates(k0[q], k1, 15.0, rng)
    q_blocks = (rng.random(nq) > 0.3).astype(np.uint8)       # some temporal points with 0 observations
    t_blocked = (rng.random(len(d1)) < 0.05).astype(np.uint8)
    m = orb.ORBmatcher(0.9, ori)
    n_got, tm_got, tb_got = m.SearchByProjection_Last(d0[q], k0["angle"][q], q_blocks, cand_off, cand_idx, d1,
                                                      k1["angle"], t_blocked, th)
    n_want, tm_want, tb_want = ol.search_by_projection_last(d0[q], k0["angle"][q], q_blocks, cand_off, cand_idx, d1,
                                                            k1["angle"], t_blocked, th, ori)
    assert n_got == n_want and np.array_equal(tm_got, tm_want) and np.array_equal(tb_got, tb_want)
    assert n_want > 100


@pytest.mark.parametrize("seed,ratio", [(0, 0.8), (1, 0.6)])
def test_search_by_projection_local(frames, seed, ratio):
    (k0, d0), (k1, d1) = frames
    rng = np.random.default_rng(10 + seed)
    q = np.sort(rng.choice(len(d0), 800, replace=False))
    cand_off, cand_idx = window_candidates(k0[q], k1, 12.0, rng)
    q_blocks = (rng.random(len(q)) > 0.2).astype(np.uint8)
    t_blocked = (rng.random(len(d1)) < 0.1).astype(np.uint8)
    m = orb.ORBmatcher(ratio, True)
    n_got, tm_got, tb_got = m.SearchByProjection_Local(d0[q], q_blocks, cand_off, cand_idx, d1, k1["octave"], t_blocked)
    n_want, tm_want, tb_want = ol.search_by_projection_local(d0[q], q_blocks, cand_off, cand_idx, d1, k1["octave"],
                                                             t_blocked, ratio)
    assert n_got == n_want and np.array_equal(tm_got, tm_want) and np.array_equal(tb_got, tb_want)
    assert n_want > 100


@pytest.mark.parametrize("seed,ori", [(0, True), (1, False)])
def test_search_for_initialization(frames, seed, ori):
    (k0, d0), (k1, d1) = frames
    rng = np.random.default_rng(20 + seed)
    grid = ol.OracleGrid(k1, 0.0, 0.0, 640.0, 480.0)
    off, idx = [0], []
    for kp in k0:
        if kp["octave"] == 0:
            idx += grid.query(kp["x"] + 3.0, kp["y"] + 2.0, 30.0, 0, 0).tolist()  # windowSize, level1, level1
        off.append(len(idx))
    m = orb.ORBmatcher(0.9, ori)
    n_got, got = m.SearchForInitialization(d0, k0["angle"], k0["octave"], off, idx, d1, k1["angle"])
    n_want, want = ol.search_for_initialization(d0, k0["angle"], k0["octave"], off, idx, d1, k1["angle"], 0.9, ori)
    assert n_got == n_want and np.array_equal(got, want)
    assert n_want > 30


def test_matchers_on_empty_inputs():
    m = orb.ORBmatcher(0.7, True)
    e32 = np.zeros((0, 32), np.uint8)
    fv0 = (np.zeros(0, np.int32), np.zeros(1, np.int32), np.zeros(0, np.int32))
    assert m.SearchByBoW_KF_F(e32, [], [], fv0, e32, [], fv0)[0] == 0
    n, tm, tb = m.SearchByProjection_Last(e32, [], [], [0], [], np.zeros((5, 32), np.uint8), np.zeros(5), np.zeros(5))
    assert n == 0 and tm.tolist() == [-1] * 5


# ----------------------------------------------------------------------------- the Frame grid on the device
def _camera_view(name, keys, w=640, h=480):
    """(mvKeysUn, bounds) of `keys` seen through camera `name`: "image" = no distortion, "tum1" / "d435i" = the BASELINE
    cameras whose Frame constructor undistorts (Frame.cc:891-955; C1 and C5)."""
    if name == "image":
        return keys, (0.0, 0.0, float(w), float(h))
    cam = ol.scaled_camera(name, w, h)
    return ol.undistort_keypoints(keys, cam), ol.image_bounds(cam)


@pytest.mark.parametrize("camera", ["image", "tum1", "d435i"])
@pytest.mark.parametrize("seed", [0, 1])
def test_device_grid_query_equals_reference_order(frames, seed, camera):
    (k0, d0), (k1, d1) = frames
    rng = np.random.default_rng(seed)
    k1, bounds = _camera_view(camera, k1)
    g_ref = ol.OracleGrid(k1, *bounds)
    g = orb.FrameGrid(k1, *bounds)
    nq = 400
    x = rng.uniform(-20, 660, nq).astype(np.float32)
    y = rng.uniform(-20, 500, nq).astype(np.float32)
    r = rng.uniform(1, 60, nq).astype(np.float32)
    lo = rng.integers(-1, 5, nq).astype(np.int32)
    hi = rng.integers(-1, 8, nq).astype(np.int32)
    off, idx = g.GetFeaturesInArea(x, y, r, lo, hi)
    for q in range(nq):
        want = g_ref.query(x[q], y[q], r[q], int(lo[q]), int(hi[q]))
        assert np.array_equal(idx[off[q]:off[q + 1]], want), q  # same elements in the same ORDER
    off2, idx2 = g.GetFeaturesInArea(x, y, r)  # KeyFrame::GetFeaturesInArea: no level filter
    for q in range(0, nq, 7):
        assert np.array_equal(idx2[off2[q]:off2[q + 1]], g_ref.query(x[q], y[q], r[q], -1, -1))
    assert off[-1] > 1000


@pytest.mark.parametrize("camera", ["image", "tum1", "d435i"])
def test_device_grid_edge_cases(camera):
    e32 = np.zeros(0, orb.KP_DTYPE)
    _, bounds = _camera_view(camera, e32)
    g = orb.FrameGrid(e32, *bounds)
    off, idx = g.GetFeaturesInArea([10.0, 700.0], [10.0, 10.0], [5.0, 5.0])
    assert off.tolist() == [0, 0, 0] and len(idx) == 0
    kp = np.zeros(3, orb.KP_DTYPE)
    kp["x"], kp["y"], kp["octave"] = [5.0, 5.0, 639.9], [5.0, 5.0, 479.9], [0, 3, 1]
    kp, bounds = _camera_view(camera, kp)  # TUM1: (5, 5) undistorts to outside the grid -- PosInGrid drops it
    g = orb.FrameGrid(kp, *bounds)
    ref = ol.OracleGrid(kp, *bounds)
    for q in [(5.0, 5.0, 1.0, -1, -1), (5.0, 5.0, 1.0, 2, 4), (639.0, 479.0, 3.0, -1, -1), (-50.0, 5.0, 10.0, -1, -1),
              (12.0, 15.0, 9.0, -1, -1), (bounds[0], bounds[1], 0.5, -1, -1), (bounds[2], bounds[3], 2.0, -1, -1)]:
        off, idx = g.GetFeaturesInArea([q[0]], [q[1]], [q[2]], [q[3]], [q[4]])
        assert idx.tolist() == ref.query(*q).tolist()


def test_device_grid_octaves_above_15():
    """A grid compares the whole octave (a resident frame's packed candidates carry 4 bits of it; a grid's do not)."""
    rng = np.random.default_rng(7)
    octaves = [0, 7, 16, 20, 300]
    kp = np.zeros(800, orb.KP_DTYPE)
    kp["x"], kp["y"] = rng.uniform(0, 640, len(kp)), rng.uniform(0, 480, len(kp))
    kp["octave"] = rng.choice(octaves, len(kp))
    bounds = (0.0, 0.0, 640.0, 480.0)
    g, ref = orb.FrameGrid(kp, *bounds), ol.OracleGrid(kp, *bounds)
    x, y = rng.uniform(0, 640, 40).astype(np.float32), rng.uniform(0, 480, 40).astype(np.float32)
    r = np.full(40, 50.0, np.float32)
    # (minLevel, maxLevel) -> the octaves GetFeaturesInArea lets through (Frame.cc:836-843)
    for (lo, hi), passing in {(-1, -1): octaves, (0, 0): [0], (-1, 15): [0, 7], (1, 7): [7], (8, 16): [16],
                              (16, -1): [16, 20, 300], (17, 20): [20], (17, 299): [20], (21, 299): [],
                              (21, 300): [300], (300, -1): [300], (301, -1): []}.items():
        off, idx = g.GetFeaturesInArea(x, y, r, np.full(40, lo, np.int32), np.full(40, hi, np.int32))
        for q in range(40):
            assert np.array_equal(idx[off[q]:off[q + 1]], ref.query(x[q], y[q], r[q], lo, hi)), (lo, hi, q)
        assert sorted(set(kp["octave"][idx].tolist())) == passing, (lo, hi)


def _grid_query_raw(g, x, y, r, idx, cap):
    """vsg_grid_query as the C caller sees it: (return value, cand_off); idx (None = NULL) is written in place."""
    off = np.full(len(x) + 1, -1, np.int32)
    rc = orb._lib.vsg_grid_query(g._h, orb._p(x, orb._f32p), orb._p(y, orb._f32p), orb._p(r, orb._f32p), None, None,
                                 len(x), orb._p(off, orb._i32p), orb._p(idx, orb._i32p) if idx is not None else None, cap)
    return rc, off


def test_device_grid_query_cap_below_total_and_count_only(frames):
    (k0, d0), (k1, d1) = frames
    bounds = (0.0, 0.0, 640.0, 480.0)
    g, ref = orb.FrameGrid(k1, *bounds), ol.OracleGrid(k1, *bounds)
    x, y = (k0["x"][:60] + 3).astype(np.float32), (k0["y"][:60] + 2).astype(np.float32)
    r = np.full(60, 30.0, np.float32)
    want = [ref.query(x[q], y[q], r[q]) for q in range(60)]
    want_off = np.concatenate([[0], np.cumsum([len(w) for w in want])]).astype(np.int32)
    want_idx = np.concatenate(want)
    total = int(want_off[-1])
    assert total > 200
    GUARD = -7
    for cap in (total // 2, 1, total - 1, total):
        idx = np.full(total + 8, GUARD, np.int32)
        rc, off = _grid_query_raw(g, x, y, r, idx, cap)
        assert rc == total, cap  # the return value is the total even when it exceeds cap
        assert np.array_equal(off, want_off), cap  # cand_off is complete
        assert np.array_equal(idx[:cap], want_idx[:cap]), cap
        assert (idx[cap:] == GUARD).all(), cap  # nothing is written behind cap
    # count-only calls: cand_idx == NULL (whatever cap says), or cap == 0
    for idx, cap in ((None, 0), (None, total), (np.full(total, GUARD, np.int32), 0)):
        rc, off = _grid_query_raw(g, x, y, r, idx, cap)
        assert rc == total and np.array_equal(off, want_off)
        assert idx is None or (idx == GUARD).all()
    rc, off = _grid_query_raw(g, x[:0], y[:0], r[:0], None, 0)  # nq == 0
    assert rc == 0 and off[0] == 0


def test_device_grid_built_on_one_thread_queried_from_another(frames):
    import threading
    (k0, d0), (k1, d1) = frames
    bounds = (0.0, 0.0, 640.0, 480.0)
    ref = ol.OracleGrid(k1, *bounds)
    x, y = (k0["x"] + 3).astype(np.float32), (k0["y"] + 2).astype(np.float32)
    # r = 5 lists fit the kernel's 16 inline slots per query; r = 60 lists go to its overflow segment
    want = {rad: [ref.query(x[q], y[q], rad) for q in range(len(x))] for rad in (5.0, 60.0)}
    assert max(len(w) for w in want[5.0]) <= 16 and sum(len(w) for w in want[5.0]) > 100
    assert sum(len(w) > 16 for w in want[60.0]) > len(x) // 2
    box = {}

    def run(name, fn):
        def body():
            try:
                box[name] = fn()
            except BaseException as e:  # noqa: BLE001 -- re-raised on the test's thread below
                box[name] = e
        t = threading.Thread(target=body)
        t.start()
        t.join()
        if isinstance(box[name], BaseException):
            raise box[name]
        return box[name]

    g = run("build", lambda: orb.FrameGrid(k1, *bounds))
    for rad in (5.0, 60.0):
        off, idx = run("query", lambda: g.GetFeaturesInArea(x, y, np.full(len(x), rad, np.float32)))
        for q in range(len(x)):
            assert np.array_equal(idx[off[q]:off[q + 1]], want[rad][q]), (rad, q)
    off, idx = g.GetFeaturesInArea(x, y, np.full(len(x), 60.0, np.float32))  # and from a third (this) thread
    assert np.array_equal(idx, np.concatenate(want[60.0]))


def test_device_grid_rejects_octave_outside_int16():
    kp = np.zeros(3, orb.KP_DTYPE)
    kp["x"], kp["y"], kp["octave"] = [5.0, 50.0, 100.0], [5.0, 50.0, 100.0], [0, 40000, 1]
    with pytest.raises(orb.VsgError) as e:
        orb.FrameGrid(kp, 0.0, 0.0, 640.0, 480.0)
    assert e.value.code == -3  # VSG_ERR_UNSUPPORTED
    kp["octave"] = [-32768, 32767, 1]  # the int16 range itself is exact
    g, ref = orb.FrameGrid(kp, 0.0, 0.0, 640.0, 480.0), ol.OracleGrid(kp, 0.0, 0.0, 640.0, 480.0)
    for lo, hi in ((-1, -1), (2, -1), (-1, 40), (32767, 32767)):
        off, idx = g.GetFeaturesInArea([50.0], [50.0], [60.0], [lo], [hi])
        assert idx.tolist() == ref.query(50.0, 50.0, 60.0, lo, hi).tolist(), (lo, hi)


@pytest.mark.parametrize("seed,blocking", [(0, True), (1, False), (2, None)])
def test_search_window_generic(frames, seed, blocking):
    """Common core of the Sim3 / relocalisation projection searches, SearchBySim3 and Fuse (per-query best)."""
    (k0, d0), (k1, d1) = frames
    rng = np.random.default_rng(40 + seed)
    q = np.sort(rng.choice(len(d0), 600, replace=False))
    grid = orb.FrameGrid(k1, 0.0, 0.0, 640.0, 480.0)
    cand_off, cand_idx = grid.GetFeaturesInArea(k0["x"][q] + 3.0, k0["y"][q] + 2.0, np.full(len(q), 14.0, np.float32))
    if blocking is None:
        q_blocks, t_blocked = None, None
    else:
        q_blocks = np.full(len(q), 1 if blocking else 0, np.uint8)
        t_blocked = (rng.random(len(d1)) < 0.1).astype(np.uint8)
    th = 50 if seed else 100
    got = orb.search_window(d0[q], q_blocks, cand_off, cand_idx, d1, t_blocked, th)
    want = ol.search_window(d0[q], q_blocks, cand_off, cand_idx, d1, t_blocked, th)
    assert got[0] == want[0] > 50
    for a, b in zip(got[1:4], want[1:4]):
        assert np.array_equal(a, b)
    if blocking is not None:
        assert np.array_equal(got[4], want[4])


def test_distinctive_descriptors(frames):
    """MapPoint::ComputeDistinctiveDescriptors (N^2 Hamming + per-row median), many map points."""
    (k0, d0), (k1, d1) = frames
    rng = np.random.default_rng(77)
    sizes = [1, 2, 3, 4, 7, 0, 16, 33, 64, 100, 128, 5, 5, 2]
    groups, off = [], [0]
    for n in sizes:
        base = d0[rng.integers(0, len(d0))]
        g = near_duplicates(np.repeat(base[None], n, 0), rng, 4) if n else np.zeros((0, 32), np.uint8)
        if n >= 4:
            g[1] = g[0]  # exact duplicates: equal medians -> the first row must win
        groups.append(g)
        off.append(off[-1] + n)
    desc = np.concatenate(groups)
    got = orb.ComputeDistinctiveDescriptors(desc, off)
    want = ol.distinctive_descriptors(desc, off)
    assert np.array_equal(got, want)
    assert want[5] == -1


def shared_pair_bits(fv1, fv2, rng, p_ok):
    """Random geometric-predicate bits for every pair of every SHARED node, in the layout of
    vsg_search_for_triangulation: pair_off[s] + i1 * n2(s) + i2."""
    ids1, off1, _ = fv1
    ids2, off2, _ = fv2
    shared = np.intersect1d(ids1, ids2)
    pair_off = [0]
    for s in shared:
        a, b = int(np.searchsorted(ids1, s)), int(np.searchsorted(ids2, s))
        pair_off.append(pair_off[-1] + int(off1[a + 1] - off1[a]) * int(off2[b + 1] - off2[b]))
    nbits = pair_off[-1]
    bits = rng.random(max(nbits, 1)) < p_ok
    words = np.zeros((nbits + 31) // 32 + 1, np.uint32)
    for i in np.nonzero(bits[:nbits])[0]:
        words[i >> 5] |= np.uint32(1 << (i & 31))
    return words, np.array(pair_off, np.int32)


@pytest.mark.parametrize("seed,n_nodes,p_ok,ori", [(0, 40, 0.7, True), (1, 5, 0.3, True), (2, 200, 1.0, False),
                                                   (3, 60, None, True)])
def test_search_for_triangulation(frames, seed, n_nodes, p_ok, ori):
    """ORBmatcher::SearchForTriangulation (ORBmatcher.cc:902-1146): predicate bits from the adaptor, dist <= TH_LOW,
    LAST minimum wins -- the duplicated descriptors make equal distances common."""
    (k0, d0), _ = frames
    rng = np.random.default_rng(300 + seed)
    perm = rng.permutation(len(d0))
    d2 = near_duplicates(d0[perm], rng, 4)
    d2[::3] = d2[1::3][:len(d2[::3])]  # exact duplicates inside KF2: ties on the distance
    a2 = k0["angle"][perm]
    e1 = (rng.random(len(d0)) > 0.2).astype(np.uint8)
    e2 = (rng.random(len(d2)) > 0.2).astype(np.uint8)
    # a feature and its near-duplicate land in the same vocabulary node (as similar descriptors do)
    node1 = rng.integers(0, n_nodes, len(d0)) * 7 + 3

    def fv_of(node):
        ids = np.unique(node)
        off_, idx_ = [0], []
        for i in ids:
            idx_ += np.nonzero(node == i)[0].tolist()
            off_.append(len(idx_))
        return ids.astype(np.int32), np.array(off_, np.int32), np.array(idx_, np.int32)
    fv1, fv2 = fv_of(node1), fv_of(node1[perm])
    ok, off = shared_pair_bits(fv1, fv2, rng, p_ok) if p_ok is not None else (None, None)
    m = orb.ORBmatcher(0.6, ori)
    n_got, got = m.SearchForTriangulation(d0, k0["angle"], e1, fv1, d2, a2, e2, fv2, ok, off)
    n_want, want = ol.search_for_triangulation(d0, k0["angle"], e1, fv1, d2, a2, e2, fv2, ok, off, ori)
    assert n_got == n_want and np.array_equal(got, want)
    assert n_want > 20
    # matches only between eligible features of the same node, inside TH_LOW, with the predicate bit set
    for i1 in np.nonzero(want >= 0)[0][:50]:
        assert e1[i1] and e2[want[i1]] and ol.descriptor_distance(d0[i1], d2[want[i1]]) <= 50


def test_block_best2_tile_boundaries_of_the_mfma_kernel():
    """The matrix-core matcher works on 32-row train tiles, 32-query column blocks, 256-query workgroups and an
    8-tile prefetch group: sizes on and around every one of those boundaries, tie-heavy data."""
    rng = np.random.default_rng(5)
    m = orb.ORBmatcher()
    sizes = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 287, 288, 289, 511, 513]
    base = rng.integers(0, 256, (9, 32), dtype=np.uint8)
    for na in sizes:
        for nb in (sizes if na in (1, 33, 129, 257) else (1, 31, 33, 256, 289)):
            a = near_duplicates(base[rng.integers(0, 9, na)], rng, 2)
            b = near_duplicates(base[rng.integers(0, 9, nb)], rng, 1)
            for g, w in zip(m.block_best2(a, b), ol.block_best2(a, b)):
                assert np.array_equal(g, w), (na, nb)
    # all-equal descriptors: distance 0 everywhere, the first train row must win and the second-best is 0 too
    z = np.zeros((70, 32), np.uint8)
    best, second, arg = m.block_best2(z, z)
    assert not best.any() and not second.any() and not arg.any()
    # complementary descriptors: distance 256 (the accumulator's extreme value) is never "better than 256": like
    # the reference's strict '<' scan from bestDist = 256, no best index
    comp = np.full((40, 32), 255, np.uint8)
    for g, w in zip(m.block_best2(z[:5], comp), ol.block_best2(z[:5], comp)):
        assert np.array_equal(g, w)
    assert m.block_best2(z[:5], comp)[2].tolist() == [-1] * 5
    off = np.array([0, 40], np.int32)
    n, qi, qd, tm, _ = orb.search_window(z[:1], None, off, np.arange(40, dtype=np.int32), comp, None, 256)
    assert (n, qi.tolist(), qd.tolist()) == (0, [-1], [256])
    assert ol.search_window(z[:1], None, off, np.arange(40, dtype=np.int32), comp, None, 256)[:3][0] == 0


@pytest.mark.parametrize("seed,n_nodes,ratio,ori", [(0, 60, 0.7, True), (1, 8, 0.9, True), (2, 1, 0.6, False)])
def test_search_by_bow_kf_f_fisheye_stereo(frames, seed, n_nodes, ratio, ori):
    """SearchByBoW(KeyFrame*, Frame&) with F.Nleft != -1 (ORBmatcher.cc:277-326, 362-389): the frame holds the left
    camera's features followed by the right camera's; a KF feature can claim one of each, the right one without a
    ratio test but only if the left best is within TH_LOW."""
    (k0, d0), _ = frames
    rng = np.random.default_rng(400 + seed)
    n = len(d0)
    permL, permR = rng.permutation(n), rng.permutation(n)
    keepR = rng.random(n) < 0.7
    f_desc = np.concatenate([near_duplicates(d0[permL], rng, 6), near_duplicates(d0[permR][keepR], rng, 9)])
    f_angle = np.concatenate([k0["angle"][permL], k0["angle"][permR][keepR]]).astype(np.float32)
    nleft = n
    kf_valid = (rng.random(n) > 0.2).astype(np.uint8)
    node_of_kf = rng.integers(0, n_nodes, n)
    node_of_f = np.concatenate([node_of_kf[permL], node_of_kf[permR][keepR]])

    def csr(node):
        ids = np.unique(node)
        idx = np.concatenate([np.nonzero(node == i)[0] for i in ids])
        off = np.concatenate([[0], np.cumsum([np.sum(node == i) for i in ids])])
        return ids.astype(np.int32), off.astype(np.int32), idx.astype(np.int32)

    kf_fv, f_fv = csr(node_of_kf), csr(node_of_f)
    m = orb.ORBmatcher(ratio, ori)
    n_got, got = m.SearchByBoW_KF_F(d0, k0["angle"], kf_valid, kf_fv, f_desc, f_angle, f_fv, f_nleft=nleft)
    n_want, want = ol.search_by_bow_kf_f(d0, k0["angle"], kf_valid, kf_fv, f_desc, f_angle, f_fv, ratio, ori, nleft)
    assert n_got == n_want and np.array_equal(got, want)
    assert (want[:nleft] >= 0).sum() > 50 and (want[nleft:] >= 0).sum() > 50  # both cameras really matched
    # with Nleft = -1 the same arrays are one block: different result, and it equals the mono entry point
    n_m, got_m = m.SearchByBoW_KF_F(d0, k0["angle"], kf_valid, kf_fv, f_desc, f_angle, f_fv)
    n_w, want_m = ol.search_by_bow_kf_f(d0, k0["angle"], kf_valid, kf_fv, f_desc, f_angle, f_fv, ratio, ori)
    assert n_m == n_w and np.array_equal(got_m, want_m) and not np.array_equal(want_m, want)


# ---- the vocabulary-node searches on FeatureVectors given as host arrays: what they refuse, and the caller-bits walk of
# SearchForTriangulation at its tile edges
NODE_FORMS = ["frame_kf_f", "frame_kf_kf", "frame_triangulation", "host_kf_f", "host_kf_kf", "host_triangulation"]


@pytest.fixture(scope="module")
def node_scene():
    """Two uploaded frames of about 300 features (the parity scene of tests/epipolar_scenes.py) with FeatureVectors of 8
    nodes: a KF1 feature lies in the node of its true correspondence, so every search finds matches."""
    import epipolar_scenes as es
    s = dict(es.frames())
    rng = np.random.default_rng(77)
    n1, n2 = len(s["k1"]), len(s["k2"])
    node2 = rng.integers(0, 8, n2)
    node1 = np.where(s["match"] >= 0, node2[np.maximum(s["match"], 0)], rng.integers(0, 8, n1))
    fv = lambda node: es._fv({int(i) * 5 + 2: np.flatnonzero(node == i).astype(np.int32) for i in range(8)})
    s["fv1"], s["fv2"] = fv(node1), fv(node2)
    assert len(s["fv1"][0]) == len(s["fv2"][0]) == 8 and 200 <= n1 <= 400 and 200 <= n2 <= 400
    s["F1"] = orb.Frame(n1 + 1).upload(s["k1"], s["d1"], es.BOUNDS)
    s["F2"] = orb.Frame(n2 + 1).upload(s["k2"], s["d2"], es.BOUNDS)
    s["v1"], s["v2"] = (rng.random(n1) > 0.2).astype(np.uint8), (rng.random(n2) > 0.2).astype(np.uint8)
    s["bits"] = shared_pair_bits(s["fv1"], s["fv2"], rng, 0.7)
    return s


def _node_search(form, s, fv1, fv2, pair_off=None):
    """The raw call of one form: (return code, output array pre-filled with 12345).  An entry of fv1 / fv2 may be None."""
    L = orb.load_library()
    p = lambda a, t: None if a is None else a.ctypes.data_as(t)
    n1, n2 = len(s["k1"]), len(s["k2"])
    a1, a2 = np.ascontiguousarray(s["k1"]["angle"]), np.ascontiguousarray(s["k2"]["angle"])
    u8, f32, i32 = orb._u8p, orb._f32p, orb._i32p
    fa, fb = [p(x, i32) for x in fv1] + [8], [p(x, i32) for x in fv2] + [8]
    ok, off = s["bits"][0], s["bits"][1] if pair_off is None else pair_off
    out = np.full(n2 if form.endswith("kf_f") else n1, 12345, np.int32)
    tail = [0.7, 1, p(out, i32)]
    tri = [ok.ctypes.data, off.ctypes.data, 1, p(out, i32)]
    h1, h2 = [p(s["d1"], u8), p(a1, f32), p(s["v1"], u8), n1], [p(s["d2"], u8), p(a2, f32), p(s["v2"], u8), n2]
    if form == "frame_kf_f":
        rc = L.vsg_frame_search_by_bow_kf_f(s["F1"].handle, p(s["v1"], u8), *fa, s["F2"].handle, *fb, *tail)
    elif form == "frame_kf_kf":
        rc = L.vsg_frame_search_by_bow_kf_kf(s["F1"].handle, p(s["v1"], u8), *fa, s["F2"].handle, p(s["v2"], u8), *fb, *tail)
    elif form == "frame_triangulation":
        rc = L.vsg_frame_search_for_triangulation(s["F1"].handle, p(s["v1"], u8), *fa, s["F2"].handle, p(s["v2"], u8), *fb, *tri)
    elif form == "host_kf_f":
        rc = L.vsg_search_by_bow_kf_f_stereo(0, *h1, *fa, p(s["d2"], u8), p(a2, f32), n2, -1, *fb, *tail)
    elif form == "host_kf_kf":
        rc = L.vsg_search_by_bow_kf_kf(0, *h1, *fa, *h2, *fb, *tail)
    else:
        rc = L.vsg_search_for_triangulation(0, *h1, *fa, *h2, *fb, *tri)
    return rc, out


@pytest.mark.parametrize("form", NODE_FORMS)
def test_node_searches_refuse_bad_feature_vectors_and_bits_then_equal_the_oracle(node_scene, form):
    """idx outside [0, n), a descending offset, only some arrays NULL and (triangulation) a pair_off one bit short are
    VSG_ERR_INVALID with the output untouched: none of them reaches the device.  The same call with valid arguments equals the
    CPU oracle."""
    s = node_scene
    n1, n2 = len(s["k1"]), len(s["k2"])
    (ids1, off1, idx1), (ids2, off2, idx2) = s["fv1"], s["fv2"]
    bad = []
    for v in (n1, -1, 1 << 30):
        b = idx1.copy()
        b[len(b) // 2] = v
        bad.append(((ids1, off1, b), s["fv2"], None))
    b = idx2.copy()
    b[-1] = n2
    bad.append((s["fv1"], (ids2, off2, b), None))
    b = off1.copy()
    b[2] = b[3] + 1
    bad.append(((ids1, b, idx1), s["fv2"], None))
    bad += [((ids1, None, idx1), s["fv2"], None), (s["fv1"], (ids2, off2, None), None), ((None, off1, idx1), s["fv2"], None)]
    if form.endswith("triangulation"):
        short = s["bits"][1].copy()
        short[-1] -= 1
        bad.append((s["fv1"], s["fv2"], short))
    for fv1, fv2, pair_off in bad:
        rc, out = _node_search(form, s, fv1, fv2, pair_off)
        assert rc == -6 and (out == 12345).all()
    rc, out = _node_search(form, s, s["fv1"], s["fv2"])
    a1, a2 = s["k1"]["angle"], s["k2"]["angle"]
    if form.endswith("kf_f"):
        want = ol.search_by_bow_kf_f(s["d1"], a1, s["v1"], s["fv1"], s["d2"], a2, s["fv2"], 0.7, True)
    elif form.endswith("kf_kf"):
        want = ol.search_by_bow_kf_kf(s["d1"], a1, s["v1"], s["fv1"], s["d2"], a2, s["v2"], s["fv2"], 0.7, True)
    else:
        want = ol.search_for_triangulation(s["d1"], a1, s["v1"], s["fv1"], s["d2"], a2, s["v2"], s["fv2"], *s["bits"], True)
    assert rc == want[0] > 10 and np.array_equal(out, want[1])


@pytest.fixture(scope="module")
def edge_frames():
    import triangulation_edges as te
    s = te.scene()
    k1, k2 = te.keypoints(s["a1"], orb.KP_DTYPE), te.keypoints(s["a2"], orb.KP_DTYPE)
    bounds = (0.0, 0.0, 640.0, 480.0)
    return orb.Frame(len(k1)).upload(k1, s["d1"], bounds), orb.Frame(len(k2)).upload(k2, s["d2"], bounds)


@pytest.mark.parametrize("flags", ["all_one", "every_third_zero"])
@pytest.mark.parametrize("pattern", ["none", "ones", "zeros", "last_bit_of_every_node"])
def test_search_for_triangulation_caller_bits_at_the_tile_edges(edge_frames, pattern, flags):
    """Nodes of (1, 1) ... (257, 130) rows around the 128-row chunks and tiles of the walk, a tie across the tile edge, four
    bit patterns, two flag settings (tests/triangulation_edges.py; the oracle's side is checked in
    tests/test_triangulation_edges.py): host-descriptor and resident form equal the CPU oracle."""
    import triangulation_edges as te
    s = te.scene()
    ok, off = te.pair_bits(pattern)
    e1, e2 = s["flags"][flags]
    want = ol.search_for_triangulation(s["d1"], s["a1"], e1, s["fv1"], s["d2"], s["a2"], e2, s["fv2"], ok, off, True)
    te.check_counts(s, pattern, flags, *want)
    host = orb.ORBmatcher(0.6, True).SearchForTriangulation(s["d1"], s["a1"], e1, s["fv1"], s["d2"], s["a2"], e2, s["fv2"], ok, off)
    assert host[0] == want[0] and np.array_equal(host[1], want[1])
    f1, f2 = edge_frames
    res = f1.SearchForTriangulation(e1, s["fv1"], f2, e2, s["fv2"], True, ok, off)
    assert res[0] == want[0] and np.array_equal(res[1], want[1])
