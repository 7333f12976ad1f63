"""GPU tests of Tracking::SearchLocalPoints in one call (vsg_frame_search_local_points) against the EXISTING
vsg_frame_search_by_projection (oracle-checked by tests/test_gpu_frame.py) fed with tests/frustum_reference.py's fields and
the same descriptors: nmatches, train_match, train_blocked identical; n_to_match, in_view, proj_x / proj_y as the
reference.  Frames are real extracted ones (gray and RGB-D, so the mvuRight gate with proj_xr is live); the map points are
the frame's keypoints un-projected at random depths through the scenario's pose, with perturbed copies of their
descriptors, among scenario points that match nothing."""
import ctypes as C
import threading

import numpy as np
import pytest

import frustum_reference as fr
import projection_reference as pr
import rgbd_reference as rr
import scenarios as sc
from frame_edge_routines import S16, resident
from test_gpu_frame_edges import in_thread
from visual_sgraphs_amd import orb, synth

pytestmark = pytest.mark.gpu
W, H = 640, 480
NNRATIO = 0.8
FIELDS = ("world_pos", "normal", "min_dist", "max_dist", "desc", "observed")


@pytest.fixture(scope="module")
def ex():
    return orb.ORBextractor(1000, 1.2, 8, 20, 7)


def make_frame(ex, seed, rgbd):
    img = synth.sequence_frame(W, H, seed, 0)
    f = orb.Frame(ex.capacity(H, W))
    bounds = (0.0, 0.0, float(W), float(H))
    if rgbd:
        plane = rr.depth_plane(30 + seed, H, W, np.uint16)
        _, _, d, ur, _ = f.extract_into_rgbd(ex, img, plane, bounds, None, None, np.float32(0.001), fr.CAMERAS["tum1"][6])
        assert (ur > 0).sum() > 100
    else:
        _, _, d = f.extract_into(ex, img, bounds)
        ur = None
    assert len(f.kps) > 500
    return f, d, ur, bounds


def local_map(frame, desc, ur, seed, per_keypoint=1, n_other=1500, mirror=False):
    """(pose, fields): every keypoint un-projected `per_keypoint` times at a random depth through the pose, mfMaxDistance
    such that the predicted level is the keypoint's octave (or one above: the window takes [level - 1, level]), the
    descriptor a copy with a few bits flipped; plus n_other scenario points."""
    rng = np.random.default_rng(seed)
    pose, _, other = fr.scenario(seed, "tum1", n=n_other)
    k = np.tile(frame.kps, per_keypoint)
    src = np.tile(np.arange(len(frame.kps)), per_keypoint)
    n = len(k)
    R, t = pose["Rcw"].astype(np.float64), pose["tcw"].astype(np.float64)
    z = rng.uniform(1.0, 8.0, n)
    if ur is not None:
        # a depth consistent with the frame's mvuRight for most points, so that the stereo gate lets them through; the rest
        # keep a random depth (proj_xr off mvuRight: the gate rejects them where the frame has a depth)
        u_r = ur[src]
        ok = (u_r > 0) & (rng.random(n) < 0.8)
        z[ok] = pose["mbf"] / (k["x"][ok].astype(np.float64) - u_r[ok])
        z = np.where(np.isfinite(z) & (z > 0.1), z, 3.0)
    x = (k["x"].astype(np.float64) + rng.normal(0, 0.7, n) - pose["cx"]) / pose["fx"] * z
    y = (k["y"].astype(np.float64) + rng.normal(0, 0.7, n) - pose["cy"]) / pose["fy"] * z
    Pc = np.stack([x, y, z], 1)
    if mirror:
        Pc = -Pc
    Pw = ((Pc - t) @ R).astype(np.float32)  # R^T (Pc - t)
    PO = Pw.astype(np.float64) - pose["Ow"]
    dist = np.linalg.norm(PO, axis=1)
    Nn = PO / dist[:, None] + rng.normal(0, 0.03, (n, 3)) * (rng.random((n, 1)) < 0.5)  # half exactly towards the camera
    Nn = (Nn / np.linalg.norm(Nn, axis=1, keepdims=True)).astype(np.float32)
    lvl = k["octave"].astype(np.float64) + rng.integers(0, 2, n)
    mf_max = (dist * 1.2 ** (lvl - 0.5)).astype(np.float32)
    mf_min = (mf_max / np.float32(1.2) ** np.float32(7)).astype(np.float32)
    d = desc[src].copy()
    for i in range(n):  # up to 20 flipped bits
        bits = rng.integers(0, 256, rng.integers(0, 21))
        d[i, bits // 8] ^= (1 << (bits % 8)).astype(np.uint8)
    mine = dict(world_pos=Pw, normal=Nn, min_dist=mf_min, max_dist=mf_max, desc=d,
                observed=(rng.random(n) < 0.8).astype(np.uint8))
    fields = {key: np.concatenate([mine[key], other[key]]) for key in FIELDS}
    order = rng.permutation(len(fields["desc"]))
    return pose, {key: v[order] for key, v in fields.items()}


def existing_path(F, ref, f, th, sf, blocked, th_far=None):
    return F.SearchByProjection(fr.search_fields(ref, f["desc"], f["observed"], th_far), th, NNRATIO, sf, blocked)


def compare(F, mp, pose, f, bounds, th, sf, blocked, slots=None, skip=None, far=None, min_share=0.10, run=lambda call: call()):
    """run: how the call under test is made (the reference call always runs on the calling thread)"""
    ref = fr.is_in_frustum(pose, bounds, f["world_pos"], f["normal"], f["min_dist"], f["max_dist"], skip=skip)
    want = existing_path(F, ref, f, th, sf, blocked, far)
    n_in = int(ref["in_view"].sum())
    print(f"n={len(ref['in_view'])} in view {n_in} nmatches {want[0]} th {th} far {far}")
    if min_share is not None:
        assert want[0] >= min_share * n_in, (want[0], n_in)  # a real share matches (condition on the existing path)
    got = run(lambda: F.SearchLocalPoints(mp, orb.FramePose.make(**pose), th, NNRATIO, sf, blocked, n=len(ref["in_view"]),
                                          slots=slots, skip=skip, far_points=far is not None, th_far_points=far or 0.0))
    assert got[0] == want[0]
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert np.array_equal(got[3], ref["in_view"]) and got[6] == n_in
    for a, k in ((got[4], "proj_x"), (got[5], "proj_y")):
        assert a.view(np.uint32).tobytes() == ref[k].view(np.uint32).tobytes(), k
    return ref, got


def store_of(f, capacity=None, slots=None):
    n = len(f["desc"])
    mp = orb.MapPoints(capacity or n)
    mp.update(np.arange(n) if slots is None else slots, **{k: f[k] for k in FIELDS})
    return mp


@pytest.mark.parametrize("rgbd", [False, True], ids=["gray", "rgbd"])
@pytest.mark.parametrize("th", [1, 3, 15])
def test_equal_to_search_by_projection(ex, rgbd, th):
    F, desc, ur, bounds = make_frame(ex, 3, rgbd)
    pose, f = local_map(F, desc, ur, 11 + th)
    sf = ex.GetScaleFactors()
    blocked = np.zeros(len(F.kps), np.uint8)
    mp = store_of(f)
    ref, got = compare(F, mp, pose, f, bounds, th, sf, blocked)
    if rgbd:
        # the gate is live: without mvuRight the same points match differently
        G, _, _, _ = make_frame(ex, 3, False)
        other = G.SearchLocalPoints(mp, orb.FramePose.make(**pose), th, NNRATIO, sf, blocked)
        assert not np.array_equal(other[1], got[1])
    # train_blocked pre-set on a tenth of the features
    rng = np.random.default_rng(th)
    blocked2 = (rng.random(len(F.kps)) < 0.1).astype(np.uint8)
    compare(F, mp, pose, f, bounds, th, sf, blocked2)


@pytest.mark.parametrize("rgbd", [False, True], ids=["gray", "rgbd"])
def test_far_points_skip_and_slots(ex, rgbd):
    F, desc, ur, bounds = make_frame(ex, 4, rgbd)
    pose, f = local_map(F, desc, ur, 21)
    n = len(f["desc"])
    sf = ex.GetScaleFactors()
    blocked = np.zeros(len(F.kps), np.uint8)
    mp = store_of(f)
    ref, base = compare(F, mp, pose, f, bounds, 3, sf, blocked)
    iv = ref["in_view"] != 0
    # far points: a threshold that removes a quarter of the in-view points from the search, not from n_to_match
    far = float(np.quantile(ref["depth"][iv], 0.75))
    assert 0.2 < (ref["depth"][iv] > np.float32(far)).mean() < 0.3
    _, got = compare(F, mp, pose, f, bounds, 3, sf, blocked, far=far)
    gone = np.flatnonzero(iv & (ref["depth"] > np.float32(far)))
    assert not np.isin(got[1], gone).any() and got[6] == base[6] and got[0] < base[0]
    # skip on a fifth of the points: none of them is matched, n_to_match drops by the in-view ones among them
    rng = np.random.default_rng(8)
    skip = (rng.random(n) < 0.2).astype(np.uint8)
    _, got = compare(F, mp, pose, f, bounds, 3, sf, blocked, skip=skip)
    assert not np.isin(got[1], np.flatnonzero(skip)).any()
    assert got[6] == base[6] - int((iv & (skip != 0)).sum())
    # the same map through a permuted placement with gaps; train_match holds QUERY indices either way
    cap = 2 * n + 5
    slots = rng.permutation(cap)[:n].astype(np.int32)
    mp2 = store_of(f, cap, slots)
    _, got = compare(F, mp2, pose, f, bounds, 3, sf, blocked, slots=slots)
    assert np.array_equal(got[1], base[1])
    # a keyframe's worth of churn: descriptors and distances of a twentieth of the slots change
    ch = rng.choice(n, n // 20, replace=False)
    f2 = {k: v.copy() for k, v in f.items()}
    f2["desc"][ch] = rng.integers(0, 256, (len(ch), 32), dtype=np.uint8)
    f2["max_dist"][ch] *= np.float32(1.2)
    mp2.update(slots[ch], desc=f2["desc"][ch], max_dist=f2["max_dist"][ch])
    compare(F, mp2, pose, f2, bounds, 3, sf, blocked, slots=slots)
    # errors are found before anything is enqueued; the call right behind one is correct
    with pytest.raises(orb.VsgError) as e:
        F.SearchLocalPoints(mp2, orb.FramePose.make(**pose), 3, NNRATIO, sf, blocked, slots=[0, cap])
    assert e.value.code == -6
    compare(F, mp2, pose, f2, bounds, 3, sf, blocked, slots=slots)


def test_more_than_2048_and_no_points_in_view(ex):
    F, desc, ur, bounds = make_frame(ex, 5, False)
    sf = ex.GetScaleFactors()
    blocked = np.zeros(len(F.kps), np.uint8)
    pose, f = local_map(F, desc, ur, 31, per_keypoint=4, n_other=500)
    ref, got = compare(F, store_of(f), pose, f, bounds, 1, sf, blocked)
    assert ref["in_view"].sum() > 2048
    # nothing in view: the reference does not search at all (nToMatch == 0, Tracking.cc:3468)
    pose, f = local_map(F, desc, ur, 32, n_other=0, mirror=True)
    ref, got = compare(F, store_of(f), pose, f, bounds, 1, sf, blocked, min_share=None)
    assert ref["in_view"].sum() == 0 and got[0] == 0 and got[6] == 0 and (got[1] == -1).all()
    # the call profile hook covers this entry point: its total is the last call's, not an earlier one's
    L, us = orb.load_library(), (C.c_float * 4)()
    assert L.vsg_debug_call_profile(us) == 0
    fill, launch, sync, total = list(us)
    assert total >= sync > 0 and total >= fill + launch + sync - 1.0 and total < 1e5, list(us)
    # n == 0
    got = F.SearchLocalPoints(store_of(f), orb.FramePose.make(**pose), 1, NNRATIO, sf, blocked, n=0)
    assert got[0] == 0 and got[6] == 0 and len(got[3]) == 0 and (got[1] == -1).all()


def test_two_threads_two_frames_one_store(ex):
    frames = [make_frame(ex, 6, False), make_frame(ex, 7, True)]
    sf = ex.GetScaleFactors()
    # one local map that holds both frames' points; each frame has its own pose
    maps = [local_map(F, d, ur, 41 + i, n_other=700) for i, (F, d, ur, _) in enumerate(frames)]
    f = {k: np.concatenate([m[1][k] for m in maps]) for k in FIELDS}
    mp = store_of(f)
    want = []
    for (F, _, _, bounds), (pose, _) in zip(frames, maps):
        want.append(compare(F, mp, pose, f, bounds, 3, sf, np.zeros(len(F.kps), np.uint8))[1])
    calls = 6
    got, errs = [[], []], []
    gate = threading.Barrier(2)

    def run(i):
        try:
            F, pose = frames[i][0], orb.FramePose.make(**maps[i][0])
            blocked = np.zeros(len(F.kps), np.uint8)
            F.SearchLocalPoints(mp, pose, 3, NNRATIO, sf, blocked)  # the thread's stream and arenas exist from here on
            for _ in range(calls):
                gate.wait(timeout=60)  # both threads enter the call together, every round
                got[i].append(F.SearchLocalPoints(mp, pose, 3, NNRATIO, sf, blocked))
            orb.load_library().vsg_thread_release()
        except Exception as e:  # noqa: BLE001
            gate.abort()
            errs.append(e)
    ts = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errs, errs
    for gs, w in zip(got, want):
        assert len(gs) == calls
        for g in gs:
            assert g[0] == w[0] and all(np.array_equal(a, b) for a, b in zip(g[1:6], w[1:6])) and g[6] == w[6]


def dense_windows_case(th_local, th_kf, n_points=65):
    """A frame packed as in test_dense_cells_left_grid (clustered cells of up to 200 entries; without mvuRight, so that
    every list is GetFeaturesInArea's own and the oracle can count it) and n_points map points above its cluster cells whose
    windows hold more than the kernel's 16 inline entries in BOTH searches.  Returns (frame dict, pose, fields, isInFrustum
    reference, KeyFrame-projection reference, overflow total of the local search, of the KeyFrame search)."""
    fd = dict(sc.dense_case(False)[0], u_right=None)
    o = sc.oracle_of(fd)
    cs, en = o.grid(False)
    occ = np.diff(cs)
    cof = sc.cell_of_features(cs, en, len(fd["keys"]))
    # the keypoints of the cluster cells whose own octave a predicted level of the 8-level pose can reach
    cand = np.flatnonzero((cof >= 0) & (occ[np.maximum(cof, 0)] >= 100) & (fd["keys"]["octave"] <= 6))
    pose, f = local_map(type("K", (), dict(kps=fd["keys"][cand]))(), fd["desc"][cand], None, 51, n_other=0)
    ref = fr.is_in_frustum(pose, fd["bounds"], f["world_pos"], f["normal"], f["min_dist"], f["max_dist"])
    kf = pr.project_kf_points(pose, fd["bounds"], f["world_pos"], f["min_dist"], f["max_dist"])
    keep, n_local, n_kf = [], [], []
    for i in np.flatnonzero((ref["in_view"] != 0) & (kf["valid"] != 0)):
        # ORBmatcher.cc:64-70 and :1928-1934 in float, as the product rounds them
        r = np.float32(2.5 if float(ref["view_cos"][i]) > 0.998 else 4.0) * np.float32(th_local)
        lvl, lk = int(ref["scale_level"][i]), int(kf["level"][i])
        a = len(o.features_in_area(ref["proj_x"][i], ref["proj_y"][i], np.float32(r * S16[lvl]), lvl - 1, lvl))
        b = len(o.features_in_area(kf["u"][i], kf["v"][i], np.float32(np.float32(th_kf) * S16[lk]), lk - 1, lk + 1))
        if a > 16 and b > 16:
            keep.append(i), n_local.append(a), n_kf.append(b)
        if len(keep) == n_points:
            break
    assert len(keep) == n_points
    keep = np.array(keep)
    f = {k: np.ascontiguousarray(v[keep]) for k, v in f.items()}
    ref = {k: v[keep] for k, v in ref.items()}
    kf = {k: v[keep] for k, v in kf.items()}
    return fd, pose, f, ref, kf, sum(n_local), sum(n_kf)


def test_overflow_retry_on_a_fresh_thread_through_the_resident_call():
    """SearchLocalPoints and SearchKeyFramePoints, each as the FIRST window search of a freshly started thread: the
    thread's candidate capacity is at its floor of 4 entries per query, 65 points (two workgroups of the projection kernel,
    the second with one live lane; 17 of the window kernel, the last with one live wave) whose lists all go to the overflow
    area need more than 4 x 65, so the first attempt ends in the retry and the whole chain -- projection kernel, window
    kernel, wait -- runs twice.  Results as the host-array SearchByProjection / SearchByProjection_KF on the same inputs."""
    th, th_kf, orb_dist = 15, 60, 100
    fd, pose, f, ref, kf, total_local, total_kf = dense_windows_case(th, th_kf)
    n = len(f["desc"])
    assert n == 65 and total_local > 4 * n and total_kf > 4 * n, (total_local, total_kf)   # every list is an overflow list
    F, _ = resident(fd)
    mp = store_of(f)
    blocked = np.zeros(len(fd["keys"]), np.uint8)
    ref2, _ = compare(F, mp, pose, f, fd["bounds"], th, S16, blocked, run=in_thread)
    assert all(np.array_equal(ref2[k], ref[k]) for k in ("in_view", "scale_level")) and ref["in_view"].all()
    # the KeyFrame form, as tests/test_gpu_search_keyframe_points.py compares it
    slots = np.arange(n, dtype=np.int32)
    kf_angle = np.random.default_rng(52).uniform(0, 360, n).astype(np.float32)
    a = pr.keyframe_fields(kf, slots, f["desc"], kf_angle, th_kf, S16)
    want = F.SearchByProjection_KF(a["desc"], a["u"], a["v"], a["radius"], a["predicted_level"], a["kf_angle"], orb_dist, True,
                                   blocked)
    want = (want[0], pr.map_back(want[1], a["index"]), want[2])
    print(f"kf n={n} overflow entries {total_kf} nmatches {want[0]}")
    assert want[0] >= 5   # the rotation histogram keeps matches under random observer angles (condition on the existing path)
    got = in_thread(lambda: F.SearchKeyFramePoints(mp, slots, orb.FramePose.make(**pose), th_kf, orb_dist, S16, blocked,
                                                   kf_angle, None, True))
    assert got[0] == want[0]
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert np.array_equal(got[3], kf["valid"])
    for x, k in ((got[4], "u"), (got[5], "v"), (got[6], "level")):
        assert x.dtype == kf[k].dtype and x.tobytes() == kf[k].tobytes(), k
