"""CPU tests of CreateNewMapPoints on resident keyframes: the restatement (tests/triangulation_reference.py) keeps the
reference's quirks, the scenes (tests/triangulation_scenes.py) are what they claim to be, and the host build of
visual_sgraphs_amd/csrc/vsg_triangulate.h (tests/_triangulatecore) equals the restatement -- bit for bit wherever no SVD is
involved, within the measured TOL where one is."""
import numpy as np
import pytest

import triangulation_hostcore as hc
import triangulation_reference as tr
import triangulation_scenes as ts

F32, F64, I32, U8 = np.float32, np.float64, np.int32, np.uint8


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ---------------------------------------------------------------------------------------------- the restatement's quirks
def _quirk(P, name):
    return dict(P, quirks=(name,))


def test_else_if_keeps_kf2s_stereo_parallax_out_when_kf1_is_stereo():
    """Both keypoints stereo, kf2's stereo parallax the larger one: the reference never looks at it (:568-571) and unprojects
    kf1's keypoint; a restatement that takes both unprojects kf2's."""
    s, _, _ = ts.directed()["stereo1"]
    j = int(s["matches"][0])
    f1 = ts.features_of(s, "1", [0])[0]
    f2 = dict(ts.features_of(s, "2", [j])[0], uright=F32(50.0), cos_stereo=F32(0.99), xyz_c=np.array([0.1, 0.1, 2.0], F32))
    assert tr.pair(s["P"], f1, f2)["source"] == tr.FROM_STEREO1
    assert tr.pair(_quirk(s["P"], "else_if"), f1, f2)["source"] == tr.FROM_STEREO2
    assert hc.pairs(s["P"], [f1], [f2])[1][0] == tr.FROM_STEREO1


def test_kf2s_right_coordinate_is_projected_with_the_current_keyframes_mbf():
    s, reason, _ = ts.directed()["stereo2"]
    assert reason == tr.ACCEPTED
    P = dict(s["P"], kf2=dict(s["P"]["kf2"], mbf=F32(3 * ts.MBF)))
    j = int(s["matches"][0])
    f1, f2 = ts.features_of(s, "1", [0])[0], ts.features_of(s, "2", [j])[0]
    assert tr.pair(P, f1, f2)["reason"] == tr.ACCEPTED and hc.pairs(P, [f1], [f2])[0][0] == tr.ACCEPTED
    assert tr.pair(_quirk(P, "own_mbf"), f1, f2)["reason"] == tr.REPROJ2


def test_parallax_limits_are_double_literals():
    """(float)0.9996 lies below 0.9996: a cosParallaxRays of exactly that float is below the double literal and not below the
    float one.  (0.9998 rounds up, so there the two comparisons agree on every float.)"""
    v = F32(0.9996)
    assert F64(v) < 0.9996 and F64(F32(0.9998)) > 0.9998
    assert tr.below_limit(v, True) and not tr.below_limit(v, True, ("float_literals",))
    for w in (np.nextafter(F32(0.9998), F32(0)), F32(0.9998), np.nextafter(F32(0.9998), F32(2))):
        assert tr.below_limit(w, False) == tr.below_limit(w, False, ("float_literals",))


def test_kf2_first_decides_the_descriptor_row():
    s = ts.parity(kf2_first=True)
    d1, d2 = s["d1"][0], s["d2"][s["matches"][0]]
    assert not np.array_equal(d1, d2)
    assert np.array_equal(tr.descriptor_row(s["P"], d1, d2), d2)
    assert np.array_equal(tr.descriptor_row(_quirk(s["P"], "kf1_first"), d1, d2), d1)
    assert np.array_equal(tr.descriptor_row(ts.parity()["P"], d1, d2), d1)


# ---------------------------------------------------------------------------------------------------------- the scenes
def test_directed_scenes_give_each_reason_and_source_off_its_threshold():
    tol, _ = ts.tolerance()
    seen_r, seen_s = set(), set()
    for name, (s, reason, source) in ts.directed().items():
        r = ts.restate(s, s["matches"])
        assert (r["reason"][0], r["source"][0]) == (reason, source), name
        assert not ts.near(s, r, tol).any(), name
        seen_r.add(reason), seen_s.add(source)
    assert seen_r == set(range(11)) and seen_s == {0, 1, 2}


def test_parity_scene_covers_the_branches_and_few_pairs_are_near_a_threshold():
    s = ts.parity()
    r = ts.restate(s, s["matches"])
    assert len(s["k1"]) == 324 and len(r["idx"]) == 300
    assert {tr.ACCEPTED, tr.LOW_PARALLAX, tr.Z1, tr.Z2, tr.REPROJ1, tr.REPROJ2, tr.FAR, tr.SCALE_RATIO} <= set(r["reason"].tolist())
    assert set(r["source"].tolist()) == {0, 1, 2}
    ok = r["reason"] == tr.ACCEPTED
    assert ok.sum() >= 150 and (ok & (r["source"] > 0)).sum() >= 10
    cpr = np.array([q["cos_parallax_rays"] for q in r["pairs"]])
    assert cpr.min() < 0.99 and (cpr > 0.99995).sum() >= 20  # from well above to below the parallax limits
    assert 0.25 < (s["ur1"] >= 0).mean() < 0.42 and 0.25 < (s["ur2"] >= 0).mean() < 0.42
    tol, _ = ts.tolerance()
    near = ts.near(s, r, tol)
    print("near pairs: %d of %d" % (near.sum(), len(near)))
    assert near.sum() <= 0.01 * len(near)


@pytest.mark.parametrize("n", [n for n in ts.EDGE_COUNTS if n])
def test_edge_scenes_accept_every_pair_far_from_the_thresholds(n):
    s = ts.edge(n)
    r = ts.restate(s, s["matches"])
    assert (r["reason"] == tr.ACCEPTED).all() and not ts.near(s, r, ts.tolerance()[0]).any()
    sets = ts.edge_sets(n)
    if n >= 65:
        assert {62, 63, 64} <= set(sets["boundaries"].tolist())
    if n > 1024:
        assert {510, 511, 512, 513, 1022, 1023, 1024, 1025} <= set(sets["chunk_boundaries"].tolist())


# --------------------------------------------------------------------------------------- the host build of the header
def _scenes():
    return list(ts.all_scenes())


def test_tolerance_is_measured_and_the_header_is_inside_it():
    tol, med = ts.tolerance()
    print("TOL = %.3g of |x3D| (median %.3g)" % (tol, med))
    assert 1e-8 < tol < 3e-7  # a float32 rounding of x3Dh and one float32 quotient per component
    worst, worst_double = 0.0, 0.0
    for name, s, m in _scenes():
        r, h = ts.restate(s, m), hc.loop(s, m)
        at = ts.triangulated(r)
        if not at:
            continue
        worst = max(worst, float(ts.deviation(r, h["x3d"]).max()))
        v = hc.null_vectors(np.stack([r["pairs"][p]["A"] for p in at]))
        exact = np.array([ts.exact_x3d(r["pairs"][p]["A"]) for p in at])
        worst_double = max(worst_double, float((np.linalg.norm(v[:, :3] / v[:, 3:] - exact, axis=1) / np.linalg.norm(exact, axis=1)).max()))
    print("header: %.3g of |x3D|; its double null vector before rounding: %.3g" % (worst, worst_double))
    assert worst <= tol            # no margin
    assert worst_double < 1e-3 * tol  # the double Jacobi is orders of magnitude inside what a float SVD can give


@pytest.mark.parametrize("which", ["parity", "parity_kf2_first", "directed", "edge"])
def test_host_build_equals_the_restatement(which):
    tol, _ = ts.tolerance()
    if which == "parity":
        scenes = [("parity", ts.parity(), ts.parity()["matches"])]
    elif which == "parity_kf2_first":
        scenes = [("parity_kf2_first", ts.parity(kf2_first=True), ts.parity(kf2_first=True)["matches"])]
    else:
        scenes = [x for x in _scenes() if x[0].startswith(which)]
    checked = 0
    for name, s, m in scenes:
        r, h = ts.restate(s, m), hc.loop(s, m)
        near = np.zeros(len(m), bool)
        near[r["idx"]] = ts.near(s, r, tol)
        assert which == "parity" or which == "parity_kf2_first" or not near.any()
        assert np.array_equal(h["reason"][~near], r["reason"][~near]), name
        assert np.array_equal(h["source"][~near], r["source"][~near]), name
        # rays and parallax: bit for bit
        if len(r["idx"]):
            par = hc.parallax(s["P"], r["f1"], r["f2"])
            want = np.array([[*q["ray1"], *q["ray2"], q["cos_parallax_rays"]] for q in r["pairs"]], F32)
            assert np.array_equal(bits(par), bits(want)), name
        # x3D: UnprojectStereo bit for bit, Triangulate within TOL
        st = np.flatnonzero(~near & (r["source"] > 0))
        assert np.array_equal(bits(h["x3d"][st]), bits(r["x3d"][st])), name
        tri = np.flatnonzero(~near & (r["source"] == 0) & (r["reason"] != tr.NO_MATCH))
        a, b = h["x3d"][tri].astype(F64), r["x3d"][tri].astype(F64)
        nz = np.linalg.norm(b, axis=1) > 0
        assert (np.linalg.norm(a - b, axis=1)[nz] <= tol * np.linalg.norm(b, axis=1)[nz]).all(), name
        assert (a[~nz] == 0).all()
        # the new point's normal and depth range: bit for bit given the same x3D
        for i in np.flatnonzero(h["reason"] == tr.ACCEPTED)[:40]:
            got = hc.normal_and_depth(s["P"], h["x3d"][i], s["k1"]["octave"][i], s["sf1"], s["nlevels"])
            want = tr.normal_and_depth(s["P"], h["x3d"][i], s["k1"]["octave"][i], s["sf1"], s["nlevels"])
            assert np.array_equal(bits(got[0]), bits(want[0])) and bits(got[1]) == bits(want[1]) and bits(got[2]) == bits(want[2])
            checked += 1
    assert checked > 0


def test_host_loop_assigns_free_slots_in_ascending_idx1_and_leaves_other_slots_alone():
    s = ts.parity(kf2_first=True)
    m, cap = s["matches"], 512
    rng = np.random.default_rng(3)
    store = dict(world_pos=rng.normal(size=(cap, 3)).astype(F32), normal=rng.normal(size=(cap, 3)).astype(F32),
                 min_dist=rng.random(cap).astype(F32), max_dist=rng.random(cap).astype(F32),
                 desc=rng.integers(0, 256, (cap, 32)).astype(U8), observed=np.full(cap, 7, U8))
    geometry = hc.loop(s, m)
    accepted = np.flatnonzero(geometry["reason"] == tr.ACCEPTED)
    for n_free in (0, len(accepted) - 1, len(accepted), len(accepted) + 5):
        free = rng.permutation(cap)[:n_free].astype(I32)
        h = hc.loop(s, m, store, free)
        k = min(n_free, len(accepted))
        assert h["n_created"] == k and np.array_equal(h["new_slot"][accepted[:k]], free[:k])
        assert (h["reason"][accepted[k:]] == tr.NO_FREE_SLOT).all() and (np.delete(h["new_slot"], accepted[:k]) == -1).all()
        assert np.array_equal(np.delete(h["reason"], accepted[k:]), np.delete(geometry["reason"], accepted[k:]))
        assert np.array_equal(bits(h["x3d"]), bits(geometry["x3d"]))
        after = h["store"]
        untouched = np.setdiff1d(np.arange(cap), free[:k])
        for key in store:
            assert np.array_equal(after[key][untouched], store[key][untouched]), key
        used = free[:k]
        assert np.array_equal(bits(after["world_pos"][used]), bits(h["x3d"][accepted[:k]])) and (after["observed"][used] == 1).all()
        assert np.array_equal(after["desc"][used], s["d2"][m[accepted[:k]]])  # kf2_first: pKF2's row
        for i, sl in list(zip(accepted[:k], used))[:25]:
            nrm, mn, mx = tr.normal_and_depth(s["P"], h["x3d"][i], s["k1"]["octave"][i], s["sf1"], s["nlevels"])
            assert np.array_equal(bits(after["normal"][sl]), bits(nrm))
            assert bits(after["min_dist"][sl]) == bits(mn) and bits(after["max_dist"][sl]) == bits(mx)
    h = hc.loop(ts.parity(), m, store, np.arange(cap, dtype=I32))
    assert np.array_equal(h["store"]["desc"][:len(accepted)], s["d1"][accepted])  # !kf2_first: the current keyframe's row


def test_hestenes_null_vector_on_random_two_view_matrices():
    """The scheme's own accuracy, away from the scenes: two-view matrices of baselines 0.003 .. 3 and depths 0.3 .. 30."""
    rng = np.random.default_rng(17)
    A = []
    for _ in range(600):
        c1, c2 = ts.cameras(baseline=float(np.exp(rng.uniform(np.log(0.003), np.log(3.0)))), yaw=float(rng.uniform(-8, 8)))
        X = ts.cloud(rng, 1, 0.3, 30.0)[0]
        xn = []
        for c in (c1, c2):
            Xc = c["Rcw"].astype(F64) @ X + c["tcw"].astype(F64)
            xn.append(np.array([Xc[0] / Xc[2], Xc[1] / Xc[2], 1.0], F32))
        A.append(tr.triangulation_matrix(xn[0], xn[1], c1, c2))
    A = np.stack(A)
    v = hc.null_vectors(A)
    exact = np.array([ts.exact_x3d(a) for a in A])
    dev = np.linalg.norm(v[:, :3] / v[:, 3:] - exact, axis=1) / np.linalg.norm(exact, axis=1)
    print("largest deviation of the double Jacobi from LAPACK: %.3g" % dev.max())
    assert dev.max() < 1e-9
    assert np.allclose(np.linalg.norm(v, axis=1), 1.0, atol=1e-12)


def test_argument_checks_that_need_no_device():
    n1, n2, o1, o2 = 5, 4, np.zeros(5, I32), np.array([0, 1, 2, 3], I32)
    m = np.array([-1, 0, 3, -1, 2], I32)
    assert hc.args_ok(n1, n2, m, o1, o2, 4) and hc.args_ok(n1, n2, m, o1, o2, 4, 8, [7, 0, 3])
    assert hc.args_ok(0, 0, [], [], [], 1) and hc.args_ok(n1, n2, m, o1, o2, 4, 8, [])
    assert not hc.args_ok(n1, n2, np.array([-1, 0, 4, -1, 2], I32), o1, o2, 4)      # a match outside [0, n2)
    assert hc.args_ok(n1, n2, np.array([-7, 0, 3, -1, 2], I32), o1, o2, 4)          # any negative value is "none"
    assert not hc.args_ok(n1, n2, m, o1, o2, 3) and not hc.args_ok(n1, n2, m, o1 - 1, o2, 4)  # octaves of either frame
    assert not hc.args_ok(n1, n2, m, o1, o2, 0) and not hc.args_ok(n1, n2, m, o1, o2, 17)
    assert not hc.args_ok(n1, n2, m, o1, o2, 4, 8, [7, 8]) and not hc.args_ok(n1, n2, m, o1, o2, 4, 8, [-1])
    assert not hc.args_ok(n1, n2, m, o1, o2, 4, 8, [3, 5, 3])                       # listed twice
