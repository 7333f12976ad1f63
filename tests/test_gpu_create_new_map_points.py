"""CreateNewMapPoints on resident keyframes on the device (vsg_frame_set_stereo_points, vsg_frame_triangulate_matches,
vsg_frame_create_new_map_points; k_new_points of csrc/vsg_triangulate.hip) against the HOST BUILD of the same header
(tests/_triangulatecore): reason, source, x3d, new_slot and n_created bit for bit on every scene of
tests/triangulation_scenes.py (no exemptions here: the scenes' thresholds and the measured TOL belong to the CPU test of the host
build against the restatement), the store writes read back from a store pre-filled with a sentinel pattern, the fused call
against the existing search followed by the triangulation call, and the refusals."""
import numpy as np
import pytest

import triangulation_hostcore as hc
import triangulation_reference as tr
import triangulation_scenes as ts
from visual_sgraphs_amd import orb, synth

pytestmark = pytest.mark.gpu
F32, I32, U8 = np.float32, np.int32, np.uint8
INVALID, UNSUPPORTED = -6, -3
CAP = 2048
FIELDS = ("world_pos", "normal", "min_dist", "max_dist", "desc", "observed")


def pose(c):
    return orb.FramePose.make(c["Rcw"], c["tcw"], c["Ow"], c["fx"], c["fy"], c["cx"], c["cy"], c["mbf"], 0.0, ts.NLEVELS)


def params(P):
    return orb.TriangulationParams.make(pose(P["kf1"]), pose(P["kf2"]), P["ratio_factor"], P["inertial"], P["far_points"],
                                        P["th_far_points"], P["kf2_first"])


def resident(s, attach=True):
    out = []
    for t in ("1", "2"):
        f = orb.Frame(max(len(s["k" + t]), 1)).upload(s["k" + t], s["d" + t], ts.BOUNDS, u_right=s["ur" + t])
        if attach:
            f.SetStereoPoints(s["stereo" + t][:, :3], s["stereo" + t][:, 3])
        out.append(f)
    return out


def tables(s):
    return s["sf1"], s["sigma2_1"], s["sf2"], s["sigma2_2"]


def same_bits(a, b):
    """Bit for bit, NaNs canonicalised: a NaN's payload is the one thing the two sides may carry differently."""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def assert_outputs(got, want, what):
    for k in ("reason", "source", "new_slot"):
        assert np.array_equal(got[k], want[k]), (what, k)
    assert same_bits(got["x3d"], want["x3d"]), what
    assert got["n_created"] == want["n_created"], what


@pytest.fixture(scope="module")
def sentinel():
    rng = np.random.default_rng(99)
    return dict(world_pos=rng.normal(size=(CAP, 3)).astype(F32), normal=rng.normal(size=(CAP, 3)).astype(F32),
                min_dist=rng.random(CAP).astype(F32), max_dist=rng.random(CAP).astype(F32),
                desc=rng.integers(0, 256, (CAP, 32)).astype(U8), observed=np.full(CAP, 7, U8))


@pytest.fixture(scope="module")
def store(sentinel):
    mp = orb.MapPoints(CAP)
    yield mp
    mp.close()


def refill(mp, sentinel):
    mp.update(np.arange(CAP), **sentinel)


def assert_store(mp, want, what):
    got = mp.read(np.arange(CAP))
    for k in FIELDS:
        if got[k].dtype == np.float32:
            assert same_bits(got[k], want[k]), (what, k)
        else:
            assert np.array_equal(got[k], want[k]), (what, k)


# ------------------------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("kf2_first", [False, True])
def test_parity_scene_geometry_and_store_equal_the_host_build(store, sentinel, kf2_first):
    s = ts.parity(kf2_first=kf2_first)
    f1, f2 = resident(s)
    P = params(s["P"])
    want = hc.loop(s, s["matches"])
    got = f1.TriangulateMatches(f2, s["matches"], P, *tables(s))
    assert_outputs(got, want, "geometry only")
    assert (want["reason"] == tr.ACCEPTED).sum() >= 150 and set(want["source"].tolist()) == {0, 1, 2}
    accepted = np.flatnonzero(want["reason"] == tr.ACCEPTED)
    rng = np.random.default_rng(5)
    for n_free in (len(accepted) + 3, len(accepted), len(accepted) - 1, 0):
        free = rng.permutation(CAP)[:n_free].astype(I32)
        refill(store, sentinel)
        want = hc.loop(s, s["matches"], sentinel, free)
        got = f1.TriangulateMatches(f2, s["matches"], P, *tables(s), mp=store, free_slots=free)
        assert_outputs(got, want, n_free)
        k = min(n_free, len(accepted))
        assert got["n_created"] == k and np.array_equal(got["new_slot"][accepted[:k]], free[:k])  # ascending idx1
        assert (got["reason"][accepted[k:]] == tr.NO_FREE_SLOT).all()
        assert_store(store, want["store"], n_free)
        after = store.read(free[:k])
        assert same_bits(after["world_pos"], got["x3d"][accepted[:k]]) and (after["observed"] == 1).all()
        rows = s["d2"][s["matches"][accepted[:k]]] if kf2_first else s["d1"][accepted[:k]]
        assert np.array_equal(after["desc"], rows)
        for p in range(0, k, 7):  # tests/observations_reference.py on the two-entry list
            i = accepted[p]
            nrm, mn, mx = tr.normal_and_depth(s["P"], got["x3d"][i], s["k1"]["octave"][i], s["sf1"], s["nlevels"])
            assert same_bits(after["normal"][p], nrm) and same_bits(after["min_dist"][p], mn) and same_bits(after["max_dist"][p], mx)
    f1.close(), f2.close()


def test_directed_scenes_equal_the_host_build(store, sentinel):
    seen = set()
    for name, (s, reason, source) in ts.directed().items():
        f1, f2 = resident(s)
        want = hc.loop(s, s["matches"], sentinel, [11])
        refill(store, sentinel)
        got = f1.TriangulateMatches(f2, s["matches"], params(s["P"]), *tables(s), mp=store, free_slots=[11])
        assert_outputs(got, want, name)
        assert (got["reason"][0], got["source"][0]) == (reason, source), name
        assert_store(store, want["store"], name)
        seen.add(reason)
        f1.close(), f2.close()
    assert seen == set(range(11))


@pytest.mark.parametrize("n", ts.EDGE_COUNTS)
def test_edge_scenes_equal_the_host_build(store, sentinel, n):
    """Feature counts around the wave and chunk sizes of the scan; matches none, all, and on both sides of every boundary; n_free
    of 0, the accepted count and one less."""
    if n == 0:
        s = ts.build(np.zeros((0, 3)), *ts.cameras(), np.random.default_rng(1))
        f1, f2 = resident(s)
        got = f1.TriangulateMatches(f2, np.zeros(0, I32), params(s["P"]), *tables(s), mp=store, free_slots=[3, 4])
        assert got["n_created"] == 0 and len(got["reason"]) == 0
        return
    s = ts.edge(n)
    f1, f2 = resident(s)
    P = params(s["P"])
    rng = np.random.default_rng(n)
    for name, which in ts.edge_sets(n).items():
        m = ts.with_matches(s, which)
        for n_free in sorted({0, max(len(which) - 1, 0), len(which)}):
            free = rng.permutation(CAP)[:n_free].astype(I32)
            want = hc.loop(s, m, sentinel, free)
            refill(store, sentinel)
            got = f1.TriangulateMatches(f2, m, P, *tables(s), mp=store, free_slots=free)
            assert_outputs(got, want, (name, n_free))
            assert got["n_created"] == min(n_free, len(which))
            assert_store(store, want["store"], (name, n_free))
    f1.close(), f2.close()


# --------------------------------------------------------------------------------------------------------- fused call
def _fused_args(s, ori):
    return (s["F12"], s["ep"], False, False, ori, params(s["P"]), *tables(s))


@pytest.mark.parametrize("ori", [True, False], ids=["orientation", "no_orientation"])
@pytest.mark.parametrize("fv", ["host", "resident"])
def test_fused_call_equals_the_search_followed_by_the_triangulation(store, sentinel, ori, fv):
    s = ts.parity()
    f1, f2 = resident(s)
    fvs = (s["fv1"], s["fv2"])
    if fv == "resident":
        voc = orb.ORBVocabulary(synth.synthetic_vocabulary(10, 6, seed=17, stop_fraction=0.05))
        f1.ComputeBoW(voc), f2.ComputeBoW(voc)
        fvs = (None, None)
    free = np.random.default_rng(8).permutation(CAP)[:100].astype(I32)  # fewer than the accepted pairs of the host form
    nm, m12 = f1.SearchForTriangulationEpipolar(s["no_mp1"], f2, s["no_mp2"], s["F12"], s["ep"], s["sf2"], s["sigma2_2"], False,
                                                False, ori, *fvs)
    refill(store, sentinel)
    two = f1.TriangulateMatches(f2, m12, params(s["P"]), *tables(s), mp=store, free_slots=free)
    two_store = store.read(np.arange(CAP))
    refill(store, sentinel)
    one = f1.CreateNewMapPoints(s["no_mp1"], f2, s["no_mp2"], *_fused_args(s, ori), mp=store, free_slots=free, fv1=fvs[0],
                                fv2=fvs[1])
    assert one["nmatches"] == nm and np.array_equal(one["matches12"], m12)
    assert_outputs(one, two, (ori, fv))
    assert_store(store, two_store, (ori, fv))
    assert nm >= (150 if fv == "host" else 20) and one["n_created"] >= (100 if fv == "host" else 5)
    if fv == "host":
        # the rotated group: pairs every gate accepts, removed by the rotation-consistency filter alone
        plain = f1.SearchForTriangulationEpipolar(s["no_mp1"], f2, s["no_mp2"], s["F12"], s["ep"], s["sf2"], s["sigma2_2"],
                                                  False, False, False, *fvs)[1]
        geometry = hc.loop(s, plain)
        removed = np.flatnonzero((plain >= 0) & (geometry["reason"] == tr.ACCEPTED) & (m12 < 0))
        if ori:
            assert len(removed) >= 1 and (one["reason"][removed] == tr.NO_MATCH).all()
        else:
            assert len(removed) == 0
    f1.close(), f2.close()


def test_fused_call_without_a_shared_node_or_with_an_empty_frame(store):
    s = ts.parity()
    f1, f2 = resident(s)
    ids2, off2, idx2 = s["fv2"]
    got = f1.CreateNewMapPoints(s["no_mp1"], f2, s["no_mp2"], *_fused_args(s, True), mp=store, free_slots=[1, 2],
                                fv1=s["fv1"], fv2=(ids2 + 1000, off2, idx2))
    assert got["nmatches"] == 0 and got["n_created"] == 0 and (got["reason"] == tr.NO_MATCH).all() and (got["new_slot"] == -1).all()
    e = ts.build(np.zeros((0, 3)), *ts.cameras(), np.random.default_rng(1))
    e2 = resident(e)[1]
    got = f1.CreateNewMapPoints(s["no_mp1"], e2, np.zeros(0, U8), *_fused_args(s, True), mp=store, free_slots=[1, 2],
                                fv1=s["fv1"], fv2=e["fv2"])
    assert got["nmatches"] == 0 and got["n_created"] == 0 and (got["matches12"] == -1).all()


# ---------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_nothing_enqueued_and_the_outputs_alone(store, sentinel):
    s = ts.parity()
    f1, f2 = resident(s)
    P = params(s["P"])
    n1, n2 = len(s["k1"]), len(s["k2"])
    want = hc.loop(s, s["matches"], sentinel, np.arange(300, dtype=I32))

    def valid():
        refill(store, sentinel)
        got = f1.TriangulateMatches(f2, s["matches"], P, *tables(s), mp=store, free_slots=np.arange(300))
        assert_outputs(got, want, "after a refusal")
        assert_store(store, want["store"], "after a refusal")

    def code(fn, *a, **kw):
        with pytest.raises(orb.VsgError) as e:
            fn(*a, **kw)
        valid()
        return e.value.code
    valid()
    refill(store, sentinel)
    bad = s["matches"].copy()
    bad[5] = n2
    assert code(f1.TriangulateMatches, f2, bad, P, *tables(s), mp=store, free_slots=[1]) == INVALID
    assert code(f1.TriangulateMatches, f2, s["matches"], P, *tables(s), mp=store, free_slots=[1, CAP]) == INVALID
    assert code(f1.TriangulateMatches, f2, s["matches"], P, *tables(s), mp=store, free_slots=[-1]) == INVALID
    assert code(f1.TriangulateMatches, f2, s["matches"], P, *tables(s), mp=store, free_slots=[4, 9, 4]) == INVALID
    short = tuple(t[:3] for t in tables(s))  # an octave of either frame >= nlevels
    assert code(f1.TriangulateMatches, f2, s["matches"], P, *short) == INVALID
    seventeen = tuple(np.ones(17, F32) for _ in range(4))
    assert code(f1.TriangulateMatches, f2, s["matches"], P, *seventeen) == INVALID
    rig = orb.Frame(n2).upload(s["k2"], s["d2"], ts.BOUNDS, nleft=n2 // 2)
    assert code(f1.TriangulateMatches, rig, s["matches"], P, *tables(s)) == UNSUPPORTED
    # the stereo attachment: required where mvuRight has entries >= 0, not otherwise, dropped by an upload
    g1, g2 = resident(s, attach=False)
    assert code(g1.TriangulateMatches, f2, s["matches"], P, *tables(s)) == INVALID
    assert code(f1.TriangulateMatches, g2, s["matches"], P, *tables(s)) == INVALID
    assert code(f1.CreateNewMapPoints, s["no_mp1"], g2, s["no_mp2"], *_fused_args(s, True), fv1=s["fv1"], fv2=s["fv2"]) == INVALID
    f2.upload(s["k2"], s["d2"], ts.BOUNDS, u_right=s["ur2"])
    with pytest.raises(orb.VsgError) as e:
        f1.TriangulateMatches(f2, s["matches"], P, *tables(s))
    assert e.value.code == INVALID
    f2.SetStereoPoints(s["stereo2"][:, :3], s["stereo2"][:, 3])
    valid()
    mono1 = orb.Frame(n1).upload(s["k1"], s["d1"], ts.BOUNDS)
    mono2 = orb.Frame(n2).upload(s["k2"], s["d2"], ts.BOUNDS, u_right=np.full(n2, -1, F32))
    sm = dict(s, ur1=None, ur2=np.full(n2, -1, F32))
    got = mono1.TriangulateMatches(mono2, s["matches"], P, *tables(s))
    assert_outputs(got, hc.loop(sm, s["matches"]), "no mvuRight, nothing attached")
    # the fused call checks its search arguments and its angles the same way
    ids, off, idx = s["fv1"]
    bidx = idx.copy()
    bidx[3] = n1
    assert code(f1.CreateNewMapPoints, s["no_mp1"], f2, s["no_mp2"], *_fused_args(s, True), mp=store, free_slots=[1],
                fv1=(ids, off, bidx), fv2=s["fv2"]) == INVALID
    assert code(f1.CreateNewMapPoints, s["no_mp1"], f2, s["no_mp2"], *_fused_args(s, True), mp=store, free_slots=[1, 1],
                fv1=s["fv1"], fv2=s["fv2"]) == INVALID
    k = s["k1"].copy()
    k["angle"][2] = 400.0
    wild = orb.Frame(n1).upload(k, s["d1"], ts.BOUNDS, u_right=s["ur1"]).SetStereoPoints(s["stereo1"][:, :3], s["stereo1"][:, 3])
    assert code(wild.CreateNewMapPoints, s["no_mp1"], f2, s["no_mp2"], *_fused_args(s, True), fv1=s["fv1"], fv2=s["fv2"]) == INVALID
    if orb.device_count() > 1:
        other = orb.MapPoints(16, device=1)
        assert code(f1.TriangulateMatches, f2, s["matches"], P, *tables(s), mp=other, free_slots=[1]) == INVALID
