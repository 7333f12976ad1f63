"""Sim3Solver on resident map points on the device (vsg_mappoints_sim3_ransac; k_sim3_points, k_sim3_hypotheses, k_sim3_select
of csrc/vsg_sim3.hip) against the HOST BUILD of the same header (tests/_sim3core): res, inlier, hyp_inliers and hyp_T12 byte for
byte (both sides canonicalise NaNs), with no exemptions -- the measured tolerance belongs to the CPU test of the host build
against the restatement.  Shapes: n at the wave's stride over the correspondences and past the 256 lanes of a workgroup, n_hyp
around the waves of a workgroup and at its cap of 1024, every way the selection can end, the degenerate triples, fix_scale, two
stores, sentinels behind every output, and the refusals."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import sim3_hostcore as hc
import sim3_scenes as ss
from visual_sgraphs_amd import orb

pytestmark = pytest.mark.gpu
F32, I32, U8 = np.float32, np.int32, np.uint8
INVALID = -6
CAP1, CAP2, PAD = 640, 320, 64
BIG1, BIG2 = 1500, 900  # the stores of the cases with more than 256 correspondences: 513 random slots each
SRC = Path(__file__).resolve().parent.parent / "visual_sgraphs_amd" / "csrc" / "vsg_sim3.hip"
WAVES = int(re.search(r"kSim3Waves = (\d+)", SRC.read_text()).group(1))


def pose(kf):
    return orb.FramePose.make(kf["Rcw"], kf["tcw"], np.zeros(3), kf["fx"], kf["fy"], kf["cx"], kf["cy"], 0.0, 0.0, 0)


@pytest.fixture(scope="module")
def stores():
    rng = np.random.default_rng(3)
    fill = [rng.normal(size=(CAP1, 3)).astype(F32), rng.normal(size=(CAP2, 3)).astype(F32)]
    mps = [orb.MapPoints(CAP1), orb.MapPoints(CAP2)]
    for mp, f in zip(mps, fill):
        mp.update(np.arange(len(f)), world_pos=f)
    yield mps, fill
    for mp in mps:
        mp.close()


@pytest.fixture(scope="module")
def big_stores():
    rng = np.random.default_rng(4)
    fill = [rng.normal(size=(BIG1, 3)).astype(F32), rng.normal(size=(BIG2, 3)).astype(F32)]
    mps = [orb.MapPoints(BIG1), orb.MapPoints(BIG2)]
    for mp, f in zip(mps, fill):
        mp.update(np.arange(len(f)), world_pos=f)
    yield mps, fill
    for mp in mps:
        mp.close()


def place(stores, s, seed=0, one_store=False):
    """The scene's points into random slots of the two stores (one_store: both sets into the first).  Returns mp1, mp2, slots1,
    slots2 and what both stores hold afterwards."""
    (mp1, mp2), fill = stores
    rng = np.random.default_rng(seed)
    n, cap1, cap2 = s["n"], len(fill[0]), len(fill[1])
    if one_store:
        perm = rng.permutation(cap1)
        sl1, sl2, mp2 = perm[:n].astype(I32), perm[n:2 * n].astype(I32), mp1
    else:
        sl1, sl2 = rng.permutation(cap1)[:n].astype(I32), rng.permutation(cap2)[:n].astype(I32)
    if n:
        mp1.update(sl1, world_pos=s["Xw1"])
        mp2.update(sl2, world_pos=s["Xw2"])
    fill[0][sl1] = s["Xw1"]
    fill[0 if one_store else 1][sl2] = s["Xw2"]
    return mp1, mp2, sl1, sl2


def raw_call(mp1, mp2, n, sl1, sl2, e1, e2, kf1, kf2, fix_scale, min_inliers, samples, want_hyp=True, n_hyp=None):
    """The C entry point on buffers with PAD sentinel entries behind every output.  Returns rc and the buffers."""
    L = orb.load_library()
    sm = np.ascontiguousarray(samples, I32).reshape(-1)
    nh = len(sm) // 3 if n_hyp is None else n_hyp
    inl = np.full(n + PAD, 0xC3, U8)
    res = np.full(hc.RESULT_BYTES + PAD, 0xC3, U8)
    hcnt, hT = np.full(max(nh, 0) + PAD, -77, I32), np.full(16 * max(nh, 0) + PAD, -5.5, F32)
    p = lambda a, t: None if a is None else np.ascontiguousarray(a).ctypes.data_as(C.POINTER(t))  # noqa: E731
    keep = [None if a is None else np.ascontiguousarray(a, t) for a, t in ((sl1, I32), (sl2, I32), (e1, F32), (e2, F32))]
    rc = L.vsg_mappoints_sim3_ransac(mp1.handle if mp1 else None, mp2.handle if mp2 else None, n, p(keep[0], C.c_int32),
                                     p(keep[1], C.c_int32), p(keep[2], C.c_float), p(keep[3], C.c_float), C.byref(kf1), C.byref(kf2),
                                     int(fix_scale), min_inliers, nh, p(sm, C.c_int32), p(inl, C.c_uint8),
                                     C.cast(res.ctypes.data, C.POINTER(orb.Sim3Result)), p(hcnt, C.c_int32) if want_hyp else None,
                                     p(hT, C.c_float) if want_hyp else None)
    return rc, dict(inlier=inl, res=res, hyp_inliers=hcnt, hyp_T12=hT, n_hyp=nh)


def untouched(out):
    return (out["inlier"] == 0xC3).all() and (out["res"] == 0xC3).all() and (out["hyp_inliers"] == -77).all() and \
        (out["hyp_T12"] == F32(-5.5)).all()


def check(stores, s, min_inliers=15, fix_scale=False, samples=None, want_hyp=True, one_store=False, what=""):
    mp1, mp2, sl1, sl2 = place(stores, s, one_store=one_store)
    sm = np.ascontiguousarray(s["samples"] if samples is None else samples, I32).reshape(-1, 3)
    n, nh = s["n"], len(sm)
    rc, out = raw_call(mp1, mp2, n, sl1, sl2, s["max_err1"], s["max_err2"], pose(s["kf1"]), pose(s["kf2"]), fix_scale, min_inliers,
                       sm, want_hyp)
    assert rc == 0, what
    want = hc.ransac(s, min_inliers, fix_scale, sm)
    assert out["res"][:hc.RESULT_BYTES].tobytes() == want["res"]["raw"], (what, hc.parse_result(out["res"][:hc.RESULT_BYTES]), want["res"])
    assert np.array_equal(out["inlier"][:n], want["inlier"]), what
    assert (out["inlier"][n:] == 0xC3).all() and (out["res"][hc.RESULT_BYTES:] == 0xC3).all(), what
    if want_hyp and n >= min_inliers:
        assert np.array_equal(out["hyp_inliers"][:nh], want["hyp_inliers"]), what
        assert out["hyp_T12"][:16 * nh].tobytes() == want["hyp_T12"].tobytes(), what
        assert (out["hyp_inliers"][nh:] == -77).all() and (out["hyp_T12"][16 * nh:] == F32(-5.5)).all(), what
    else:
        assert (out["hyp_inliers"] == -77).all() and (out["hyp_T12"] == F32(-5.5)).all(), what
    return want


@pytest.mark.parametrize("n", (63, 64, 65, 129))
def test_wave_stride_over_the_correspondences(stores, n):
    s = ss.make(100 + n, n=n, n_hyp=2 * WAVES + 1)
    w = check(stores, s, min_inliers=n, what="never")  # every hypothesis counts every correspondence
    assert not w["res"]["converged"] and w["res"]["iterations"] == 2 * WAVES + 1
    check(stores, s, min_inliers=15, fix_scale=True)


@pytest.mark.parametrize("fix_scale", (False, True))
@pytest.mark.parametrize("n", ss.LARGE_SIZES)
def test_more_than_one_workgroup_of_correspondences(big_stores, n, fix_scale):
    """blockIdx.x >= 1 in k_sim3_points and the second and third trips of k_sim3_select's loop over the correspondences."""
    s = ss.large_scene(n)
    w = check(big_stores, s, min_inliers=n, fix_scale=fix_scale, what="never")  # every hypothesis counts every correspondence
    assert not w["res"]["converged"] and w["res"]["iterations"] == 9
    assert w["inlier"][256:].any() or n <= 256  # the flags past the first trip are not all zero: a dropped trip shows
    check(big_stores, s, min_inliers=15, fix_scale=fix_scale)
    (mp1, mp2), fill = big_stores
    assert mp1.read(np.arange(BIG1))["world_pos"].tobytes() == fill[0].tobytes()
    assert mp2.read(np.arange(BIG2))["world_pos"].tobytes() == fill[1].tobytes()


@pytest.mark.parametrize("n_hyp", (1023, 1024))
def test_hypotheses_at_the_cap_with_the_returned_one_last(stores, n_hyp):
    """n_hyp = sim3::kMaxHypotheses: s_counts full, the last samples, counts and hyp_T12 records read and written."""
    s, sm = ss.winner_last(n_hyp)
    mi = ss.winner_last_min_inliers(hc.ransac(s, 0, False, sm)["hyp_inliers"])
    w = check(stores, s, min_inliers=mi, samples=sm, what="n_hyp %d" % n_hyp)
    assert w["res"]["converged"] and w["res"]["best_hypothesis"] == n_hyp - 1 and w["res"]["iterations"] == n_hyp
    check(stores, s, min_inliers=mi, samples=sm, want_hyp=False, what="n_hyp %d, optional outs NULL" % n_hyp)


def test_three_correspondences(stores):
    s = ss.make(7, n=3, outliers=0.0, noise=0.001, n_hyp=1)
    sm = np.array([[0, 1, 2], [2, 0, 1], [1, 2, 0], [2, 1, 0]], I32)
    w = check(stores, s, min_inliers=2, samples=sm)
    assert w["res"]["converged"] and w["res"]["n_inliers"] == 3
    check(stores, s, min_inliers=3, samples=sm)  # 3 is not above 3: never converges, the last of the tie
    w = check(stores, s, min_inliers=4, samples=sm)  # N < mRansacMinInliers: nothing is computed
    assert w["res"]["no_more"] and w["res"]["best_hypothesis"] == -1 and (w["res"]["T12"] == np.eye(4)).all()


@pytest.mark.parametrize("n_hyp", (1, WAVES - 1, WAVES, WAVES + 1, 300))
@pytest.mark.parametrize("fix_scale", (False, True))
def test_hypotheses_around_a_workgroup(stores, n_hyp, fix_scale):
    s = ss.issue_scene(ss.SEEDS[0])
    check(stores, s, samples=s["samples"][:n_hyp], fix_scale=fix_scale, what="n_hyp %d" % n_hyp)


def test_every_way_the_selection_ends(stores):
    s = ss.issue_scene(ss.SEEDS[1])
    good = np.array([int(i) for i in np.flatnonzero(~s["outlier"])[:3]], I32)
    bad = np.array([int(i) for i in np.flatnonzero(s["outlier"])[:3]], I32)
    w = check(stores, s, samples=np.stack([good] + [bad] * 6), what="at hypothesis 0")
    assert w["res"]["converged"] and w["res"]["best_hypothesis"] == 0 and w["res"]["iterations"] == 1
    w = check(stores, s, samples=np.stack([bad] * 6 + [good]), what="at the last hypothesis")
    assert w["res"]["converged"] and w["res"]["best_hypothesis"] == 6 and w["res"]["iterations"] == 7
    w = check(stores, s, min_inliers=s["n"], what="never")
    assert not w["res"]["converged"] and w["res"]["no_more"] and w["res"]["iterations"] == 300
    w = check(stores, s, min_inliers=s["n"], samples=np.stack([bad, good, bad, good, bad, bad]), what="a tie of the maximum")
    assert w["res"]["best_hypothesis"] == 3 and w["hyp_inliers"][1] == w["hyp_inliers"][3] == w["res"]["n_inliers"]
    check(stores, s, want_hyp=False, what="optional outs NULL")
    check(stores, s, one_store=True, what="both point sets in one store")


def test_degenerate_triples(stores):
    base = ss.issue_scene(ss.SEEDS[2])
    sm = np.concatenate([[[0, 1, 2]], base["samples"][:6]]).astype(I32)
    w = check(stores, ss.collinear_triple(base), samples=sm, what="collinear")
    s = ss.identical_triple(base)
    w = check(stores, s, samples=sm, min_inliers=s["n"], what="P1 == P2")
    assert w["hyp_inliers"][0] == 0 and np.isnan(w["hyp_T12"][0, :3, :3]).all()
    w = check(stores, s, samples=np.array([[0, 1, 2], [1, 2, 0]], I32), min_inliers=s["n"], what="only NaN hypotheses")
    assert w["res"]["best_hypothesis"] == 1 and np.isnan(w["res"]["R12"]).all() and not w["inlier"].any()


def test_refusals_leave_everything_as_it_was(stores):
    s = ss.issue_scene(ss.SEEDS[3])
    mp1, mp2, sl1, sl2 = place(stores, s)
    n, sm = s["n"], s["samples"][:9]
    k1, k2, e1, e2 = pose(s["kf1"]), pose(s["kf2"]), s["max_err1"], s["max_err2"]

    def edit(a, i, v):
        a = np.array(a, copy=True)
        a.reshape(-1)[i] = v
        return a
    bad_calls = {
        "mp1 NULL": dict(mp1=None), "mp2 NULL": dict(mp2=None), "n < 0": dict(n=-1), "slots1 NULL": dict(sl1=None),
        "max_err2 NULL": dict(e2=None), "slot1 past the store": dict(sl1=edit(sl1, 5, CAP1)), "slot2 negative": dict(sl2=edit(sl2, 0, -1)),
        "slot2 past ITS store": dict(sl2=edit(sl2, 7, CAP2)), "n_hyp 0": dict(n_hyp=0), "n_hyp 1025": dict(samples=np.tile(sm[:1], (1025, 1))),
        "min_inliers < 0": dict(min_inliers=-1), "sample == n": dict(samples=edit(sm, 4, n)), "sample < 0": dict(samples=edit(sm, 26, -1)),
        "equal samples": dict(samples=edit(sm, 1, sm[0, 0])), "n < 3": dict(n=2, min_inliers=2),
    }
    for what, kw in bad_calls.items():
        a = dict(mp1=mp1, mp2=mp2, n=n, sl1=sl1, sl2=sl2, e1=e1, e2=e2, kf1=k1, kf2=k2, fix_scale=False, min_inliers=15, samples=sm)
        a.update(kw)
        rc, out = raw_call(**a)
        assert rc == INVALID and untouched(out), what
    (_, _), fill = stores
    assert mp1.read(np.arange(CAP1))["world_pos"].tobytes() == fill[0].tobytes()
    assert mp2.read(np.arange(CAP2))["world_pos"].tobytes() == fill[1].tobytes()
    check(stores, s, what="a good call after the refusals")


def test_python_binding(stores):
    s = ss.issue_scene(ss.SEEDS[0])
    mp1, mp2, sl1, sl2 = place(stores, s)
    got = mp1.Sim3Ransac(sl1, sl2, orb.sim3_max_err(ss.SIGMA2, s["oct1"]), orb.sim3_max_err(ss.SIGMA2, s["oct2"]), pose(s["kf1"]),
                         pose(s["kf2"]), s["samples"], 15, other=mp2, per_hypothesis=True)
    want = hc.ransac(s)
    assert bytes(got["result"]) == want["res"]["raw"] and np.array_equal(got["inlier"], want["inlier"].astype(bool))
    assert np.array_equal(got["hyp_inliers"], want["hyp_inliers"]) and got["converged"] and got["iterations"] == got["best_hypothesis"] + 1
