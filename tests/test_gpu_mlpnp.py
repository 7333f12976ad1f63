"""MLPnPsolver on a resident frame and resident map points on the device (vsg_frame_mlpnp_ransac; k_mlpnp_points, k_mlpnp_hypotheses,
k_mlpnp_select of csrc/vsg_mlpnp.hip) against the HOST BUILD of the same header
(tests/_mlpnpcore): res, inlier, hyp_inliers and hyp_T byte for byte (both sides canonicalise NaNs), with no exemptions -- the
measured tolerance belongs to the CPU test of the host build against the restatement.  Shapes: the correspondences at the
wave's stride, scattered among the features of a frame whose feature count is no multiple of 64 with negative slots in
between and a store larger than the scene, and past the 256 lanes of a workgroup among up to 720 features; n_hyp around the
waves of a workgroup, past 300 and at its cap of 1024; a directed scene of groups of growing size (284 correspondences, the
last 28 in the second workgroup of k_mlpnp_points), each consistent with a pose of its own, for every way the call can end and
for resumed calls; the planar branch; degenerate sets, one of which gives a NaN pose; the optional outputs NULL; sentinels
behind every output; every refusal a single device can show."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import mlpnp_hostcore as hc
import mlpnp_scenes as ms
from visual_sgraphs_amd import orb

pytestmark = pytest.mark.gpu
F32, F64, I32, U8 = np.float32, np.float64, np.int32, np.uint8
INVALID, UNSUPPORTED = -6, -3
PAD = 64
BOUNDS = (0.0, 0.0, 640.0, 480.0)
SRC = (Path(__file__).resolve().parent.parent / "visual_sgraphs_amd" / "csrc" / "vsg_mlpnp.hip").read_text()
WAVES = int(re.search(r"kMlpnpWaves = (\d+)", SRC).group(1))
GROUPS = (8, 9, 10, 11, 12, 13, 14, 15, 63, 64, 65)  # counts around the wave's stride


def keypoints(s):
    k = np.zeros(s["n_feat"], orb.KP_DTYPE)
    k["x"], k["y"], k["octave"], k["size"], k["angle"] = s["kx"], s["ky"], s["octave"], 31.0, -1.0
    return k


class Device:
    """A scene's frame and store on the device."""

    def __init__(self, s, nleft=-1):
        self.s = s
        self.frame = orb.Frame(s["n_feat"] + 3).upload(keypoints(s), np.zeros((s["n_feat"], 32), U8), BOUNDS, nleft=nleft)
        self.mp = orb.MapPoints(s["capacity"])
        self.mp.update(np.arange(s["capacity"]), world_pos=s["world_pos"])

    def close(self):
        self.frame.close(), self.mp.close()


def raw_call(d, min_inliers, max_its, first, n_iterations, sets, want_hyp=True, **kw):
    """The C entry point on buffers with PAD sentinel entries behind every output.  kw replaces single arguments."""
    L, s = orb.load_library(), d.s
    sm = None if sets is None else np.ascontiguousarray(sets, I32).reshape(-1)
    a = dict(frame=d.frame.handle, mp=d.mp.handle, slots=s["slots"], cam=ms.CAM, sigma2=ms.LEVEL_SIGMA2, nlevels=ms.NLEVELS,
             th2=ms.TH2, n_hyp=0 if sm is None else len(sm) // 6, sets=sm, inlier=True, res=True)
    a.update(kw)
    nh, nf = a["n_hyp"], s["n_feat"]
    inl, res = np.full(nf + PAD, 0xC3, U8), np.full(hc.RESULT_BYTES + PAD, 0xC3, U8)
    hcnt, hT = np.full(max(nh, 0) + PAD, -77, I32), np.full(12 * max(nh, 0) + PAD, -5.5, F64)
    p = lambda v, t, ct: None if v is None else np.ascontiguousarray(v, t).ctypes.data_as(C.POINTER(ct))  # noqa: E731
    keep = [None if a[k] is None else np.ascontiguousarray(a[k], t) for k, t in (("slots", I32), ("sigma2", F32), ("sets", I32))]
    rc = L.vsg_frame_mlpnp_ransac(
        a["frame"], a["mp"], p(keep[0], I32, C.c_int32), *[float(F32(c)) for c in a["cam"]], p(keep[1], F32, C.c_float), a["nlevels"],
        float(a["th2"]), min_inliers, max_its, first, n_iterations, nh, p(keep[2], I32, C.c_int32),
        inl.ctypes.data_as(C.POINTER(C.c_uint8)) if a["inlier"] else None,
        C.cast(res.ctypes.data, C.POINTER(orb.MlpnpResult)) if a["res"] else None,
        hcnt.ctypes.data_as(C.POINTER(C.c_int32)) if want_hyp else None, hT.ctypes.data_as(C.POINTER(C.c_double)) if want_hyp else None)
    return rc, dict(inlier=inl, res=res, hyp_inliers=hcnt, hyp_T=hT, n_hyp=nh)


def untouched(out):
    return (out["inlier"] == 0xC3).all() and (out["res"] == 0xC3).all() and (out["hyp_inliers"] == -77).all() and \
        (out["hyp_T"] == -5.5).all()


def check(d, min_inliers, max_its, first=0, n_iterations=5, sets=None, want_hyp=True, what=""):
    s = d.s
    sm = np.ascontiguousarray(s["sets"] if sets is None else sets, I32).reshape(-1, 6)
    nh, nf = len(sm), s["n_feat"]
    rc, out = raw_call(d, min_inliers, max_its, first, n_iterations, sm, want_hyp)
    assert rc == 0, what
    want = hc.ransac(s, ms.CAM, ms.LEVEL_SIGMA2, ms.TH2, min_inliers, max_its, first, n_iterations, sm)
    got = hc.parse_result(out["res"][:hc.RESULT_BYTES])
    assert got["raw"] == want["res"]["raw"], (what, got, want["res"])
    assert np.array_equal(out["inlier"][:nf], want["inlier"]), what
    assert (out["inlier"][nf:] == 0xC3).all() and (out["res"][hc.RESULT_BYTES:] == 0xC3).all(), what
    if want_hyp and s["n"] >= min_inliers:
        assert np.array_equal(out["hyp_inliers"][:nh], want["hyp_inliers"]), what
        assert out["hyp_T"][:12 * nh].tobytes() == want["hyp_T"].tobytes(), what
        assert (out["hyp_inliers"][nh:] == -77).all() and (out["hyp_T"][12 * nh:] == -5.5).all(), what
    else:
        assert (out["hyp_inliers"] == -77).all() and (out["hyp_T"] == -5.5).all(), what
    return want


@pytest.mark.parametrize("n", (6, 7, 63, 64, 65, 129))
def test_wave_stride_over_the_correspondences(n):
    s = ms.make(200 + n, n=n, n_hyp=5, outliers=0.3 if n > 20 else 0.0)
    d = Device(s)
    w = check(d, 6, 5, what="n %d" % n)
    assert w["res"]["n_correspondences"] == n
    check(d, n, 3, what="only a full count qualifies")
    d.close()


@pytest.mark.parametrize("n,extra", ms.LARGE)
def test_more_than_one_workgroup_of_correspondences(n, extra):
    """blockIdx.x >= 1 in k_mlpnp_points, the later trips of k_mlpnp_select's clearing loop over the features and of its
    scatter through feat[e] with feat[e] != e."""
    s = ms.large_scene(n, extra)
    assert s["n_feat"] > n and (s["where"][256:] != np.arange(256, n)).all()
    d = Device(s)
    w = check(d, 6, 5, what="n %d of %d features" % (n, s["n_feat"]))
    assert w["res"]["n_correspondences"] == n and w["res"]["found"]
    assert w["inlier"][s["where"][256:]].any() or n <= 256  # flags set past the first trip: a dropped trip shows
    check(d, n, 5, what="only a full count qualifies")
    d.close()


def test_planar_branch_past_a_workgroup():
    s = ms.large_scene(257, 100, kind="plane0")
    pts = hc.points(s, ms.CAM, ms.LEVEL_SIGMA2, ms.TH2)
    assert hc.hypotheses(pts, ms.CAM, s["sets"])["info"][:, 0].all()  # the 9-column branch, every hypothesis
    d = Device(s)
    w = check(d, 50, 5, what="planar, n 257")
    assert w["res"]["found"] and w["inlier"][s["where"][256:]].any()
    d.close()


@pytest.mark.parametrize("first,n_iterations,max_its,want_hyp", ((0, 1024, 1, True), (1019, 5, 1024, False)))
def test_hypotheses_at_the_cap_with_the_returned_one_last(first, n_iterations, max_its, want_hyp):
    """n_hyp = mlpnp::kMaxHypotheses: s_counts full, the last sets, counts, hyp and hyp_T records read and written, and the
    selection walks all 1024 counts (a first call, and a resumed one whose max_its reaches the end)."""
    s, sets = ms.winner_last(1024)
    mi = ms.winner_last_min_inliers(hc.ransac(s, ms.CAM, ms.LEVEL_SIGMA2, ms.TH2, s["n"], 1024, 0, 0, sets)["hyp_inliers"])
    d = Device(s)
    w = check(d, mi, max_its, first, n_iterations, sets=sets, want_hyp=want_hyp, what="n_hyp 1024")
    assert w["res"]["found"] and w["res"]["refined"] and w["res"]["best_hypothesis"] == 1023 and w["res"]["iterations"] == 1024
    d.close()


@pytest.fixture(scope="module")
def general():
    d = Device(ms.make(ms.SEEDS[0], n=100, n_hyp=305))
    yield d
    d.close()


@pytest.mark.parametrize("n_hyp", sorted({h for h in (1, WAVES - 1, WAVES, WAVES + 1, 300, 305) if h > 0}))
def test_hypotheses_around_a_workgroup(general, n_hyp):
    # min_inliers = n: no hypothesis qualifies, every one is walked and counted
    w = check(general, general.s["n"], n_hyp, n_iterations=min(5, n_hyp), sets=general.s["sets"][:n_hyp], what="n_hyp %d" % n_hyp)
    assert w["res"]["no_more"] and not w["res"]["found"] and w["res"]["iterations"] == n_hyp


@pytest.fixture(scope="module")
def groups():
    d = Device(ms.group_scene(GROUPS))
    yield d
    d.close()


def test_records_and_every_ending(groups):
    d, nh, n = groups, len(GROUPS), sum(GROUPS)
    w = check(d, 8, nh, what="8 inliers pass the gate and fail Refine(), the next hypothesis returns")
    assert list(w["hyp_inliers"]) == list(GROUPS) and w["res"]["n_records"] == 2
    assert w["res"]["found"] and w["res"]["refined"] and w["res"]["best_hypothesis"] == 1 and w["res"]["iterations"] == 2
    assert w["res"]["n_inliers"] == 9 and np.array_equal(w["res"]["Tcw"][:3], w["hyp_T"][1].astype(F32))  # hypothesis 1 itself
    w = check(d, 65, nh, what="no more, with a best")  # 65 inliers are not MORE than 65
    assert w["res"]["found"] and w["res"]["no_more"] and not w["res"]["refined"] and w["res"]["best_hypothesis"] == nh - 1
    assert w["res"]["n_records"] == 1
    w = check(d, 66, nh, what="no more, without a best")
    assert not w["res"]["found"] and w["res"]["no_more"] and w["res"]["best_hypothesis"] == -1 and (w["res"]["Tcw"] == np.eye(4)).all()
    w = check(d, n + 1, nh, what="N < min_inliers")
    assert w["res"]["no_more"] and w["res"]["iterations"] == 0 and w["res"]["n_records"] == 0
    back = d.s["sets"][::-1]
    w = check(d, 10, nh, sets=back, what="success at k = 0")
    assert w["res"]["found"] and w["res"]["refined"] and w["res"]["iterations"] == 1 and w["res"]["n_records"] == 1
    check(d, 8, nh, want_hyp=False, what="optional outputs NULL")


def test_resumed_calls(groups):
    d, nh = groups, len(GROUPS)
    # at min_inliers 64 nothing returns before the 65: entered past the others, and past max_its
    w = check(d, 64, 4, first=0, n_iterations=5, what="the first call walks max(max_its, n_iterations)")
    assert not w["res"]["found"] and w["res"]["iterations"] == 5 and w["res"]["no_more"]
    w = check(d, 64, 4, first=5, n_iterations=5, what="first >= max_its: five more")
    assert w["res"]["iterations"] == 10 and w["res"]["found"] and not w["res"]["refined"] and w["res"]["best_hypothesis"] == 9
    w = check(d, 64, 4, first=10, n_iterations=1, what="the last hypothesis returns")
    assert w["res"]["found"] and w["res"]["refined"] and w["res"]["best_hypothesis"] == 10 and not w["res"]["no_more"]
    w = check(d, 9, nh, first=3, n_iterations=2, what="first > 0: the best before it is the state")
    assert w["res"]["found"] and w["res"]["iterations"] == 4 and w["res"]["n_records"] == 3
    back = d.s["sets"][::-1]
    w = check(d, 9, nh, first=1, n_iterations=1, sets=back, what="a resumed call returns a hypothesis that is not the best")
    assert w["res"]["refined"] and w["res"]["best_hypothesis"] == 0 and w["res"]["iterations"] == 2 and w["res"]["n_inliers"] == 64
    check(d, 9, 2, first=nh, n_iterations=0, what="nothing left to walk")


def test_planar_branch():
    s = ms.make(ms.SEEDS[1], n=100, kind="plane0", n_hyp=24)
    pts = hc.points(s, ms.CAM, ms.LEVEL_SIGMA2, ms.TH2)
    assert hc.hypotheses(pts, ms.CAM, s["sets"])["info"][:, 0].all()  # the 9-column branch, every hypothesis
    d = Device(s)
    w = check(d, 50, 24, what="planar")
    assert w["res"]["found"]
    check(d, 100, 24, what="planar, every hypothesis")
    d.close()


def test_degenerate_sets():
    s = ms.make(ms.SEEDS[2], n=64, n_hyp=6, outliers=0.0)
    c = s["where"]
    s["world_pos"][s["slots"][c[1]]] = s["world_pos"][s["slots"][c[0]]]  # two samples with one 3D position: a finite pose
    s["kx"][c[1]], s["ky"][c[1]] = s["kx"][c[0]], s["ky"][c[0]]
    s["sets"][0] = [0, 1, 2, 3, 4, 5]
    s["world_pos"][s["slots"][c[6:12]]] = 0.0                            # six samples at the world origin: a NaN translation
    s["sets"][1] = [6, 7, 8, 9, 10, 11]
    d = Device(s)
    other = hc.ransac(ms.make(ms.SEEDS[2], n=64, n_hyp=6, outliers=0.0), ms.CAM, ms.LEVEL_SIGMA2, ms.TH2, 64, 6, 0, 5)
    w = check(d, 64, 6, what="degenerate")
    nan = np.frombuffer(w["hyp_T"][1, :, 3].tobytes(), np.uint64)
    assert (nan == 0x7ff8000000000000).all() and w["hyp_inliers"][1] == 0  # canonical NaNs, no inlier
    assert (w["hyp_T"][1, :, :3] == np.eye(3)).all()                      # acos of a NaN trace: omega = 0
    keep = [k for k in range(2, 6) if not ({1, 6, 7, 8, 9, 10, 11} & set(s["sets"][k]))]
    assert keep and all(w["hyp_T"][k].tobytes() == other["hyp_T"][k].tobytes() for k in keep)  # the others are unaffected
    d.close()


def test_refusals_leave_everything_as_it_was(general):
    d, s = general, general.s
    sm, n = s["sets"][:9], s["n"]

    def edit(a, i, v):
        a = np.array(a, copy=True)
        a.reshape(-1)[i] = v
        return a
    used = np.flatnonzero(s["slots"] >= 0)
    other_levels = int(s["octave"][used].max())
    bad_calls = {
        "frame NULL": dict(frame=None), "store NULL": dict(mp=None), "slots NULL": dict(slots=None), "sigma2 NULL": dict(sigma2=None),
        "sets NULL": dict(sets=None, n_hyp=9), "inlier NULL": dict(inlier=False), "res NULL": dict(res=False),
        "slot == capacity": dict(slots=edit(s["slots"], used[3], s["capacity"])), "nlevels 0": dict(nlevels=0), "nlevels 17": dict(nlevels=17),
        "an octave >= nlevels": dict(nlevels=other_levels), "th2 0": dict(th2=0.0), "th2 < 0": dict(th2=-1.0), "th2 nan": dict(th2=np.nan),
        "th2 inf": dict(th2=np.inf), "min_inliers 5": dict(min_inliers=5), "max_its 0": dict(max_its=0), "first < 0": dict(first=-1),
        "n_iterations < 0": dict(n_iterations=-1), "n_hyp 0": dict(n_hyp=0), "n_hyp 1025": dict(sets=np.tile(sm[:1], (1025, 1))),
        "max_its > n_hyp": dict(max_its=10), "first + n_iterations > n_hyp": dict(first=5, n_iterations=5),
        "sample == n": dict(sets=edit(sm, 4, n)), "sample < 0": dict(sets=edit(sm, 26, -1)), "equal samples": dict(sets=edit(sm, 1, sm[0, 0])),
    }
    for what, kw in bad_calls.items():
        a = dict(min_inliers=10, max_its=9, first=0, n_iterations=5, sets=sm)
        a.update({k: kw.pop(k) for k in list(kw) if k in ("min_inliers", "max_its", "first", "n_iterations")})
        if "sets" in kw:
            a["sets"] = kw.pop("sets")
        rc, out = raw_call(d, a["min_inliers"], a["max_its"], a["first"], a["n_iterations"], a["sets"], **kw)
        assert rc == INVALID and untouched(out), what
    # an octave below 0 cannot reach the call on a resident frame: the upload refuses such a keypoint (the check itself runs
    # in tests/test_abi_mlpnp.py through mlpnp::args_ok)
    neg = ms.make(6, n=20, n_hyp=3)
    neg["octave"][neg["where"][4]] = -1
    with pytest.raises(orb.VsgError):
        Device(neg)
    pair = Device(ms.make(5, n=20, n_hyp=3), nleft=9)
    rc, out = raw_call(pair, 6, 3, 0, 3, pair.s["sets"])
    assert rc == UNSUPPORTED and untouched(out)
    pair.close()
    assert d.mp.read(np.arange(s["capacity"]))["world_pos"].tobytes() == s["world_pos"].tobytes()
    check(d, 50, 9, sets=sm, what="a good call after the refusals")


def test_python_binding(general):
    d, s = general, general.s
    mi, mx = orb.mlpnp_ransac_parameters(s["n"])
    assert (mi, mx) == hc.parameters(0.99, 10, 300, 6, 0.5, s["n"])
    sets = np.concatenate([ms.good_sets(s, 1), s["sets"][:mx]])  # a set of true correspondences first
    got = d.frame.mlpnp_ransac(d.mp, s["slots"], ms.CAM, ms.LEVEL_SIGMA2, sets, mi, mx, th2=ms.TH2, per_hypothesis=True)
    want = hc.ransac(s, ms.CAM, ms.LEVEL_SIGMA2, ms.TH2, mi, mx, 0, 5, sets)
    assert bytes(got["result"]) == want["res"]["raw"] and np.array_equal(got["inlier"], want["inlier"].astype(bool))
    assert np.array_equal(got["hyp_inliers"], want["hyp_inliers"]) and got["hyp_T"].tobytes() == want["hyp_T"].tobytes()
    assert got["found"] and got["refined"] and got["best_hypothesis"] == 0 and got["iterations"] == 1
