"""TwoViewReconstruction::Reconstruct on the device (vsg_frame_two_view_reconstruct / vsg_two_view_reconstruct; k_tv_prepare,
k_tv_hypotheses, k_tv_select, k_tv_check_rt of csrc/vsg_two_view.hip) against the HOST BUILD of the same header
(tests/_twoviewcore): the result, triangulated, x3d, both inlier vectors and every score byte for byte (both sides canonicalise
NaNs), with no exemptions -- the measured tolerance belongs to the CPU test of the host build against the restatement.  Shapes:
the number of matches at the wave's stride and around the 1024-entry LDS tile of the rank count (a rank holder and a tie past the
first tile), n_iter around the waves of a workgroup and at its cap of 1024, the index rule min(50, size - 1) at its edge, every
reason the routine can end with, both models, both forms, sentinels behind every output, and the refusals."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import two_view_hostcore as hc
import two_view_scenes as ts
from test_two_view_reference import tile_cases
from visual_sgraphs_amd import orb

pytestmark = pytest.mark.gpu
F32, I32, U8 = np.float32, np.int32, np.uint8
INVALID = -6
PAD = 64
SRC = Path(__file__).resolve().parent.parent / "visual_sgraphs_amd" / "csrc" / "vsg_two_view.hip"
WAVES = int(re.search(r"kTvWaves = (\d+)", SRC.read_text()).group(1))
BOUNDS = (0.0, 0.0, 640.0, 480.0)


def _ptr(a, t):
    return None if a is None else a.ctypes.data_as(C.POINTER(t))


@pytest.fixture(scope="module")
def frames():
    f = [orb.Frame(4096), orb.Frame(4096)]
    yield f
    for x in f:
        x.close()


def upload(frames, s):
    for f, xy in zip(frames, (s["xy1"], s["xy2"])):
        k = np.zeros(len(xy), orb.KP_DTYPE)
        k["x"], k["y"], k["size"], k["octave"] = xy[:, 0], xy[:, 1], 31.0, 0
        f.upload(k, np.zeros((len(xy), 32), U8), BOUNDS)
    return frames


def buffers(s, n_iter):
    n1, N = len(s["xy1"]), int((s["matches12"] >= 0).sum())
    x3d = np.full(3 * n1 + PAD, hc.X3D_SENTINEL, F32)
    return dict(res=np.full(hc.RESULT_BYTES + PAD, 0xC3, U8), tri=np.full(n1 + PAD, 0xAA, U8), x3d=x3d,
                in_h=np.full(N + PAD, 0xC3, U8), in_f=np.full(N + PAD, 0xC3, U8), sc_h=np.full(n_iter + PAD, -5.5, F32),
                sc_f=np.full(n_iter + PAD, -5.5, F32))


def untouched(b):
    return (b["res"] == 0xC3).all() and (b["tri"] == 0xAA).all() and (b["x3d"] == hc.X3D_SENTINEL).all() and \
        (b["in_h"] == 0xC3).all() and (b["in_f"] == 0xC3).all() and (b["sc_h"] == F32(-5.5)).all() and (b["sc_f"] == F32(-5.5)).all()


def raw_call(frames, s, params_, sets_, resident=True, optional=True, **edit):
    """The C entry point on buffers with PAD sentinel entries behind every output.  edit: arguments replaced (None = NULL)."""
    L = orb.load_library()
    st = np.ascontiguousarray(sets_, I32).reshape(-1, 8)
    a = dict(matches12=np.ascontiguousarray(s["matches12"], I32), K=np.ascontiguousarray(s["K"], F32), params=params_, sets=st,
             n_iter=len(st), f1=frames[0].handle if resident else None, f2=frames[1].handle if resident else None,
             xy1=np.ascontiguousarray(s["xy1"], F32), xy2=np.ascontiguousarray(s["xy2"], F32), device=0, tri=True, x3d=True, res=True)
    a.update(edit)
    b = buffers(s, max(a["n_iter"], 0))
    pp = a["params"]
    tail = (_ptr(a["matches12"], C.c_int32), _ptr(a["K"], C.c_float), None if pp is None else C.cast(pp.ctypes.data, C.POINTER(orb.TwoViewParams)),
            a["n_iter"], _ptr(a["sets"], C.c_int32), C.cast(b["res"].ctypes.data, C.POINTER(orb.TwoViewResult)) if a["res"] else None,
            _ptr(b["tri"], C.c_uint8) if a["tri"] else None, _ptr(b["x3d"], C.c_float) if a["x3d"] else None,
            _ptr(b["in_h"], C.c_uint8) if optional else None, _ptr(b["in_f"], C.c_uint8) if optional else None,
            _ptr(b["sc_h"], C.c_float) if optional else None, _ptr(b["sc_f"], C.c_float) if optional else None)
    if resident:
        rc = L.vsg_frame_two_view_reconstruct(a["f1"], a["f2"], *tail)
    else:
        rc = L.vsg_two_view_reconstruct(a["device"], _ptr(a["xy1"], C.c_float), len(s["xy1"]), _ptr(a["xy2"], C.c_float), len(s["xy2"]), *tail)
    return rc, b


def check(frames, s, params=None, sets=None, resident=True, optional=True, what=""):
    """One call against the host build.  Returns the host build's parsed result."""
    params = hc.params_blob() if params is None else params
    st = np.ascontiguousarray(s["sets"] if sets is None else sets, I32).reshape(-1, 8)
    if resident:
        upload(frames, s)
    rc, b = raw_call(frames, s, params, st, resident, optional)
    assert rc == 0, what
    want = hc.reconstruct(s, params, st)
    n1, N, ni = len(s["xy1"]), int((s["matches12"] >= 0).sum()), len(st)
    assert b["res"][:hc.RESULT_BYTES].tobytes() == want["res"]["raw"], (what, hc.parse_result(b["res"][:hc.RESULT_BYTES]), want["res"])
    assert b["tri"][:n1].tobytes() == want["triangulated"].tobytes(), what
    assert b["x3d"][:3 * n1].tobytes() == want["x3d"].tobytes(), what
    if optional:
        assert b["in_h"][:N].tobytes() == want["inlier_h"].tobytes() and b["in_f"][:N].tobytes() == want["inlier_f"].tobytes(), what
        assert b["sc_h"][:ni].tobytes() == want["score_h"].tobytes() and b["sc_f"][:ni].tobytes() == want["score_f"].tobytes(), what
    else:
        assert (b["in_h"] == 0xC3).all() and (b["in_f"] == 0xC3).all() and (b["sc_h"] == F32(-5.5)).all() and (b["sc_f"] == F32(-5.5)).all()
    # the sentinels behind every output
    assert (b["res"][hc.RESULT_BYTES:] == 0xC3).all() and (b["tri"][n1:] == 0xAA).all() and (b["x3d"][3 * n1:] == hc.X3D_SENTINEL).all()
    assert (b["in_h"][N:] == 0xC3).all() and (b["in_f"][N:] == 0xC3).all() and (b["sc_h"][ni:] == F32(-5.5)).all() and \
        (b["sc_f"][ni:] == F32(-5.5)).all(), what
    return want["res"]


@pytest.mark.parametrize("n", [8, 63, 64, 65, 129])
def test_match_counts_at_the_wave_stride(frames, n):
    s = ts.make(200 + n, n=n, outliers=0.1 if n > 8 else 0.0, n_iter=12, extra1=5, extra2=9)
    r = check(frames, s, hc.params_blob(min_triangulated=4), what="n=%d" % n)
    assert r["n_inliers"] > 0


@pytest.mark.parametrize("n_iter", sorted({1, max(1, WAVES - 1), WAVES + 1, 200}))
def test_iterations_around_the_waves_of_a_workgroup(frames, n_iter):
    s = ts.make(31, n=100, n_iter=200)
    check(frames, s, sets=s["sets"][:n_iter], what="n_iter=%d" % n_iter)


@pytest.mark.parametrize("n", [51, 52, 53])
def test_index_rule_at_its_edge(frames, n):
    """51 / 52 / 53 noise-free matches: min(50, size - 1) is the last, the last but one, the last but two element."""
    s = ts.make(300 + n, n=n, outliers=0.0, noise=0.0, n_iter=16)
    r = check(frames, s, what="n=%d" % n)
    assert r["ok"] == 1 and r["model"] == 1 and max(r["n_good"]) == n


@pytest.mark.parametrize("n", ts.TILE_SIZES)
def test_match_counts_around_the_tile_of_the_rank_count(frames, n):
    """k_tv_check_rt past its first LDS tile: a partial last tile, whole tiles, one match in the last tile, three tiles."""
    r = check(frames, tile_cases()["matches_%d" % n], what="n=%d" % n)
    assert r["ok"] == 1 and r["model"] == 1 and max(r["n_good"]) > 0.8 * n


def test_rank_holder_past_the_first_tile(frames):
    """The candidate trips reach base >= 1024 (tests/test_two_view_reference.py asserts where the rank holder lies)."""
    r = check(frames, tile_cases()["rank_holder_late"])
    assert r["ok"] == 1 and max(r["n_good"]) == 1500


def test_tie_across_the_tile_boundary(frames):
    """Two matches of one cosine, the rank-50 value, at the compacted indices 1023 and 1024: the last entry of the first tile
    and the first of the second."""
    r = check(frames, tile_cases()["tie_across_the_tile"])
    assert r["ok"] == 1


def test_iterations_at_the_cap_with_the_winner_last(frames):
    """n_iter = two_view::kMaxIterations: s_score full, the last records of score and models read."""
    s = tile_cases()["winner_last"]
    r = check(frames, s)
    assert r["best_it_f"] == 1023 and len(s["sets"]) == 1024
    check(frames, s, optional=False)


def test_host_array_form_past_the_tile(frames):
    s = tile_cases()["matches_1025"]
    upload(frames, s)
    rc1, b1 = raw_call(frames, s, hc.params_blob(), s["sets"], resident=True)
    rc2, b2 = raw_call(frames, s, hc.params_blob(), s["sets"], resident=False)
    assert rc1 == 0 and rc2 == 0
    for k in b1:
        assert b1[k].tobytes() == b2[k].tobytes(), k
    check(frames, s, resident=False)


def test_f_path_success_and_the_optional_outputs_null(frames):
    s = ts.issue_scene(11, 100, False)
    r = check(frames, s)
    assert r["ok"] == 1 and r["model"] == 1 and r["reason"] == 0
    check(frames, s, optional=False)


def test_h_path_success_leaves_x3d_alone(frames):
    s = ts.issue_scene(12, 100, True)
    r = check(frames, s, hc.params_blob(rh_threshold=0.40))
    assert r["ok"] == 1 and r["model"] == 0  # check() compared x3d with the host build's, which is all sentinel


def test_reasons(frames):
    g = ts.issue_scene(11, 100, False)
    assert check(frames, g, hc.params_blob(rh_threshold=0.0), what="rh 0")["reason"] == 3       # H forced on a general scene
    assert check(frames, ts.pure_rotation(41), hc.params_blob(rh_threshold=0.40), what="rotation")["reason"] == 2
    assert check(frames, ts.tiny_baseline(42), what="baseline")["reason"] == 4
    assert check(frames, ts.identical_keypoints(), what="identical")["reason"] == 1


def test_first_maximum_with_a_repeated_set_and_a_nan_hypothesis(frames):
    s = ts.nan_hypothesis_scene()
    sets = s["sets"].copy()
    r0 = hc.reconstruct(s)
    best = r0["res"]["best_it_f"]
    sets = np.concatenate([sets[:best + 1], sets[best:best + 1], sets[best + 1:]])  # the winner listed twice: the first wins
    r = check(frames, s, sets=sets)
    want = hc.reconstruct(s, sets=sets)
    assert np.isnan(want["score_h"][0]) or np.isnan(want["score_f"][0])
    assert r["best_it_f"] == best and r["ok"] == 1


def test_host_array_form_equals_the_resident_form(frames):
    s = ts.issue_scene(13, 300, False)
    upload(frames, s)
    rc1, b1 = raw_call(frames, s, hc.params_blob(), s["sets"], resident=True)
    rc2, b2 = raw_call(frames, s, hc.params_blob(), s["sets"], resident=False)
    assert rc1 == 0 and rc2 == 0
    for k in b1:
        assert b1[k].tobytes() == b2[k].tobytes(), k
    check(frames, s, resident=False)


def test_every_refusal_leaves_its_buffers_untouched(frames):
    s = ts.issue_scene(11, 100, False)
    upload(frames, s)
    N, n2 = s["n"], s["n2"]
    m12, sets, Kn, pb = s["matches12"], s["sets"][:4], s["K"].copy(), hc.params_blob()

    def edit(a, i, v):
        a = np.array(a, copy=True)
        a.reshape(-1)[i] = v
        return a
    first = int(np.nonzero(m12 >= 0)[0][0])
    few = np.full_like(m12, -1)
    few[np.nonzero(m12 >= 0)[0][:7]] = m12[np.nonzero(m12 >= 0)[0][:7]]
    Kn[1, 1] = np.nan
    cases = [dict(f1=None), dict(f2=None), dict(matches12=None), dict(K=None), dict(params=None), dict(sets=None), dict(res=False),
             dict(tri=False), dict(x3d=False), dict(matches12=edit(m12, first, n2)), dict(matches12=edit(m12, first, -2)),
             dict(matches12=few), dict(n_iter=0), dict(n_iter=1025, sets=np.resize(sets, (1025, 8))), dict(sets=edit(sets, 5, N)),
             dict(sets=edit(sets, 9, -1)), dict(sets=edit(sets, 3, sets[0, 0])), dict(K=Kn),
             dict(params=hc.params_blob(sigma=np.inf)), dict(params=hc.params_blob(sigma=0.0)), dict(params=hc.params_blob(sigma=-1.0))]
    for kw in cases:
        rc, b = raw_call(frames, s, pb, sets, **kw)
        assert rc == INVALID and untouched(b), kw.keys()
    for kw in (dict(xy1=None), dict(xy2=None), dict(matches12=edit(m12, first, n2)), dict(sets=edit(sets, 5, N))):
        rc, b = raw_call(frames, s, pb, sets, resident=False, **kw)
        assert rc == INVALID and untouched(b), kw.keys()
    check(frames, s, sets=sets)  # and the frames still serve a good call
