"""The host build of csrc/vsg_global_ba.h (tests/_gbacore) against the restatement (tests/gba_reference.py): every scene
within the measured tolerance of gba_scenes.py with all counters, the stop reason and `included` equal and no edge or point
left out; the blocked reduced solve against lba::solve_reduced_host bit for bit; the returns before optimize; every argument
error with nothing written."""
import numpy as np
import pytest

import gba_hostcore as hc
import gba_scenes as gs
import lba_scenes as ls

NAMES = list(gs.scenes())
INVALID, UNSUPPORTED = -6, -3


def check_against_reference(name, got):
    """got: a result in gba_hostcore.result's form (the host build's or the device's)."""
    s, ref = gs.scenes()[name], gs.references()[name]
    assert got["ret"] == 0 and got["ran"] == 1
    for k in ("n_opt_kf", "n_fixed_kf", "n_points", "n_edges", "n_mono", "n_stereo", "iterations_run", "trials_run", "stop_reason"):
        assert got[k] == ref[k], k
    assert (got["included"] == ref["included"]).all()
    assert len(got["chi2"]) == ref["n_edges"] and len(got["pos_out"]) == ref["n_points"]
    for k, v in gs.deviations(ref, got).items():
        assert v <= gs.TOL[k], (k, v)
    for k in ("lambda", "chi2_initial", "chi2_final"):
        assert abs(got[k] - ref[k]) <= gs.TOL["chi2_rel"] * max(abs(ref[k]), 1e-6), k
    check_store(s, got)


def check_store(s, got):
    """write_store = 1: the included points' slots hold the outs and everything else keeps its bytes; 0: every byte is kept."""
    expect = s["store_pos"].copy()
    if s["write_store"]:
        vertex = np.diff(s["obs_off"]) > 0
        expect[s["slots"][vertex]] = got["pos_out"][vertex]
    assert expect.tobytes() == got["store_pos"].tobytes()


@pytest.mark.parametrize("name", NAMES)
def test_scene(name):
    check_against_reference(name, hc.run(gs.scenes()[name]))


def test_geometry_is_the_scenes():
    panel, tile, cap = hc.geometry()
    assert (panel, tile) == (gs.PANEL, gs.TILE) and cap >= 512 and panel % 6 == 0


def test_robust_and_write_store_arguments():
    s = gs.scenes()["mixed_robust_20"]
    on, off = hc.run(s), hc.run(s, robust=0)
    assert on["chi2_initial"] < off["chi2_initial"] and not np.array_equal(on["kf_out"], off["kf_out"])
    kept, written = hc.run(s, write_store=0), hc.run(s, write_store=1)
    assert kept["pos_out"].tobytes() == written["pos_out"].tobytes() and kept["res_bytes"] == written["res_bytes"]
    assert kept["store_pos"].tobytes() == s["store_pos"].tobytes() != written["store_pos"].tobytes()


def test_mono_delta_is_5_99_not_5_991():
    """This call's monocular delta is the float sqrt(5.99); the local call's is sqrt(5.991).  The scenes with outliers hold
    edges far beyond both, so test_scene could not tell them apart: here one edge's chi2 lies between the two squares."""
    d_global, d_local = gs.gr.DELTA[0], ls.lr.DELTA[0]
    assert d_global ** 2 < 5.9905 < d_local ** 2
    s = dict(gs.scenes()["initialisation"])
    g = gs.gr.Graph(s)
    _, _, _, chi2 = g.errors(g.est, g.X)
    e = int(np.argmax(chi2))                       # scale that edge's information so that its chi2 is 5.9905
    k, i = int(s["obs_kf"][e]), int(s["obs_idx"][e])
    level = 7
    kfs = [dict(f) for f in s["kfs"]]
    kfs[k] = dict(kfs[k], octave=kfs[k]["octave"].copy())
    kfs[k]["octave"][i] = level
    sig = s["sig"].copy()
    sig[level] = np.float32(5.9905 / (chi2[e] / g.w[e]))
    s.update(kfs=kfs, sig=sig, iterations=1)
    ref, got = gs.gr.global_ba(s), hc.run(s)
    c = float(sig[level]) * (chi2[e] / g.w[e])
    assert d_global ** 2 < c < d_local ** 2
    plain = hc.run(s, robust=0)
    assert plain["chi2_initial"] - got["chi2_initial"] > 0                      # that edge is an outlier of THIS kernel
    assert abs(got["chi2_initial"] - ref["chi2_initial"]) <= gs.TOL["chi2_rel"] * ref["chi2_initial"]


# ---- the blocked reduced solve

def solver_sizes(panel, tile):
    return [1, 5, 6, panel - 1, panel, panel + 1, 2 * panel, 3 * panel + 6, tile + 1, panel + tile + 2]


def spd(n, seed):
    rng = np.random.default_rng(seed)
    A = rng.normal(0, 1, (n, n))
    return A @ A.T + n * np.eye(n), rng.normal(0, 1, n)


def bad_pivot_systems(panel):
    """(M, b) with a non-positive pivot in the first column, inside a panel and in the last column."""
    n = 2 * panel + 6
    out = []
    for col in (0, panel + panel // 2, n - 1):
        M, b = spd(n, 77 + col)
        M[col, col] = -1.0 if col == 0 else -abs(M[col, col])
        out.append((M, b))
    return out


def solver_cases(panel, tile):
    """name -> (M, b, whether x is compared); shared with the device test."""
    cases = {"n_%d" % n: spd(n, 100 + n) + (True,) for n in solver_sizes(panel, tile)}
    for k, (M, b) in enumerate(bad_pivot_systems(panel)):
        cases["bad_pivot_%d" % k] = (M, b, False)
    return cases


@pytest.mark.parametrize("case", list(solver_cases(gs.PANEL, gs.TILE)))
def test_blocked_solve_equals_the_plain_sweep_bit_for_bit(case):
    panel, tile, _ = hc.geometry()
    M, b, compare_x = solver_cases(panel, tile)[case]
    ok_plain, x_plain = hc.solve(M, b, blocked=False)
    ok_blocked, x_blocked = hc.solve(M, b, blocked=True)
    assert ok_plain == ok_blocked == int(compare_x)
    if compare_x:
        assert x_plain.tobytes() == x_blocked.tobytes()
        assert np.allclose(M @ x_plain, b, rtol=0, atol=1e-9 * len(b))


# ---- arguments

def untouched(s, got):
    return (got["kf_out"] == hc.SENTINEL_F).all() and (got["pos_out"] == hc.SENTINEL_F).all() and \
        (got["included"] == hc.SENTINEL_INCLUDED).all() and (got["chi2"] == hc.SENTINEL_F).all() and \
        got["store_pos"].tobytes() == np.ascontiguousarray(s["store_pos"], np.float32).tobytes() and \
        got["res_bytes"] == b"\x5a" * len(got["res_bytes"])


def error_cases():
    """name -> (overrides / arguments of gba_hostcore.run, the expected return code); shared with the device test."""
    s = gs.scenes()["mixed_robust_0"]
    E, P, K = int(s["obs_off"][-1]), len(s["slots"]), len(s["kfs"])

    def put(key, i, v):
        a = s[key].copy()
        a[i] = v
        return {key: a}
    twice = s["slots"].copy()
    twice[5] = twice[2]
    deep = [dict(f) for f in s["kfs"]]
    deep[1] = dict(deep[1], octave=deep[1]["octave"].copy())
    deep[1]["octave"][int(s["obs_idx"][np.flatnonzero(s["obs_kf"] == 1)[0]])] = s["nlevels"]
    nleft = np.full(K, -1, np.int32)
    nleft[1] = 3
    cases = {
        "null_slots": (dict(null=("slots",)), INVALID), "null_obs_off": (dict(null=("obs_off",)), INVALID),
        "null_obs_kf": (dict(null=("obs_kf",)), INVALID), "null_obs_idx": (dict(null=("obs_idx",)), INVALID),
        "null_Tcw": (dict(null=("kf_Tcw",)), INVALID), "null_fixed": (dict(null=("kf_fixed",)), INVALID),
        "null_cam": (dict(null=("kf_cam",)), INVALID), "null_sigma": (dict(null=("inv_level_sigma2",)), INVALID),
        "null_kf_out": (dict(null=("kf_Tcw_out",)), INVALID), "null_included": (dict(null=("included",)), INVALID),
        "null_res": (dict(null=("res",)), INVALID),
        "null_pos_out_without_write_store": (dict(null=("world_pos_out",), write_store=0), INVALID),
        "off_not_from_zero": (put("obs_off", 0, 1), INVALID), "off_descends": (put("obs_off", 3, int(s["obs_off"][2]) - 1), INVALID),
        "kf_negative": (put("obs_kf", 4, -1), INVALID), "kf_past_end": (put("obs_kf", 4, K), INVALID),
        "idx_negative": (put("obs_idx", E - 1, -1), INVALID),
        "idx_past_end": (put("obs_idx", 0, len(s["kfs"][int(s["obs_kf"][0])]["x"])), INVALID),
        "slot_negative": (put("slots", 1, -1), INVALID), "slot_past_end": (put("slots", P - 1, s["capacity"]), INVALID),
        "slot_twice": (dict(slots=twice), INVALID),
        "nlevels_0": (dict(nlevels=0), INVALID), "nlevels_17": (dict(nlevels=17), INVALID),
        "octave_past_nlevels": (dict(kfs=deep), INVALID),
        "iterations_0": (dict(iterations=0), INVALID), "iterations_101": (dict(iterations=101), INVALID),
        "robust_2": (dict(robust=2), INVALID), "robust_negative": (dict(robust=-1), INVALID),
        "write_store_2": (dict(write_store=2), INVALID), "write_store_negative": (dict(write_store=-1), INVALID),
        "nleft": (dict(nleft=nleft), UNSUPPORTED),
        "edges_on_fixed_alone": (dict(fixed=np.ones(K, np.uint8)), UNSUPPORTED),
    }
    return s, cases


@pytest.mark.parametrize("case", list(error_cases()[1]))
def test_argument_error(case):
    s, cases = error_cases()
    kw, code = cases[case]
    scene_over = {k: v for k, v in kw.items() if k not in ("null", "nleft")}
    got = hc.run(s, null=kw.get("null", ()), nleft=kw.get("nleft"), **scene_over)
    assert got["ret"] == code
    if "null" not in kw:
        assert untouched(dict(s, **scene_over), got)


def test_null_pos_out_is_fine_with_write_store():
    s = gs.scenes()["mixed_robust_0"]
    got, full = hc.run(s, null=("world_pos_out",), write_store=1), hc.run(s, write_store=1)
    assert got["ret"] == 0 and got["store_pos"].tobytes() == full["store_pos"].tobytes() and got["res_bytes"] == full["res_bytes"]


def over_cap_scene():
    """One point seen by cap + 1 optimised keyframes of two features each, and one fixed keyframe: the cap is decided on the
    lists alone.  Shared with the device test."""
    cap = hc.geometry()[2]
    K = cap + 2
    f = dict(x=np.array([10, 20], np.float32), y=np.array([10, 20], np.float32), octave=np.zeros(2, np.int32), ur=None)
    return dict(kfs=[f] * K, Tcw=np.tile(np.array([0, 0, 0, 1, 0, 0, 0], np.float32), (K, 1)), fixed=np.eye(1, K, 0, np.uint8)[0],
                cam=np.tile(np.array(ls.TUM1, np.float32), (K, 1)), sig=ls.INV_SIGMA2, nlevels=ls.NLEVELS, iterations=10, capacity=16,
                store_pos=np.ones((16, 3), np.float32), slots=np.array([3], np.int32), obs_off=np.array([0, K], np.int32),
                obs_kf=np.arange(K, dtype=np.int32), obs_idx=np.zeros(K, np.int32), robust=0, write_store=0)


def test_more_optimised_keyframes_than_the_cap():
    many = over_cap_scene()
    K = len(many["kfs"])
    got = hc.run(many)
    assert got["ret"] == UNSUPPORTED and untouched(many, got)
    at_cap = dict(many, obs_off=np.array([0, K - 1], np.int32))   # cap optimised keyframes with an edge: not refused for its size
    assert hc.run(at_cap, stop_flag=1)["ret"] == 0


@pytest.mark.parametrize("name,after", [("rows_54", 1), ("rows_54", 3), ("kf_129", 2), ("mixed_robust_20", 9)])
def test_stop_flag_set_between_iterations(name, after):
    """The flag lands at the look behind iteration `after`, as a second thread's store would: the run ends there with
    stop_reason 3, and its outs are those of a run asked for that many iterations."""
    s = gs.scenes()[name]
    full = hc.run(s, stop_flag=0)
    assert full["iterations_run"] > after and full["res_bytes"] == hc.run(s)["res_bytes"]
    got, want = hc.run(s, stop_flag=0, stop_after=after), hc.run(s, iterations=after)
    assert got["ret"] == 0 and got["ran"] == 1 and got["stop_reason"] == 3 and got["iterations_run"] == after
    assert want["stop_reason"] == 0 and want["iterations_run"] == after
    for k in ("kf_out", "pos_out", "included", "chi2", "store_pos"):
        assert got[k].tobytes() == want[k].tobytes(), k
    for k in hc.RES_INTS + hc.RES_DOUBLES:
        assert k == "stop_reason" or got[k] == want[k], k


def test_stop_flag_at_the_last_look_changes_nothing():
    """A flag that lands when the run has already finished (the iterations are done, or _nBad >= 3) is not looked at."""
    s = gs.scenes()["rows_54"]
    full = hc.run(s)
    assert hc.run(s, stop_flag=0, stop_after=full["iterations_run"])["res_bytes"] == full["res_bytes"]


def test_returns_before_optimize():
    s = gs.scenes()["mixed_robust_0"]
    K = len(s["kfs"])
    empty = dict(slots=s["slots"][:0], obs_off=np.zeros(1, np.int32), obs_kf=s["obs_kf"][:0], obs_idx=s["obs_idx"][:0])
    for kw, over in ((dict(stop_flag=1), {}), ({}, dict(obs_off=np.zeros_like(s["obs_off"]))), ({}, empty)):
        got = hc.run(s, **kw, **over)
        s2 = dict(s, **over)
        assert got["ret"] == 0 and got["ran"] == 0 and got["iterations_run"] == 0
        # only res and included are written
        assert (got["kf_out"] == hc.SENTINEL_F).all() and (got["pos_out"] == hc.SENTINEL_F).all() and (got["chi2"] == hc.SENTINEL_F).all()
        assert got["store_pos"].tobytes() == s["store_pos"].tobytes()
        assert (got["included"] == (np.diff(s2["obs_off"]) > 0)).all()
    # no fixed keyframe is NO reason to return
    got = hc.run(s, fixed=np.zeros(K, np.uint8))
    assert got["ret"] == 0 and got["ran"] == 1 and got["n_fixed_kf"] == 0 and got["n_opt_kf"] == K
    assert hc.run(s, stop_flag=0)["res_bytes"] == hc.run(s)["res_bytes"]


def test_iterations_argument():
    s = gs.scenes()["rows_54"]
    one, ten = hc.run(s, iterations=1), hc.run(s)
    assert one["iterations_run"] == 1 and one["stop_reason"] == 0 and ten["iterations_run"] > 1
    assert one["chi2_initial"] == ten["chi2_initial"] and one["chi2_final"] > ten["chi2_final"]


def test_host_build_equals_the_local_call_s_host_build_bit_for_bit():
    """On a scene both calls accept, started so near its solution that both Huber kernels are the identity, the two host
    builds differ in the reduced solve's schedule alone: blocked against lba::solve_reduced_host inside the whole loop."""
    import lba_hostcore as lhc
    s = gs._with(ls.make(861, 9, 1, 80, 5, start=(0.0005, 0.02)), 1, 1)
    got, want = hc.run(s), lhc.run(s)
    assert got["ret"] == want["ret"] == 0 and got["iterations_run"] == want["iterations_run"] >= 2
    assert want["chi2"].max() < 5.0 and want["erase"].sum() == 0
    for k in ("kf_out", "pos_out", "chi2", "store_pos"):
        assert got[k].tobytes() == want[k].tobytes(), k
    for k in hc.RES_INTS + hc.RES_DOUBLES:
        assert got[k] == want[k], k
