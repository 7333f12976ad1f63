"""The header's host build (csrc/vsg_essential_graph.h through tests/_egcore) against the restatement
(tests/eg_reference.py): decisions exactly, estimates and positions within eg_scenes.TOL = 16 x the restatement's own spread
over its perturbation set; the written-out log against libm; the 3 x 3 solve with partial pivoting; every argument error;
the edge-list builder of the adaptor against the restatement's walk."""
import math

import numpy as np
import pytest

import eg_hostcore as hc
import eg_reference as er
import eg_scenes as es

F32, F64, I32, U8 = np.float32, np.float64, np.int32, np.uint8
INVALID, UNSUPPORTED = -6, -3


@pytest.mark.parametrize("name", sorted(es.scenes()))
def test_host_build_matches_the_restatement(name):
    s, ref = es.scenes()[name], es.references()[name]
    got = hc.run(s)
    assert got["ret"] == 0
    assert es.decisions(got) == es.decisions(ref)
    dev = es.deviations(got, ref)
    for k, v in dev.items():
        assert v <= es.TOL[k], (k, v, es.TOL[k])
    # NaN sits where the restatement has it
    assert np.array_equal(np.isnan(got["kf_Scw"]), np.isnan(ref["kf_Scw"]))
    assert got["n_kf"] == len(s["fixed"]) and got["n_edges"] == len(s["ei"]) and got["n_points"] == len(s["slots"])
    assert got["n_fixed_kf"] == int(np.count_nonzero(s["fixed"]))
    if math.isfinite(ref["chi2_final"]):
        assert abs(got["chi2_final"] - ref["chi2_final"]) <= es.TOL["chi2_rel"] * max(1.0, abs(ref["chi2_final"]))
        assert abs(got["chi2_initial"] - ref["chi2_initial"]) <= 1e-9 * max(1.0, abs(ref["chi2_initial"]))
    # the store: listed slots hold the outs, every other slot its bytes
    store = np.array(s["store_pos"], F32)
    assert np.array_equal(got["store_pos"][s["slots"]].view(np.uint32), got["world_pos"].view(np.uint32))
    rest = np.setdiff1d(np.arange(s["capacity"]), s["slots"])
    assert np.array_equal(got["store_pos"][rest].view(np.uint32), store[rest].view(np.uint32))


def test_keyframes_that_are_no_vertex_keep_their_bytes():
    s = es.scenes()["kf_without_edge"]
    got = hc.run(s)
    assert got["kf_Scw"][4].tobytes() == np.asarray(s["Scw"], F64)[4].tobytes()
    assert got["kf_Scw"][0].tobytes() == np.asarray(s["Scw"], F64)[0].tobytes()  # fixed
    assert got["n_opt_kf"] == 8


def test_fix_scale_keeps_every_scale():
    for name in ("loop_fix1_s1", "loop_fix1_s13"):
        s = es.scenes()[name]
        assert np.array_equal(hc.run(s)["kf_Scw"][:, 7], np.asarray(s["Scw"], F64)[:, 7])


def test_no_edges_runs_nothing_and_returns_the_inputs():
    s = dict(es.scenes()["loop_fix0_s1"])
    s["ei"], s["ej"], s["eloop"] = np.zeros(0, I32), np.zeros(0, I32), np.zeros(0, U8)
    got = hc.run(s)
    assert got["ret"] == 0 and got["ran"] == 0 and got["n_opt_kf"] == 0
    assert got["kf_Scw"].tobytes() == np.asarray(s["Scw"], F64).tobytes()
    assert (got["world_pos"] == hc.SENT).all() and got["store_pos"].tobytes() == np.asarray(s["store_pos"], F32).tobytes()


def test_pose_graph_alone_without_a_store():
    s = dict(es.scenes()["loop_fix0_s13"])
    full = hc.run(s)
    s["slots"], s["point_ref"], s["store_pos"] = np.zeros(0, I32), np.zeros(0, I32), None
    got = hc.run(s)
    assert got["ret"] == 0 and got["kf_Scw"].tobytes() == full["kf_Scw"].tobytes() and got["chi2"].tobytes() == full["chi2"].tobytes()


def test_written_out_log_against_libm():
    rng = np.random.default_rng(11)
    x = np.concatenate([np.exp(rng.uniform(-1e-8, 1e-8, 4000)), np.exp(rng.uniform(-1, 1, 20000)), np.exp(rng.uniform(-30, 30, 4000)),
                        [1.0, 2.0, 0.5, 1.3, 1.0 / 1.3, np.nextafter(1.0, 2.0), np.nextafter(1.0, 0.0), 2.2250738585072014e-308, 1e308]])
    got, want = hc.dlog(x), np.log(x)
    ulp = np.spacing(np.abs(want))
    assert (np.abs(got - want) <= ulp).all()
    assert hc.dlog([1.0])[0] == 0.0
    near = np.abs(x - 1) < 1e-7
    assert np.array_equal(got[near], want[near])  # what sigma of a near-consistent edge sees
    bad = hc.dlog([0.0, -1.0, np.inf, np.nan, 4.9e-324])
    assert np.isnan(bad).all()


def test_pivoting_solve_on_a_matrix_that_needs_a_row_swap():
    for W in ([[0.0, 2.0, 1.0], [1.0, 1.0, 1.0], [4.0, -1.0, 3.0]],      # zero leading entry: no elimination without a swap
              [[1e-20, 1.0, 0.0], [1.0, 1.0, 0.0], [0.0, 0.0, 1.0]],      # a tiny pivot an unpivoted sweep would keep
              [[2.0, 1.0, 0.0], [4.0, 2.0, 1.0], [1.0, 3.0, 5.0]]):       # second column: zero pivot after the first step
        W, t = np.array(W), np.array([1.0, -2.0, 0.5])
        x = hc.lu3(W, t)
        assert np.abs(x - np.linalg.solve(W, t)).max() < 1e-12, (W, x)
    x = hc.lu3(np.array([[1e-20, 1.0, 0.0], [1.0, 1.0, 0.0], [0.0, 0.0, 1.0]]), np.array([1.0, 2.0, 3.0]))
    assert abs(x[0] - 1.0) < 1e-12 and abs(x[1] - 1.0) < 1e-12  # without the swap x[0] would be 0


def test_sim3_log_in_every_branch_against_the_restatement():
    rng = np.random.default_rng(12)
    for theta, sigma in ((1e-7, 1e-7), (0.3, 1e-7), (1e-7, 0.2), (0.4, -0.3), (2.5, 0.1)):
        ax = rng.normal(size=3)
        S = er.pack(er.s_exp(np.concatenate([theta * ax / np.linalg.norm(ax), rng.normal(size=3), [sigma]])))
        want = er.s_log(tuple(a[None] for a in er.sim3(S)), er.Trace())[0]
        assert np.abs(hc.sim3_log(S) - want).max() < 1e-12


def error_cases():
    """name -> (scene overrides / run keywords, expected code).  Shared with the ABI and GPU tests."""
    base = es.scenes()["loop_fix0_s1"]
    K, E, P = len(base["fixed"]), len(base["ei"]), len(base["slots"])

    def sim3_with(arr, k, col, v):
        a = np.array(base[arr], F64)
        a[k, col] = v
        return {arr: a}

    def edge_with(arr, e, v):
        a = np.array(base[arr], I32)
        a[e] = v
        return {arr: a}
    twice = np.array(base["slots"], I32)
    twice[3] = twice[9]
    cases = {
        "null_Scw": (dict(null=("Scw",)), INVALID), "null_has": (dict(null=("has",)), INVALID), "null_fixed": (dict(null=("fixed",)), INVALID),
        "null_nonc_with_entry": (dict(null=("nonc",)), INVALID), "null_edge_i": (dict(null=("ei",)), INVALID),
        "null_edge_j": (dict(null=("ej",)), INVALID), "null_edge_loop": (dict(null=("el",)), INVALID),
        "null_slots": (dict(null=("slots",)), INVALID), "null_point_ref": (dict(null=("ref",)), INVALID),
        "null_store_with_points": (dict(null=("store",)), INVALID), "null_kf_out": (dict(null=("kf_out",)), INVALID),
        "null_res": (dict(null=("res",)), INVALID),
        "negative_n_kf": (dict(n_kf=-1), INVALID), "negative_n_edges": (dict(n_edges=-1), INVALID),
        "negative_n_points": (dict(n_points=-1), INVALID),
        "edge_i_negative": (edge_with("ei", 2, -1), INVALID), "edge_i_past_end": (edge_with("ei", 2, K), INVALID),
        "edge_j_negative": (edge_with("ej", 5, -1), INVALID), "edge_j_past_end": (edge_with("ej", 5, K), INVALID),
        "edge_self": (edge_with("ej", 0, int(base["ei"][0])), INVALID),
        "slot_negative": (dict(slots=np.where(np.arange(P) == 4, -1, base["slots"]).astype(I32)), INVALID),
        "slot_past_end": (dict(slots=np.where(np.arange(P) == 4, base["capacity"], base["slots"]).astype(I32)), INVALID),
        "slot_twice": (dict(slots=twice), INVALID),
        "ref_negative": (dict(point_ref=np.where(np.arange(P) == 1, -1, base["point_ref"]).astype(I32)), INVALID),
        "ref_past_end": (dict(point_ref=np.where(np.arange(P) == 1, K, base["point_ref"]).astype(I32)), INVALID),
        "Scw_nan": (sim3_with("Scw", 3, 1, np.nan), INVALID), "Scw_inf": (sim3_with("Scw", 3, 5, np.inf), INVALID),
        "Scw_scale_zero": (sim3_with("Scw", 6, 7, 0.0), INVALID), "Scw_scale_negative": (sim3_with("Scw", 6, 7, -1.0), INVALID),
        "Scw_scale_nan": (sim3_with("Scw", 6, 7, np.nan), INVALID),
        "nonc_nan_on_entry": (sim3_with("nonc", K - 1, 4, np.nan), INVALID), "nonc_scale_zero_on_entry": (sim3_with("nonc", K - 1, 7, 0.0), INVALID),
        "fix_scale_2": (dict(fix_scale=2), INVALID), "fix_scale_negative": (dict(fix_scale=-1), INVALID),
        "iterations_0": (dict(iterations=0), INVALID), "iterations_101": (dict(iterations=101), INVALID),
    }
    return base, cases


@pytest.mark.parametrize("case", sorted(error_cases()[1]))
def test_argument_error_returns_its_code_and_writes_nothing(case):
    base, cases = error_cases()
    kw, code = cases[case]
    run_kw = {k: v for k, v in kw.items() if k in ("null", "n_kf", "n_edges", "n_points")}
    s = dict(base, **{k: v for k, v in kw.items() if k not in run_kw})
    got = hc.run(s, **run_kw)
    assert got["ret"] == code
    assert (got["kf_Scw"] == hc.SENT).all() and (got["world_pos"] == hc.SENT).all() and (got["chi2"] == hc.SENT).all()
    assert got["res_untouched"]
    assert got["store_pos"].tobytes() == np.asarray(base["store_pos"], F32).tobytes()


def test_a_non_finite_entry_of_non_corrected_without_its_flag_is_not_read():
    base = es.scenes()["loop_fix0_s1"]
    a = np.array(base["nonc"], F64)
    a[0] = np.nan  # keyframe 0 has no entry
    assert hc.run(dict(base, nonc=a))["kf_Scw"].tobytes() == hc.run(base)["kf_Scw"].tobytes()


def _chain(n_opt):
    K = n_opt + 1
    Scw = np.zeros((K, 8))
    Scw[:, 3] = Scw[:, 7] = 1.0
    fixed = np.zeros(K, U8)
    fixed[0] = 1
    return dict(Scw=Scw, nonc=Scw.copy(), has=np.zeros(K, U8), fixed=fixed, ei=np.arange(1, K, dtype=I32), ej=np.arange(0, K - 1, dtype=I32),
                eloop=np.zeros(K - 1, U8), fix_scale=0, iterations=1, slots=np.zeros(0, I32), point_ref=np.zeros(0, I32), store_pos=None)


def test_cap_is_438_optimised_keyframes():
    got = hc.run(_chain(439))
    assert got["ret"] == UNSUPPORTED and got["res_untouched"] and (got["kf_Scw"] == hc.SENT).all()


def test_correct_sim3_is_the_point_correction_of_the_call():
    s = es.scenes()["loop_fix0_s13"]
    full = hc.run(s)
    inv = er.pack(er.s_inv(er.sim3(full["kf_Scw"])))
    got = hc.correct(s["store_pos"], s["slots"], s["point_ref"], s["Scw"], inv)
    want = er.correct_points(s["Scw"], full["kf_Scw"], s["point_ref"], np.asarray(s["store_pos"], F32)[s["slots"]])
    assert got["ret"] == 0 and np.abs(got["world_pos"].astype(F64) - want.astype(F64)).max() <= es.TOL["pos"]
    # the call inverts the estimate itself (sim3_inverse); the restatement's inverse may differ by a rounding
    assert np.abs(got["world_pos"].astype(F64) - full["world_pos"].astype(F64)).max() <= 4 * 2.0 ** -21
    for kw, bad in ((dict(null=("slots",)), None), (dict(null=("ref",)), None), (dict(null=("from",)), None), (dict(null=("to",)), None),
                    ({}, "slot"), ({}, "ref"), ({}, "scale")):
        sl, ref, to = np.array(s["slots"], I32), np.array(s["point_ref"], I32), inv.copy()
        if bad == "slot":
            sl[2] = sl[5]
        if bad == "ref":
            ref[0] = len(s["fixed"])
        if bad == "scale":
            to[1, 7] = 0.0
        r = hc.correct(s["store_pos"], sl, ref, s["Scw"], to, **kw)
        assert r["ret"] == INVALID and (r["world_pos"] == hc.SENT).all()
        assert r["store_pos"].tobytes() == np.asarray(s["store_pos"], F32).tobytes()


@pytest.mark.parametrize("name", [n for n, s in sorted(es.scenes().items()) if s["graph"] is not None])
def test_adaptor_builds_the_edge_list_of_the_reference_walk(name):
    s = es.scenes()[name]
    ei, ej, el = hc.edges(s["graph"])
    assert np.array_equal(ei, s["ei"]) and np.array_equal(ej, s["ej"]) and np.array_equal(el, s["eloop"])


def test_adaptor_builder_skips_bad_keyframes_and_inserted_pairs():
    g = es.graph(12, 11, 1)
    g["covisibles"][6] = [-1, 5, 4, 3]        # a bad keyframe among the covisibles
    g["covisibles"][11] = [10, 9, 2, 1]       # 2 and 1 are loop connections of 11: in sInsertedEdges
    g["loop_connections"][0][1].append((-1, 500))
    want = er.build_edges(g["parent"], g["loops"], g["children"], g["covisibles"], g["loop_connections"], g["cur"], g["loop_kf"])
    got = hc.edges(g)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    normal = [(i, j) for i, j, l in zip(*got) if not l]
    assert (11, 2) not in normal and (11, 1) not in normal and (11, 9) in normal
