"""The restatement of Optimizer::OptimizeEssentialGraph (tests/eg_reference.py) on its own: the fixture conditions every
other essential-graph test rests on, asserted for every scene and every member of its perturbation set, and the committed
tolerance against a fresh measurement."""
import numpy as np
import pytest

import eg_reference as er
import eg_scenes as es


def _all_runs():
    for name, ref in es.references().items():
        yield name, "reference", ref
        for m, p in enumerate(es.perturbed_references()[name]):
            yield name, "member %d" % m, p


def test_no_evaluation_comes_near_a_branch_of_log():
    """Over every error evaluation of every run, d stays away from 1 - 1e-5 and |sigma| from 1e-5 by more than 1e-8: a
    perturbation of 1e-9 never straddles a branch, so the numeric Jacobian differentiates one formula."""
    for name, who, r in _all_runs():
        assert r["ran"] == 1, (name, who)
        assert r["min_d_dist"] > 1e-8 and r["min_sigma_dist"] > 1e-8, (name, who, r["min_d_dist"], r["min_sigma_dist"])


def test_every_member_of_the_perturbation_set_takes_the_same_decisions():
    """Accepted trials, stop reason, iteration and trial counts: the scenes are chosen so that rounding does not decide them."""
    for name, who, r in _all_runs():
        assert es.decisions(r) == es.decisions(es.references()[name]), (name, who)


def test_committed_spread_bounds_the_measured_one():
    """eg_scenes.SPREAD is the measured spread as committed: a fresh measurement may differ with another NumPy / libm (the
    quantity is rounding noise amplified by 5e8), so it is bounded from both sides by a factor 4, not compared for equality."""
    spread, _ = es.measure()
    for k, v in spread.items():
        m = max(v, 2.0 ** -52)
        assert m <= 4 * es.SPREAD[k] and es.SPREAD[k] <= 4 * m, (k, v, es.SPREAD[k])
        assert es.TOL[k] == 16 * es.SPREAD[k]


def test_scenes_cover_what_they_claim():
    sc, refs = es.scenes(), es.references()
    assert {(s["fix_scale"], round(float(s["Scw"][-1, 7]), 1)) for n, s in sc.items() if n.startswith("loop_")} == \
        {(0, 1.0), (0, 1.3), (1, 1.0), (1, 1.3)}
    iso = sc["kf_without_edge"]
    assert 4 not in set(iso["ei"]) | set(iso["ej"]) and np.array_equal(refs["kf_without_edge"]["kf_Scw"][4], iso["Scw"][4])
    assert not sc["no_fixed_kf"]["fixed"].any() and not any(refs["no_fixed_kf"]["accepted"])
    dup = sc["duplicate_pair"]
    pairs = [tuple(sorted(p)) for p in zip(dup["ei"].tolist(), dup["ej"].tolist())]
    assert pairs.count((4, 5)) == 3
    ff = sc["fixed_fixed_edge"]
    assert any(ff["fixed"][i] and ff["fixed"][j] for i, j in zip(ff["ei"], ff["ej"]))
    assert np.array_equal(refs["fixed_fixed_edge"]["kf_Scw"][:2], ff["Scw"][:2])
    nan = refs["nan_estimate"]
    assert not any(nan["accepted"]) and not np.isfinite(nan["chi2_final"])


def test_log_branches_scene_starts_one_edge_in_each_branch():
    s = es.scenes()["log_branches"]
    meas = er.measurements(s["Scw"], s["nonc"], s["has"], s["ei"], s["ej"], s["eloop"])
    V = er.sim3(s["Scw"])
    err = er.edge_error(meas, er.take(V, s["ei"]), er.take(V, s["ej"]), er.Trace())
    sigma, theta = err[:, 6], np.linalg.norm(err[:, :3], axis=1)
    d = np.cos(theta)
    assert [(abs(x) < 1e-5, y > 1 - 1e-5) for x, y in zip(sigma, d)] == [(True, True), (True, False), (False, True), (False, False)]


def test_exp_and_log_are_inverse_in_every_branch():
    rng = np.random.default_rng(5)
    for theta, sigma in ((1e-7, 1e-7), (0.3, 1e-7), (1e-7, 0.2), (0.4, -0.3), (2.5, 0.1)):
        ax = rng.normal(size=3)
        u = np.concatenate([theta * ax / np.linalg.norm(ax), rng.normal(size=3), [sigma]])
        S = er.s_exp(u)
        back = er.s_log(tuple(np.asarray(a)[None] for a in S), er.Trace())[0]
        assert np.abs(back - u).max() < 1e-9, (theta, sigma, back, u)


def test_builder_walk_applies_the_filters():
    g = es.graph(12, 11, 1)
    ei, ej, el = er.build_edges(g["parent"], g["loops"], g["children"], g["covisibles"], g["loop_connections"], g["cur"], g["loop_kf"])
    loop = [(i, j) for i, j, l in zip(ei, ej, el) if l]
    assert loop == [(11, 1), (11, 2), (10, 1)]  # :2542: weight 30 kept for the pair itself, weight 50 dropped
    normal = [(i, j) for i, j, l in zip(ei, ej, el) if not l]
    assert (7, 2) in normal and (2, 7) not in normal  # :2608
    assert all(j < i for i, j in normal)
    assert (5, 4) in normal and normal.count((5, 4)) == 1  # the parent comes from the spanning tree alone
    assert (5, 6) not in normal  # a child
    assert (5, 3) in normal and (5, 2) in normal


@pytest.mark.parametrize("solver", ["ldlt", "numpy"])
def test_solvers_agree_on_a_positive_definite_system(solver):
    rng = np.random.default_rng(3)
    A = rng.normal(size=(14, 14))
    A = A @ A.T + 14 * np.eye(14)
    b = rng.normal(size=14)
    x, ok = (er.ldlt_solve if solver == "ldlt" else er.numpy_solve)(A, b)
    assert ok and np.abs(A @ x - b).max() < 1e-10
    x, ok = (er.ldlt_solve if solver == "ldlt" else er.numpy_solve)(A - 40 * np.eye(14), b)
    assert not ok
