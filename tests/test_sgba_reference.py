"""Assertions on tests/sgba_reference.py ALONE (the NumPy restatement of Optimizer::LocalBundleAdjustment with planes and
rooms), for every scene of tests/sgba_scenes.py and every member of its perturbation set (8 edge orders and the +-1-ulp
libm): the branch distances stay above a stated margin, every member takes the same Levenberg decisions and sets the same
flags, the measured SPREAD covers every member, and each directed scene has the condition it was built for.  No edge is
excluded from any comparison; the code under test takes no part."""
import math

import numpy as np
import pytest

import lba_reference as lr
import lba_scenes as ls
import sgba_reference as sr
import sgba_scenes as ss

NAMES, BIG_NAMES = list(ss.scenes()), list(ss.big_scenes())
BRANCH_MARGIN, CHI2_MARGIN = 1e-8, 1e-3  # as the essential graph's test; relative for the chi2 thresholds
ALL = [(n, False) for n in NAMES] + [(n, True) for n in BIG_NAMES]


def decisions(r):
    return [[(good, ok2) for _, good, ok2 in tr] for tr in r["trace"]]


@pytest.mark.parametrize("name,big", ALL)
def test_fixture_condition(name, big):
    ref = ss.references(big)[name]
    members = [ref] + ss.perturbed_references(big)[name]
    spread = ss.SPREAD_BIG if big else ss.SPREAD
    for m in members:
        assert m["ran"] == ref["ran"]
        if not ref["ran"]:
            continue
        for key in ("seam", "pole", "dir", "fabs", "dist"):
            assert m["branch"][key] > BRANCH_MARGIN, (key, m["branch"][key])
        assert m["branch"]["chi2"] > CHI2_MARGIN, m["branch"]["chi2"]
        assert decisions(m) == decisions(ref)
        for k in ("stop_reason", "iterations_run", "trials_run", "n_rows", "n_erase", "n_erase_plane"):
            assert m[k] == ref[k], k
        assert (m["erase"] == ref["erase"]).all() and (m["erase_plane"] == ref["erase_plane"]).all()
        for k, v in ss.deviations(ref, m).items():
            assert v <= spread[k], (k, v)


def test_no_planes_no_rooms_is_the_visual_restatement():
    for name in ("kf_2_1", "special_vertices", "far_start"):
        s = ls.scenes()[name]
        a, b = sr.local_ba_sgraph(ss.no_sem(s)), lr.local_ba(s)
        assert decisions(a) == decisions(b) and (a["erase"] == b["erase"]).all()
        assert a["kf_out"].tobytes() == b["kf_out"].tobytes() and a["pos_out"].tobytes() == b["pos_out"].tobytes()
        assert a["chi2"].tobytes() == b["chi2"].tobytes() and a["n_rows"] == 6 * len(np.unique(s["obs_kf"][s["fixed"][s["obs_kf"]] == 0]))


def test_semantic_part_converges_and_moves_the_planes():
    for name in ("both", "corridor", "room4", "two_rooms_shared_wall"):
        ref, s = ss.references()[name], ss.scenes()[name]
        assert ref["chi2_final"] < 0.2 * ref["chi2_initial"] and all(good for tr in ref["trace"] for _, good, _ in tr)
        moved = np.abs(ref["plane_out"] - s["sem"]["plane_eq"]).max(1)
        assert (moved > 1e-3).all()  # started 1 cm / 0.5 degrees off
        assert np.abs(np.linalg.norm(ref["plane_out"][:, :3], axis=1) - 1).max() < 1e-12


def test_directed_scenes_have_their_condition():
    R = ss.references()
    r = R["fixed_only_plane"]
    assert r["n_planes_active"] == 2 and r["plane_out"][2].tobytes() == ss.scenes()["fixed_only_plane"]["sem"]["plane_eq"][2].tobytes()
    assert (r["plane_out"][1] != ss.scenes()["fixed_only_plane"]["sem"]["plane_eq"][1]).any()
    r, s = R["plane_only_kf"], ss.scenes()["plane_only_kf"]
    assert 2 not in s["obs_kf"] and not s["fixed"][2] and (r["kf_out"][2] != s["Tcw"][2].astype(np.float64)).any()
    assert r["n_rows"] == 6 * 4 + 3 * 2
    r = R["room_unobserved_walls"]
    assert r["n_planes_active"] == 5 and r["n_plane_kf"] == 3 and r["n_rows"] == 12 + 15 + 6
    r = R["two_rooms_shared_wall"]
    assert r["n_rooms_active"] == 2 and r["n_room_edges"] == 2 and r["n_rows"] == 12 + 15 + 12
    # every side of correctPlaneDirection and of fabs(d1) > fabs(d2) is taken in room_branches
    q = ss.scenes()["room_branches"]["sem"]
    signs, bigger = set(), set()
    for room, nw in enumerate(q["room_n_walls"]):
        w = q["plane_eq"][q["room_wall"][room, :nw]]
        for a, b in zip(w[0::2], w[1::2]):
            signs.update([bool(a[3] > 0), bool(b[3] > 0)]), bigger.add(bool(abs(a[3]) > abs(b[3])))
    assert signs == {True, False} and bigger == {True, False}
    r = R["classification"]
    assert list(r["erase_plane"][[0, 1, 2, 4, 6, 7, 9]]) == [0, 0, 0, 1, 1, 1, 1]
    assert r["chi2_pp"][4] > sr.TH_PP and r["chi2_pk"][4] < sr.TH_PK           # one edge flags, the other does not
    assert (r["chi2_pk"][6:8] < sr.TH_PK).all() and (r["chi2_pp"][6:8] < sr.TH_PP).all()  # isDistanceCorrect alone
    assert r["chi2_pk"][9] > sr.DELTA_3D ** 2 and r["chi2_pk"][9] > sr.TH_PK   # rho[1] < 1
    assert any(not good for tr in r["trace"] for _, good, _ in tr)              # a rejected trial
    assert R["rooms_only_edges"]["ran"] == 0 and R["iterations_1"]["iterations_run"] == 1
    assert R["edges_4"]["n_plane_point"] == 4 and R["edges_5"]["n_plane_point"] == 5
    B = ss.references(True)
    for n in (255, 256, 257):
        assert B["obs_%d" % n]["n_plane_point"] == n
    for n in (63, 64, 65):
        assert B["one_plane_%d" % n]["n_plane_point"] == n and B["one_plane_%d" % n]["n_planes_active"] == 1
    assert B["rows_768"]["n_rows"] == 768 and B["rows_768"]["n_planes_active"] == 54


def test_jitter_is_a_function_and_moves_by_an_ulp():
    jit = sr.scalar_jitter(3)
    vals = [math.atan2(0.3, k + 0.5) for k in range(200)]
    out = [jit(v) for v in vals]
    assert out == [jit(v) for v in vals] and jit(0.0) == 0.0 and jit(1.0) == 1.0
    steps = {round((o - v) / math.ulp(v)) for o, v in zip(out, vals)}
    assert steps == {-1, 0, 1}
