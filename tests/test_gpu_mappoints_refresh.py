"""vsg_mappoints_refresh_from_observations on the GPU: MapPoint::ComputeDistinctiveDescriptors and UpdateNormalAndDepth of
resident map points from their observation lists, against tests/observations_reference.py (the NumPy float32 restatement and
the oracle's distinctive descriptor), byte for byte over the WHOLE store: the listed slots hold the restatement's values,
every other slot and every field `what` does not name hold what they held.  Scenes: tests/refresh_scenes.py."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import frustum_reference as fr
import obs_cases as oc
import observations_reference as obr
import projection_scenes as ps
import refresh_scenes as rs
from visual_sgraphs_amd import orb

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
ADAPTOR = ROOT / "tests" / "_adaptor_refresh"
FIELDS = ("world_pos", "normal", "min_dist", "max_dist", "desc", "observed")
CAP = 1000


def upload(frames):
    return [orb.Frame(len(k) + 1).upload(k, d, rs.BOUNDS) for k, d in frames]


def store_of(fields):
    mp = orb.MapPoints(len(fields["desc"]))
    mp.update(np.arange(len(fields["desc"])), **{k: fields[k] for k in FIELDS})
    return mp


def whole(mp):
    return mp.read(np.arange(mp.capacity))


def call(mp, prob, F, what=3):
    return mp.refresh(prob["slots"], prob["off"], prob["kf"], prob["idx"], prob["ref_pos"], [F[f] for f in prob["table"]],
                      prob["Ow"], prob["scale_factors"], obs_bad=prob["bad"], what=what)


def same_store(got, want):
    for k in FIELDS:
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k]).reshape(np.shape(got[k]))
        assert g.tobytes() == w.tobytes(), (k, np.flatnonzero((g != w).reshape(len(g), -1).any(axis=1))[:8])


def same_outs(got, want):
    assert np.array_equal(got["best"], want["best"]), np.flatnonzero(got["best"] != want["best"])[:8]
    for k in ("normal", "min_dist", "max_dist"):
        assert np.ascontiguousarray(got[k]).tobytes() == np.ascontiguousarray(want[k], np.float32).tobytes(), k


def run_and_compare(mp, prob, F, what=3):
    before = whole(mp)
    want, want_outs = obr.refresh(before, prob, what)
    outs = call(mp, prob, F, what)
    same_store(whole(mp), want)
    same_outs(outs, want_outs)
    return before, want, outs


@pytest.fixture(scope="module")
def main_scene():
    """The scene, its frames on the device and the restatement for what = 1, 2, 3, computed once.  The conditions on the
    fixture are asserted on the restatement alone, before the library runs."""
    frames, store, prob = rs.main_scene()
    moved, ties, count = rs.fixture_conditions(prob)
    print(f"main scene: {count} points with >= 3 good observations, best != 0 for {moved:.2f}, tied least median {ties:.2f}")
    assert count >= 60 and moved >= 0.5 and ties >= 0.05
    assert 380 <= len(prob["slots"]) <= 420 and len(store["desc"]) == CAP
    refs = {w: obr.refresh(store, prob, w) for w in (1, 2, 3)}
    n_good3 = sum(1 for i in range(len(prob["slots"]))
                  if (prob["bad"][prob["off"][i]:prob["off"][i + 1]] == 0).sum() >= 3)
    assert n_good3 == count
    return frames, store, prob, refs, upload(frames)


@pytest.mark.parametrize("what", [1, 2, 3])
def test_store_equals_the_restatement(main_scene, what):
    frames, store, prob, refs, F = main_scene
    mp = store_of(store)
    same_store(whole(mp), store)
    outs = call(mp, prob, F, what)
    want, want_outs = refs[what]
    same_store(whole(mp), want)
    same_outs(outs, want_outs)
    # the call did something: fields it names changed in most listed slots, and only there
    changed = {k: int((np.asarray(want[k]).reshape(CAP, -1) != np.asarray(store[k]).reshape(CAP, -1)).any(axis=1).sum())
               for k in FIELDS}
    assert changed["world_pos"] == 0 and changed["observed"] == 0
    assert (changed["desc"] > 250) == bool(what & 1) and (changed["desc"] == 0) == (not what & 1)
    for k in ("normal", "min_dist", "max_dist"):
        assert (changed[k] > 250) == bool(what & 2) and (changed[k] == 0) == (not what & 2)
    if not what & 1:
        assert (outs["best"] == -1).all()


def test_indices_at_the_ends(main_scene):
    """idx = n - 1 of every keyframe, the n = 1 keyframe and kf = n_kf - 1, in a call of their own."""
    frames, store, prob, refs, F = main_scene
    table = prob["table"]
    lists = [[(e, len(frames[table[e]][0]) - 1) for e in range(len(table))], [(0, 0)], [(len(table) - 1, 299), (0, 0)]]
    p = rs.problem(frames, table, lists, None, [len(table) - 1, 0, 0], [CAP - 1, 0, 500], prob["Ow"])
    assert p["kf"].max() == len(table) - 1 and table[0] == 0 and len(frames[0][0]) == 1
    mp = store_of(store)
    run_and_compare(mp, p, F)


def test_observation_counts_at_the_kernels_edges():
    """1, 2, 3, 63, 64, 65 and 128 good observations (65 and 128: the workgroup form), some lists longer than their
    candidates; more observations than keyframes through a keyframe table whose entries name the two 300-feature frames in
    turn.  N = 2: every median is 0 and the first good row wins; N = 3 is the first case of rank 1."""
    frames, store, prob = rs.edge_scene()
    good = [int((prob["bad"][prob["off"][i]:prob["off"][i + 1]] == 0).sum()) for i in range(len(prob["slots"]))]
    assert good == [1, 2, 3, 63, 64, 65, 128] and max(np.diff(prob["off"])) > 128
    F = upload(frames)
    mp = store_of(store)
    for what in (3, 1):
        before, want, outs = run_and_compare(mp, prob, F, what)
    o1 = prob["off"][1]
    assert outs["best"][1] == np.flatnonzero(prob["bad"][o1:prob["off"][2]] == 0)[0]
    assert (outs["best"] >= 0).all()
    # 129 candidates: refused before anything is enqueued, with the cap's own code
    lists = [[(e, e) for e in range(129)]]
    p = rs.problem(frames, prob["table"], lists, None, [0], [7], prob["Ow"])
    before = whole(mp)
    with pytest.raises(orb.VsgError) as e:
        call(mp, p, F)
    assert e.value.code == oc.UNSUPPORTED
    same_store(whole(mp), before)
    # ... and 129 of which one is bad runs
    p = rs.problem(frames, prob["table"], lists, [np.eye(1, 129, 64, dtype=np.uint8)[0]], [64], [7], prob["Ow"])
    run_and_compare(mp, p, F)


def test_bad_flags(main_scene):
    frames, store, prob, refs, F = main_scene
    table = prob["table"]
    lists = [[(2, 3), (3, 4), (4, 5), (5, 6), (6, 7)],   # one bad observation in the middle
             [(2, 8), (3, 9), (4, 10)],                  # a bad reference observation
             [(3, 11), (4, 12), (7, 13)],                # all bad
             []]                                         # no observation
    bad = [[0, 0, 1, 0, 0], [0, 1, 0], [1, 1, 1], []]
    p = rs.problem(frames, table, lists, bad, [0, 1, 2, 0], [10, 11, 12, 13], prob["Ow"])
    mp = store_of(store)
    before, want, outs = run_and_compare(mp, p, F)
    after = whole(mp)
    assert outs["best"][0] in (0, 1, 3, 4) and outs["best"][1] in (0, 2)
    assert outs["best"][2] == -1 and after["desc"][12].tobytes() == before["desc"][12].tobytes()
    assert not np.array_equal(after["normal"][12], before["normal"][12]) and after["max_dist"][12] != before["max_dist"][12]
    # the bad observation counts for the normal: without it the mean differs
    no_mid = rs.problem(frames, table, [lists[0][:2] + lists[0][3:]], None, [0], [10], prob["Ow"])
    assert not np.array_equal(obr.refresh(before, no_mid, 2)[0]["normal"][10], after["normal"][10])
    assert outs["best"][3] == -1
    for k in FIELDS:
        assert np.asarray(after[k][13]).tobytes() == np.asarray(before[k][13]).tobytes()
    assert outs["normal"][3].tobytes() == before["normal"][13].tobytes() and outs["min_dist"][3] == before["min_dist"][13]


def test_refusals_leave_the_store_alone_and_the_next_call_right(main_scene):
    """Every refusal of csrc/vsg_obs_args.h (tests/obs_cases.py, on the frames those cases are written for) and a keyframe
    with Nleft != -1: the code, a byte-identical store, and a valid call on the same thread right after that is right."""
    frames, store, prob, refs, F = main_scene
    table = [0, 1, 2, 3, 4]
    Ow = prob["Ow"][:5]
    mp = store_of(store)
    default = oc.octaves()
    assert all(np.array_equal(frames[k][0]["octave"], default[k]) for k in range(5))

    def as_problem(c):
        p = dict(slots=c["slots"], off=c["off"], kf=c["kf"], idx=c["idx"], bad=c["bad"] if c["use_bad"] else None,
                 ref_pos=c["ref_pos"], frames=[frames[f] for f in table], table=table, Ow=Ow,
                 scale_factors=(np.float32(1.2) ** np.arange(c["nlevels"], dtype=np.float32)).astype(np.float32))
        return p

    refused = accepted = 0
    for name, (c, rc) in sorted(oc.cases().items()):
        if not all(np.array_equal(a, b) for a, b in zip(c["oct"], default)) or c["nlevels"] < 1:
            continue  # octaves other than the uploaded frames': covered below through nlevels
        p = as_problem(c)
        if rc == oc.OK:
            run_and_compare(mp, p, F)
            accepted += 1
            continue
        before = whole(mp)
        with pytest.raises(orb.VsgError) as e:
            call(mp, p, F)
        assert e.value.code == rc, name
        same_store(whole(mp), before)
        refused += 1
    assert refused >= 14 and accepted >= 8
    before = whole(mp)
    base = as_problem(oc.base())

    def refuse(p, code, frames_=None, what=3):
        with pytest.raises(orb.VsgError) as e:
            call(mp, p, frames_ or F, what)
        assert e.value.code == code
        same_store(whole(mp), before)

    # the reference keypoint's octave (7) is not below nlevels = 7; nlevels 0 and 17; what outside 1 .. 3
    refuse(dict(base, scale_factors=rs.SF[:7]), oc.INVALID)
    refuse(dict(base, scale_factors=np.ones(17, np.float32)), oc.INVALID)
    refuse(dict(base, scale_factors=np.ones(0, np.float32)), oc.INVALID)
    refuse(base, oc.INVALID, what=0)
    refuse(base, oc.INVALID, what=4)
    # a keyframe uploaded with Nleft != -1
    two = orb.Frame(301).upload(frames[3][0], frames[3][1], rs.BOUNDS, nleft=150)
    refuse(base, oc.UNSUPPORTED, frames_=F[:3] + [two] + F[4:])
    # no points: nothing happens
    empty = dict(base, slots=np.zeros(0, np.int32), off=np.zeros(1, np.int32), kf=np.zeros(0, np.int32),
                 idx=np.zeros(0, np.int32), bad=None, ref_pos=np.zeros(0, np.int32))
    assert len(call(mp, empty, F)["best"]) == 0
    same_store(whole(mp), before)
    # ... and the valid call right after
    run_and_compare(mp, prob, F)


def test_search_local_points_is_the_same_on_refreshed_and_uploaded_fields():
    """Two stores of the same points: in one the four fields come from the restatement through update, in the other from
    refresh.  Tracking::SearchLocalPoints on a resident frame gives identical outputs from both."""
    rng = np.random.default_rng(23)
    n = 600
    pose, bounds, f = fr.scenario(5, "tum1", n=n)
    frames = rs.keyframes(7)
    table = [3, 4, 3, 4, 2, 3]
    Ow = (pose["Ow"][None, :] + rng.normal(0, 0.3, (len(table), 3))).astype(np.float32)
    lists = []
    for i in range(n):
        entries = np.sort(rng.choice(len(table), rng.integers(2, 6), replace=False))
        lists.append([(int(e), int(rng.integers(0, len(frames[table[e]][0])))) for e in entries])
    prob = rs.problem(frames, table, lists, None, [int(rng.integers(0, len(l))) for l in lists], np.arange(n), Ow)
    want, _ = obr.refresh(f, prob, 3)
    want["observed"], want["world_pos"] = f["observed"], f["world_pos"]
    ref0 = fr.is_in_frustum(pose, bounds, want["world_pos"], want["normal"], want["min_dist"], want["max_dist"])
    iv = np.flatnonzero(ref0["in_view"])
    assert len(iv) >= 40, len(iv)
    keys = np.zeros(len(iv), orb.KP_DTYPE)
    keys["x"] = ref0["proj_x"][iv] + rng.normal(0, 0.5, len(iv)).astype(np.float32)
    keys["y"] = ref0["proj_y"][iv] + rng.normal(0, 0.5, len(iv)).astype(np.float32)
    keys["octave"] = np.maximum(ref0["scale_level"][iv] - rng.integers(0, 2, len(iv)), 0)
    desc = want["desc"][iv].copy()
    desc[:, 0] ^= rng.integers(0, 256, len(iv), dtype=np.uint8)
    Fr = orb.Frame(len(keys) + 1).upload(keys, desc, bounds)
    mp_a = ps.store_of(want, np.arange(n))
    mp_b = ps.store_of(f, np.arange(n))
    call(mp_b, prob, upload(frames))
    same_store(whole(mp_b), want)
    P = orb.FramePose.make(**pose)
    a = Fr.SearchLocalPoints(mp_a, P, 3.0, 0.8, rs.SF, np.zeros(len(keys), np.uint8))
    b = Fr.SearchLocalPoints(mp_b, P, 3.0, 0.8, rs.SF, np.zeros(len(keys), np.uint8))
    assert a[0] == b[0] and a[0] >= 0.5 * len(iv) and a[6] == b[6] == len(iv)
    for x, y in zip(a[1:6], b[1:6]):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()


def _blob(a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    return np.int32(a.size if a.dtype.names is None else len(a)).tobytes() + a.tobytes()


def _load(buf, pos, dtype):
    n = int(np.frombuffer(buf, np.int32, 1, pos)[0])
    a = np.frombuffer(buf, dtype, n, pos + 4)
    return a, pos + 4 + a.nbytes


def test_cpp_adaptor_equals_the_restatement(main_scene, tmp_path):
    frames, store, prob, refs, F = main_scene
    subprocess.check_call(["make", "-C", str(ADAPTOR)], stdout=subprocess.DEVNULL)
    table = prob["table"]
    parts = [_blob([CAP, 3, len(table)], np.int32)]
    for f in table:
        parts += [_blob(frames[f][0], orb.KP_DTYPE), _blob(frames[f][1], np.uint8)]
    parts += [_blob(prob["Ow"], np.float32), _blob(rs.SF, np.float32), _blob(store["world_pos"][prob["slots"]], np.float32),
              _blob(prob["slots"], np.int32), _blob(prob["off"], np.int32), _blob(prob["kf"], np.int32),
              _blob(prob["idx"], np.int32), _blob(prob["ref_pos"], np.int32), _blob(prob["bad"], np.uint8)]
    src, out = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(b"".join(parts))
    r = subprocess.run([str(ADAPTOR / "refresh_check"), str(src), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    buf, pos, got = out.read_bytes(), 0, {}
    for name, dt in (("best", np.int32), ("normal", np.float32), ("min_dist", np.float32), ("max_dist", np.float32),
                     ("s_normal", np.float32), ("s_min", np.float32), ("s_max", np.float32), ("s_desc", np.uint8)):
        got[name], pos = _load(buf, pos, dt)
    assert pos == len(buf)
    # the program's store starts from zeros: the restatement of THAT store (positions set, the rest 0)
    zero = {k: np.zeros_like(v) for k, v in store.items()}
    zero["world_pos"][prob["slots"]] = store["world_pos"][prob["slots"]]
    want, outs = obr.refresh(zero, prob, 3)
    same_outs({k: got[k].reshape(np.shape(outs[k])) for k in outs}, outs)
    s = prob["slots"]
    assert got["s_normal"].tobytes() == want["normal"][s].tobytes() and got["s_desc"].tobytes() == want["desc"][s].tobytes()
    assert got["s_min"].tobytes() == want["min_dist"][s].tobytes() and got["s_max"].tobytes() == want["max_dist"][s].tobytes()
