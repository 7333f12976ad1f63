"""GPU parity test of the C++ drop-in layer: tests/_adaptor/adaptor_check.cpp drives include/vsg_orb_adaptor.hpp
(vsg::ORBextractor / FrameGrid / ORBVocabulary / ORBmatcher) from plain C++ over the C ABI, generating its inputs
with include/vsg_synth.h; everything it produces must equal the CPU oracle bit for bit."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import oracle_lib as ol
from visual_sgraphs_amd import orb, synth

pytestmark = pytest.mark.gpu
DIR = Path(__file__).resolve().parent / "_adaptor"


def _read(path):
    raw = Path(path).read_bytes()
    pos = 0

    def take(dtype):
        nonlocal pos
        n = int(np.frombuffer(raw, np.int32, 1, pos)[0])
        pos += 4
        a = np.frombuffer(raw, dtype, n, pos).copy()
        pos += a.nbytes
        return a
    out = {"head": take(np.int32)}
    for t in range(2):
        out[f"kps{t}"] = take(orb.KP_DTYPE)
        out[f"desc{t}"] = take(np.uint8).reshape(-1, 32)
    for k in ("cand_off", "cand_idx", "best_idx", "best_dist", "train_match", "match_f", "init12", "bow_ids"):
        out[k] = take(np.int32)
    out["bow_vals"] = take(np.float64)
    out["tri"] = take(np.int32).reshape(-1, 2)
    for k in ("r_last", "r_sim3", "r_fuse_idx", "r_fuse_dist", "r_init"):
        out[k] = take(np.int32)
    for t in range(2):
        out[f"big_kps{t}"] = take(orb.KP_DTYPE)
        out[f"big_desc{t}"] = take(np.uint8).reshape(-1, 32)
    for k in ("big_match_f", "big_match12"):
        out[k] = take(np.int32)
    out["edge_head"] = take(np.int32)
    out["b_kps"], out["b_desc"] = take(orb.KP_DTYPE), take(np.uint8).reshape(-1, 32)
    for k in ("b_off", "b_idx", "b_sim3", "b_last"):
        out[k] = take(np.int32)
    out["c_kps"], out["c_desc"] = take(orb.KP_DTYPE), take(np.uint8).reshape(-1, 32)
    for k in ("c_x", "c_y", "c_r"):
        out[k] = take(np.float32)
    out["c_qdesc"] = take(np.uint8).reshape(-1, 32)
    for k in ("c_level", "c_off", "c_idx", "c_sim3", "c_fuse_idx", "c_fuse_dist"):
        out[k] = take(np.int32)
    assert pos == len(raw)
    return out


def test_cpp_adaptor_end_to_end_equals_oracle(tmp_path):
    from visual_sgraphs_amd import build
    build.build()
    subprocess.check_call(["make", "-C", str(DIR)], stdout=subprocess.DEVNULL)
    blob = synth.synthetic_vocabulary(k=10, L=3, seed=4)
    (tmp_path / "voc.bin").write_bytes(blob)
    r = subprocess.run([str(DIR / "adaptor_check"), str(tmp_path / "voc.bin"), str(tmp_path / "out.bin")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
    got = _read(tmp_path / "out.bin")

    # extractor
    ref = ol.OracleExtractor(1000, 1.2, 8, 20, 7)
    want = [ref(synth.sequence_frame(640, 480, 5, t)) for t in range(2)]
    for t in range(2):
        assert int(got["head"][t]) == want[t][0]
        assert got[f"kps{t}"].tobytes() == want[t][1].tobytes()
        assert np.array_equal(got[f"desc{t}"], want[t][2])
    (_, k0, d0), (_, k1, d1) = want
    assert len(k0) > 900 and len(k1) > 900

    # grid candidates
    g = ol.OracleGrid(k1, 0.0, 0.0, 640.0, 480.0)
    scale = ref.tables()["scale"]
    off, idx = [0], []
    for k in k0:
        c = g.query(np.float32(k["x"]) - np.float32(3), np.float32(k["y"]) - np.float32(2),
                    np.float32(15) * np.float32(scale[k["octave"]]), int(k["octave"]) - 1, int(k["octave"]) + 1)
        idx.extend(c.tolist())
        off.append(len(idx))
    assert np.array_equal(got["cand_off"], off) and np.array_equal(got["cand_idx"], idx)
    assert len(idx) > len(k0)  # the windows are not trivially empty

    # window search
    n, qi, qd, tm, _ = ol.search_window(d0, np.ones(len(d0), np.uint8), off, idx, d1, np.zeros(len(d1), np.uint8), 100)
    assert int(got["head"][2]) == n > 300
    assert np.array_equal(got["best_idx"], qi) and np.array_equal(got["best_dist"], qd)
    assert np.array_equal(got["train_match"], tm)

    # vocabulary + SearchByBoW
    voc = ol.OracleVocabulary(blob)
    t0, t1 = voc.transform(d0, 2), voc.transform(d1, 2)
    assert np.array_equal(got["bow_ids"], t1["bow_ids"]) and got["bow_vals"].tobytes() == t1["bow_vals"].tobytes()
    valid = np.ones(len(d0), np.uint8)
    valid[::7] = 0
    nb, mf = ol.search_by_bow_kf_f(d0, k0["angle"], valid, t0["fv"], d1, k1["angle"], t1["fv"], 0.7, True)
    assert int(got["head"][3]) == nb > 50
    assert np.array_equal(got["match_f"], mf)

    # SearchForTriangulation through the adaptor's predicate-to-bitmask glue
    e0, e1 = np.ones(len(d0), np.uint8), np.ones(len(d1), np.uint8)
    e0[::5] = 0
    e1[::9] = 0
    ids0, off0, idx0 = t0["fv"]
    ids1, off1, idx1 = t1["fv"]
    pair_off, bits = [0], []
    for s_ in np.intersect1d(ids0, ids1):
        a, b = int(np.searchsorted(ids0, s_)), int(np.searchsorted(ids1, s_))
        for i1 in idx0[off0[a]:off0[a + 1]]:
            for i2 in idx1[off1[b]:off1[b + 1]]:
                bits.append(bool(e0[i1] and e1[i2] and (int(i1) * 7 + int(i2) * 3) % 5 != 0))
        pair_off.append(len(bits))
    words = np.zeros(len(bits) // 32 + 2, np.uint32)
    for i in np.nonzero(bits)[0]:
        words[i >> 5] |= np.uint32(1 << (i & 31))
    nt, m12 = ol.search_for_triangulation(d0, k0["angle"], e0, t0["fv"], d1, k1["angle"], e1, t1["fv"], words,
                                          np.array(pair_off, np.int32), True)
    assert int(got["head"][6]) == nt > 20
    want_pairs = np.array([(i, m12[i]) for i in range(len(m12)) if m12[i] >= 0], np.int32).reshape(-1, 2)
    assert np.array_equal(got["tri"], want_pairs)

    # SearchForInitialization + DescriptorDistance
    ni, m12 = ol.search_for_initialization(d0, k0["angle"], k0["octave"], off, idx, d1, k1["angle"], 0.7, True)
    assert int(got["head"][4]) == ni and np.array_equal(got["init12"], m12)
    assert int(got["head"][5]) == ol.descriptor_distance(d0[0], d1[0])

    # ---- resident path (vsg::ResidentFrame / ResidentMatcher) vs the routine-level oracle
    b = (0.0, 0.0, 640.0, 480.0)
    o0, o1 = ol.OracleFrame(k0, d0, b), ol.OracleFrame(k1, d1, b)
    u, v = (k0["x"] - np.float32(3)).astype(np.float32), (k0["y"] - np.float32(2)).astype(np.float32)
    octv, ang = k0["octave"].astype(np.int32), k0["angle"].astype(np.float32)
    ones, zeros = np.ones(len(k0), np.uint8), np.zeros(len(k1), np.uint8)
    nl, tm, _ = o1.search_by_projection_last(d0, ones, u, v, None, octv, ang, 15.0, 0, scale, True, zeros)
    assert int(got["head"][7]) == nl > 300 and np.array_equal(got["r_last"], tm)
    rad = (np.float32(10) * scale[octv]).astype(np.float32)
    ns, m = o1.search_by_projection_sim3(d0, u, v, rad, octv, 1.0, np.full(len(k1), -1, np.int32))
    assert int(got["head"][8]) == ns > 300 and np.array_equal(got["r_sim3"], m)
    inv2 = ref.tables()["inv_sigma2"]
    z = np.zeros(len(k0) + len(k1), np.int32)
    r = o1.fuse(np.arange(len(k0)), d0, u, v, u, rad, octv, inv2, np.full(len(k1), -1, np.int32), z, z.astype(np.uint8))
    assert int(got["head"][9]) == r[0] > 100
    assert np.array_equal(got["r_fuse_idx"], r[1]) and np.array_equal(got["r_fuse_dist"], r[2])
    ni2, mi = o0.search_for_initialization(o1, k0["x"], k0["y"], 100, 0.7, True)
    assert int(got["head"][10]) == ni2 > 50 and np.array_equal(got["r_init"], mi)

    # NULL-FeatureVector SearchByBoW above 2048 features (host-assembled FeatureVectors in the frames) and with empty frames
    gk0, gd0, gk1, gd1 = got["big_kps0"], got["big_desc0"], got["big_kps1"], got["big_desc1"]
    assert len(gd0) == len(gd1) == 3000
    g0, g1 = voc.transform(gd0, 2)["fv"], voc.transform(gd1, 2)["fv"]
    gv0, gv1 = np.ones(3000, np.uint8), np.ones(3000, np.uint8)
    gv0[::4] = 0
    gv1[::9] = 0
    nb, mf = ol.search_by_bow_kf_f(gd0, gk0["angle"], gv0, g0, gd1, gk1["angle"], g1, 0.7, True)
    assert int(got["head"][11]) == nb > 300 and np.array_equal(got["big_match_f"], mf)
    nk, m12 = ol.search_by_bow_kf_kf(gd0, gk0["angle"], gv0, g0, gd1, gk1["angle"], gv1, g1, 0.7, True)
    assert int(got["head"][12]) == nk > 300 and np.array_equal(got["big_match12"], m12)
    assert got["head"][13:16].tolist() == [0, 0, 0]

    # ---- resident frames at the window search's size edges
    # (1) more than 4096 device-built features (the grid launch orders its cells in global memory): the extractor's output,
    # every list of GetFeaturesInArea and two matcher routines equal the oracle's
    bk, bd = got["b_kps"], got["b_desc"]
    _, wk, wd = ol.OracleExtractor(6000, 1.2, 8, 20, 7)(synth.sequence_frame(1280, 720, 21, 0))
    assert len(wk) > 4200 and bk.tobytes() == wk.tobytes() and np.array_equal(bd, wd)
    ob = ol.OracleFrame(wk, wd, (0.0, 0.0, 1280.0, 720.0))
    occ = np.diff(ob.grid()[0])
    assert (occ >= 2).sum() >= 30 and occ.max() >= 8   # unsorted cells would show
    qs = np.arange(0, len(wk), 3)
    qu, qv = (wk["x"][qs] + np.float32(1)).astype(np.float32), (wk["y"][qs] - np.float32(1)).astype(np.float32)
    qo = wk["octave"][qs].astype(np.int32)
    qr = (np.float32(12) * scale[qo]).astype(np.float32)
    off, idx = [0], []
    for i in range(len(qs)):
        idx.extend(ob.features_in_area(qu[i], qv[i], qr[i], kf_form=True).tolist())
        off.append(len(idx))
    assert np.array_equal(got["b_off"], off) and np.array_equal(got["b_idx"], idx) and len(idx) > 10 * len(qs)
    ns, m = ob.search_by_projection_sim3(wd[qs], qu, qv, qr, qo, 1.0, np.full(len(wk), -1, np.int32))
    assert int(got["edge_head"][0]) == ns > 1000 and np.array_equal(got["b_sim3"], m)
    nl, tm, _ = ob.search_by_projection_last(wd[qs], np.ones(len(qs), np.uint8), qu, qv, qu, qo,
                                             wk["angle"][qs].astype(np.float32), 12.0, 0, scale, True,
                                             np.zeros(len(wk), np.uint8))
    assert int(got["edge_head"][1]) == nl > 1000 and np.array_equal(got["b_last"], tm)
    # (2) cells of 1, 32, 33 and 150 entries: the full 32-entry cell goes through the last bit of the kernel's survivor mask,
    # the larger ones through its two-pass filter
    ck, cd = got["c_kps"], got["c_desc"]
    oc = ol.OracleFrame(ck, cd, b)
    assert sorted(np.diff(oc.grid()[0])[np.diff(oc.grid()[0]) > 0].tolist()) == [1, 32, 33, 150]
    cx, cy, cr = got["c_x"], got["c_y"], got["c_r"]
    off, idx = [0], []
    for i in range(len(cx)):
        idx.extend(oc.features_in_area(cx[i], cy[i], cr[i], kf_form=True).tolist())
        off.append(len(idx))
    assert np.array_equal(got["c_off"], off) and np.array_equal(got["c_idx"], idx)
    assert {32, 33, 150} <= set(np.diff(off).tolist())   # whole cells are listed
    cq, cl = got["c_qdesc"], got["c_level"]
    ns, m = oc.search_by_projection_sim3(cq, cx, cy, cr, cl, 3.0, np.full(len(ck), -1, np.int32))
    assert int(got["edge_head"][2]) == ns >= 10 and np.array_equal(got["c_sim3"], m)
    z = np.zeros(len(cx) + len(ck), np.int32)
    r = oc.fuse_sim3(np.arange(len(cx)), cq, cx, cy, cr, cl, np.full(len(ck), -1, np.int32), z, z.astype(np.uint8))
    assert int(got["edge_head"][3]) == r[0]
    assert np.array_equal(got["c_fuse_idx"], r[1]) and np.array_equal(got["c_fuse_dist"], r[2]) and (r[1] >= 0).sum() >= 10
