"""The parity scene of the triangulation search with the epipolar test on the device, built on the CPU (the oracle extractor)
so that tests/test_epipolar_reference.py can check it against the restatement alone before any GPU test uses it:

  * two frames of a synthetic 320 x 240 sequence, the second one the "t + 1" frame shifted by (-3, -2) px: true
    correspondences are near-equal descriptors 3.6 px apart;
  * mvuRight on about a third of the features of each frame;
  * F12 of a sideways translation along the image shift (equal intrinsics, no rotation): x2 = x1 + shift lies on the epipolar
    line of x1.  The epipole handed in sits inside a keypoint cluster of the second frame, so the gate fires;
  * a second matrix whose lines all pass through ONE keypoint of the first frame: for that keypoint a = b = 0 exactly
    (den == 0);
  * synthetic FeatureVectors of 10 / 10 nodes, 8 of them shared: a node of more rows on each side than the kernel's 128-row tiles, a node of
    more than 64 rows on the KF2 side, nodes of one row on a side, nodes only one frame has, and KF2 features duplicated
    inside their node (descriptor and keypoint), the copy LATER in the node's list: the later-wins rule decides."""
import functools

import numpy as np

import epipolar_reference as er
import oracle_lib as ol
from visual_sgraphs_amd import synth

F32 = np.float32
W, H, SHIFT = 320, 240, (-3.0, -2.0)
BOUNDS = (0.0, 0.0, float(W), float(H))
TILE = 128  # kEpiTile = kEpiRows of k_triangulation_walk


def fundamental_sideways(f, cx, cy, t):
    """F12 = K^-T [t]x K^-1 for R12 = I and equal pinhole intrinsics, in double, rounded to float once per entry."""
    K = np.array([[f, 0, cx], [0, f, cy], [0, 0, 1]], np.float64)
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]], np.float64)
    Ki = np.linalg.inv(K)
    return (Ki.T @ tx @ Ki).astype(F32)


def fundamental_through(x0, y0):
    """A matrix whose line for kp1 is (x1 - x0, y1 - y0, .): a = b = 0 exactly at (x0, y0) -- products with 1 and 0 and one
    exact difference -- and nowhere else."""
    return np.array([[1, 0, 0], [0, 1, 0], [-x0, -y0, 1]], F32)


def _node_lists(order, sizes):
    """Consecutive runs of `order` with the given sizes (the rest is dropped)."""
    out, at = [], 0
    for s in sizes:
        out.append(np.asarray(order[at:at + s], np.int32))
        at += s
    return out


def _fv(nodes):
    """{node id: feature list} -> (ids, off, idx) in ascending id."""
    ids = sorted(nodes)
    off = np.concatenate([[0], np.cumsum([len(nodes[i]) for i in ids])]).astype(np.int32)
    idx = np.concatenate([nodes[i] for i in ids]).astype(np.int32) if ids else np.zeros(0, np.int32)
    return np.asarray(ids, np.int32), off, idx


@functools.lru_cache(maxsize=None)
def frames(seed=1):
    """dict with k1, d1, ur1, no_mp1, fv1 (and the same for frame 2), sf, sigma2, F12, F12_den0, ep."""
    rng = np.random.default_rng(100 + seed)
    ex = ol.OracleExtractor(390, 1.2, 4, 20, 7)
    (_, k1, d1), (_, k2, d2) = (ex(synth.sequence_frame(W, H, seed, t)) for t in range(2))
    k1, d1, k2, d2 = k1.copy(), d1.copy(), k2.copy(), d2.copy()
    n1, n2 = len(k1), len(k2)
    assert 200 <= n1 <= 400 and 200 <= n2 <= 400, (n1, n2)
    tb = ex.tables()
    # the true correspondence of a KF1 feature: the nearest descriptor among the KF2 features one shift away
    dist = er.hamming(d1[:, None, :], d2[None, :, :])
    dx = k2["x"][None, :] - k1["x"][:, None] - SHIFT[0]
    dy = k2["y"][None, :] - k1["y"][:, None] - SHIFT[1]
    near = dx * dx + dy * dy <= 4.0
    best = np.where(near, dist, 999).argmin(1)
    match = np.where(np.where(near, dist, 999).min(1) <= er.TH_LOW, best, -1)
    # ---- FeatureVectors: KF2 features in x order cut into nodes; a KF1 feature goes where its correspondence is, one
    # without a correspondence where a KF2 feature at its own position would be
    order2 = np.argsort(k2["x"], kind="stable")
    sizes2 = [TILE + 12, 70, 1, 24, 17, 9, 30, 13]
    assert sum(sizes2) <= n2
    lists2 = _node_lists(order2, sizes2)
    rest2 = order2[sum(sizes2):]
    node_of2 = np.full(n2, -1)
    for s, l in enumerate(lists2):
        node_of2[l] = s
    edges = [k2["x"][l].max() for l in lists2]
    own = np.searchsorted(edges, k1["x"] + SHIFT[0])
    node_of1 = np.where(match >= 0, node_of2[np.maximum(match, 0)], np.minimum(own, len(sizes2)))
    ids = [3, 7, 12, 20, 21, 33, 40, 57]  # ascending ids of the eight shared nodes
    nodes1 = {ids[s]: np.flatnonzero(node_of1 == s).astype(np.int32) for s in range(len(sizes2))}
    nodes2 = {ids[s]: lists2[s] for s in range(len(sizes2))}
    # node 12 has ONE row on the KF2 side; node 33 gets one row on the KF1 side (the others move to a KF1-only node)
    extra1 = nodes1[33][1:]
    nodes1[33] = nodes1[33][:1]
    only1 = np.concatenate([np.flatnonzero((node_of1 < 0) | (node_of1 >= len(sizes2))), extra1]).astype(np.int32)
    nodes1.update({5: only1[::2], 60: only1[1::2]})       # nodes only KF1 has (before, between and after the shared ones)
    nodes2.update({4: rest2[::2].astype(np.int32), 58: rest2[1::2].astype(np.int32)})  # nodes only KF2 has
    nodes1 = {i: l for i, l in nodes1.items() if len(l)}
    nodes2 = {i: l for i, l in nodes2.items() if len(l)}
    # ---- duplicates inside a node: a later row of the node becomes a copy of a matched row (descriptor AND keypoint)
    ndup = 0
    for nid in (3, 7, 20, 40):
        l = nodes2[nid]
        matched = [p for p in range(len(l) - 1) if (match == l[p]).any()]
        for p in matched[:4]:
            q = int(rng.integers(p + 1, len(l)))
            if (match == l[q]).any():
                continue  # a row that is a correspondence itself stays
            d2[l[q]], k2[l[q]] = d2[l[p]], k2[l[p]]
            ndup += 1
    assert ndup >= 4
    ur1 = np.where(rng.random(n1) < 0.33, k1["x"] - rng.uniform(1, 20, n1), -1.0).astype(F32)
    ur2 = np.where(rng.random(n2) < 0.33, k2["x"] - rng.uniform(1, 20, n2), -1.0).astype(F32)
    no_mp1, no_mp2 = (rng.random(n1) < 0.8).astype(np.uint8), (rng.random(n2) < 0.8).astype(np.uint8)
    # the epipole inside the densest part of the big node's KF2 features; the translation along the shift
    big = nodes2[3]
    ep = np.array([np.median(k2["x"][big]), np.median(k2["y"][big])], F32)
    F12 = fundamental_sideways(260.0, 160.0, 120.0, (0.3, 0.2, 0.0))
    # den == 0 for one KF1 feature of the big node that has a correspondence, no map point and is mono (so is its partner)
    cand = [i for i in nodes1[3] if match[i] >= 0 and no_mp1[i] and no_mp2[match[i]]]
    assert cand
    pivot = int(cand[0])
    return dict(k1=k1, d1=d1, ur1=ur1, no_mp1=no_mp1, fv1=_fv(nodes1), k2=k2, d2=d2, ur2=ur2, no_mp2=no_mp2, fv2=_fv(nodes2),
                sf=tb["scale"], sigma2=tb["sigma2"], F12=F12, F12_den0=fundamental_through(k1["x"][pivot], k1["y"][pivot]),
                ep=ep, match=match, pivot=pivot)


# the legs every parity test runs: name -> (matrix key, only_stereo, coarse, KF1 has mvuRight, KF2 has mvuRight)
LEGS = {
    "plain": ("F12", False, False, True, True),
    "only_stereo": ("F12", True, False, True, True),
    "coarse": ("F12", False, True, True, True),
    "den0": ("F12_den0", False, False, True, True),
    "kf1_without_uright": ("F12", False, False, False, True),
    "kf2_without_uright_only_stereo": ("F12", True, False, True, False),
}


def leg_scene(s, leg, no_mp1=None, no_mp2=None):
    """The restatement of one leg of frames()."""
    key, only_stereo, coarse, u1, u2 = LEGS[leg]
    return er.scene(s["k1"], s["ur1"] if u1 else None, s["no_mp1"] if no_mp1 is None else no_mp1, s["fv1"], s["d1"], s["k2"],
                    s["ur2"] if u2 else None, s["no_mp2"] if no_mp2 is None else no_mp2, s["fv2"], s["d2"], s[key], s["ep"],
                    s["sf"], s["sigma2"], only_stereo, coarse)


def _around(v, k):
    i = np.asarray(v, F32).view(np.int32).astype(np.int64) + np.arange(-k, k + 1)
    return i.astype(np.int32).view(F32)


def directed_cases(sf, sigma2):
    """The edge cases of tests/test_epipolar_reference.py as lists of pairs, for the device predicate: name -> dict of
    per-pair arrays x1, y1, ur1, x2, y2, ur2, octave2 and F12, ep, only_stereo, coarse.  The expected codes are the
    restatement's (`reason`); `must` lists codes that have to occur in the case."""
    sf, sigma2 = np.asarray(sf, F32), np.asarray(sigma2, F32)
    nl = len(sf)
    line_y = np.array([[0, 0, 0], [0, 0, 0], [0, 1, 0]], F32)
    far = np.array([1e6, 1e6], F32)
    cases = {}

    def add(name, x1, y1, ur1, x2, y2, ur2, octave2, F12, ep, only_stereo=False, coarse=False, must=()):
        n = max(np.size(v) for v in (x1, y1, ur1, x2, y2, ur2, octave2))
        c = {k: np.ascontiguousarray(np.broadcast_to(np.asarray(v, F32), (n,)))
             for k, v in dict(x1=x1, y1=y1, ur1=ur1, x2=x2, y2=y2, ur2=ur2).items()}
        c["octave2"] = np.ascontiguousarray(np.broadcast_to(np.asarray(octave2, np.int32), (n,)))
        c.update(F12=np.asarray(F12, F32).reshape(9), ep=np.asarray(ep, F32), only_stereo=only_stereo, coarse=coarse)
        c["reason"] = er.pair_reasons(c["x1"], c["y1"], c["ur1"], c["x2"], c["y2"], c["ur2"], c["octave2"], c["F12"], c["ep"],
                                      sf, sigma2, only_stereo, coarse)
        assert set(must) <= set(c["reason"].tolist()), (name, must, set(c["reason"].tolist()))
        cases[name] = c

    ramp = np.linspace(0, 300, 64, dtype=F32)
    add("zero_matrix", 10, 20, -1, ramp, ramp, -1, 0, np.zeros(9), far, must=(er.DEN_ZERO,))
    ep = np.array([100.0, 50.0], F32)
    u1, u2 = np.array([-1, 7, -1, 7, 0.0, -0.0], F32), np.array([-1, -1, 9, 9, -1, -1], F32)
    for coarse in (False, True):
        add("stereo_exempt_from_gate_coarse%d" % coarse, 0, 0, u1, np.full(6, 103.0), np.full(6, 50.0), u2, 0, line_y, ep,
            coarse=coarse, must=(er.EPIPOLE_GATE, er.PASS) if coarse else (er.EPIPOLE_GATE, er.CHI_SQUARE))
    add("only_stereo", 0, 0, u1[:4], np.full(4, 100.0), np.array([50, 50, 50, 1.0]), u2[:4], 0, line_y, ep, only_stereo=True,
        must=(er.NOT_STEREO,))
    for at in range(9):
        F = line_y.copy().reshape(9)
        F[at] = np.nan
        add("nan_in_matrix_%d" % at, 10, 20, 5, ramp[:16], np.zeros(16), 5, 0, F, far, must=(er.CHI_SQUARE,))
    # dsqr one ulp either side of 3.84 * sigma2 (see the CPU test): per scale b of the line, every level's floats round the
    # y2 whose dsqr is the largest float below the bound
    for b in (1.0, 1.25, 1.5, 1.75, 0.7, 0.9, 1.1, 1.3, 1.7, 2.3, 3.1, 5.3):
        F = np.zeros((3, 3), F32)
        F[2, 1] = b
        ys, lv = [], []
        for level in range(nl):
            bound = np.float64(3.84) * np.float64(sigma2[level])
            T = F32(bound)
            T = np.nextafter(T, F32(0)) if np.float64(T) >= bound else T
            y2 = _around(F32(np.sqrt(np.float64(T))), 24)   # dsqr = (b y2)^2 / b^2
            ys.append(y2), lv.append(np.full(len(y2), level))
        add("chi_square_ulp_b%g" % b, 3, 4, 5, 0, np.concatenate(ys), 5, np.concatenate(lv), F, far,
            must=(er.PASS, er.CHI_SQUARE))
    # the gate distance one ulp either side of 100 * sf (see the CPU test)
    xs, ys, lv = [], [], []
    for level in range(nl):
        gate = F32(F32(100) * sf[level])
        top = np.floor(np.sqrt(np.float64(gate) - 1.0) * 4) / 4
        for dy in (top, top - 0.25, top - 0.5):
            x2 = _around(F32(4.0 - np.sqrt(np.float64(gate) - dy * dy)), 40)
            xs.append(x2), ys.append(np.full(len(x2), 100.0 - dy)), lv.append(np.full(len(x2), level))
    add("gate_ulp", 0, 0, -1, np.concatenate(xs), np.concatenate(ys), -1, np.concatenate(lv), line_y, [4.0, 100.0], coarse=True,
        must=(er.EPIPOLE_GATE, er.PASS))
    return cases
