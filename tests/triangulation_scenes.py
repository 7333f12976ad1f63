"""True 3D scenes for the tests of CreateNewMapPoints on resident keyframes (vsg_frame_triangulate_matches /
vsg_frame_create_new_map_points), built on the CPU so that tests/test_triangulation_reference.py can check them against the
restatement alone (tests/triangulation_reference.py) before any GPU test uses them.

  * parity(): about 300 points seen from two poses of a 320 x 240 pinhole camera (f = 260), depths 0.4 .. 80 against a
    baseline of 0.09 (just under mb, so that all three sources occur), the parallax of the true pairs running from far below to
    far above the 0.9998 / 0.9996 limits; a third
    of the features of each frame with mvuRight (mb = 0.1); 4 levels; pixel noise of 0.3 px; outlier matches (a wrong partner)
    that fail the depth signs, the reprojection gates and the far-point gate; descriptors random with true partners a few bits
    apart; keypoint angles of true partners within 25 degrees (four rotation bins, the fourth loses), and a group rotated by 90
    degrees: geometrically good pairs that only the rotation-consistency filter of the fused call removes; host FeatureVectors of 12 nodes.
  * directed(): one scene per reason code and per source, each gate's value clearly off its threshold.  w_zero needs a point at
    infinity to reach Triangulate, which parallel rays (cosParallaxRays = 1) never do on their own: the scene hands in
    cos_parallax = 2 for a stereo keypoint (it is an input the library does not interpret) with both cameras rolled about one
    optical axis and both keypoints at the principal point, so that A's first column is exactly zero.
  * edge(n): n features (1, 63, 64, 65, 255, 256, 257, 1030; 0 is an empty build()), every feature a good pair; edge_sets(n) lists
    which features carry a match.  k_new_points scans in waves of 64 lanes and chunks of 512 features: the sets put accepted
    pairs on both sides of 63|64, 511|512 and 1023|1024.

TOL -- how far x3D of the header's host build may lie from the restatement -- is MEASURED, not chosen: the largest deviation,
over the triangulated pairs of all scenes here, of x3D from numpy.linalg.svd run on the float32 A from x3D of the same run in
float64, relative to |x3D| (the float32 SVD stands in for the reference's float JacobiSVD; the header has to be at least as close to the float64 null
vector as a float SVD is).  No margin is added.  Measured on this tree (python tests/triangulation_scenes.py prints both):
    2202 triangulated pairs
    TOL (float32 SVD against the unrounded float64 SVD)   1.06e-07 of |x3D|   (its median over the pairs: 3.0e-08)
    the header's x3D against the same                     1.06e-07 of |x3D|   (bit for bit the float32 SVD's x3D on every pair)
    the header's double null vector, before its rounding  5.2e-13 of |x3D|
Both deviations are taken from x3D of the float64 SVD BEFORE any rounding to float32: numpy.linalg.svd computes a float32 input in
double and rounds the result, so TOL is what the rounding of x3Dh to float32 and the float32 quotient cost, and the header, whose
double null vector is five orders of magnitude closer than that, pays exactly the same.
A pair is NEAR a threshold when moving x3D by TOL * |x3D| along any of the 14 axis and diagonal directions changes the reason the
restatement's gates give; near pairs are exempt from the reason comparison of the host build against the restatement (never of
the device against the host build).  test_triangulation_reference.py asserts on the restatement alone that at most 1 % of the
parity scene's matched pairs are near and none of the directed and edge scenes'."""
import functools

import numpy as np

import triangulation_reference as tr

F32, F64, I32, U8 = np.float32, np.float64, np.int32, np.uint8
W, H, FOCAL, CX, CY, MB = 320, 240, 260.0, 160.0, 120.0, 0.1
MBF = FOCAL * MB
BOUNDS = (0.0, 0.0, float(W), float(H))
NLEVELS = 4
SF = (F32(1.2) ** np.arange(NLEVELS, dtype=F32)).astype(F32)
SIGMA2 = (SF * SF).astype(F32)
WAVE, CHUNK = 64, 512  # k_new_points: lanes per scan, features per chunk
EDGE_COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 1030)


def kp_dtype():
    from visual_sgraphs_amd import orb
    return orb.KP_DTYPE


def rot(axis, deg):
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def stereo_values(x, y, depth):
    """{x3Dc, cos parallax} per feature as the caller of vsg_frame_set_stereo_points computes them (KeyFrame.cc:887-894 with
    mvKeys = mvKeysUn here; LocalMapping.cc:569), float32 throughout."""
    x, y, z = np.asarray(x, F32), np.asarray(y, F32), np.asarray(depth, F32)
    invf = F32(1) / F32(FOCAL)
    with np.errstate(all="ignore"):
        cosp = np.cos(F32(2) * np.arctan2(F32(MB) / F32(2), z)).astype(F32)
    return np.stack([(x - F32(CX)) * z * invf, (y - F32(CY)) * z * invf, z, cosp], axis=1).astype(F32)


def _keys(x, y, octave, angle):
    k = np.zeros(len(x), kp_dtype())
    k["x"], k["y"], k["octave"], k["angle"] = x, y, octave, angle
    k["size"] = 31.0 * SF[np.asarray(octave, int)] if len(x) else 0
    return k


def _fv(nodes):
    ids = sorted(nodes)
    off = np.concatenate([[0], np.cumsum([len(nodes[i]) for i in ids])]).astype(I32)
    idx = np.concatenate([nodes[i] for i in ids]).astype(I32) if ids else np.zeros(0, I32)
    return np.asarray(ids, I32), off, idx


def fundamental(c1, c2):
    """F12 = K1^-T [t12]x R12 K2^-1 (Pinhole.cpp:121-124) and ep = project_2(T2w * Ow1) (ORBmatcher.cc:913-915), in double,
    rounded once per entry."""
    R1, t1, R2, t2 = (np.asarray(a, F64) for a in (c1["Rcw"], c1["tcw"], c2["Rcw"], c2["tcw"]))
    R12 = R1 @ R2.T
    t12 = -R12 @ t2 + t1
    tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])
    K = np.array([[FOCAL, 0, CX], [0, FOCAL, CY], [0, 0, 1.0]])
    Ki = np.linalg.inv(K)
    C1 = R2 @ np.asarray(c1["Ow"], F64) + t2
    with np.errstate(all="ignore"):
        ep = np.array([FOCAL * C1[0] / C1[2] + CX, FOCAL * C1[1] / C1[2] + CY])
    return (Ki.T @ tx @ R12 @ Ki).astype(F32), ep.astype(F32)


def build(points, c1, c2, rng, stereo_frac=1 / 3, noise=0.3, outliers=0, extra=0, rotated=0, P_kw=None, octaves=None):
    """A scene: frame 1 sees points[i] as feature i, frame 2 as feature perm[i]; `extra` features per frame see nothing shared.
    The last `outliers` matched features of frame 1 are matched to a WRONG partner; `rotated` true pairs get keypoint angles 90
    degrees apart."""
    X = np.asarray(points, F64).reshape(-1, 3)
    n = len(X)
    n1 = n2 = n + extra

    def view(c):
        Xc = X @ np.asarray(c["Rcw"], F64).T + np.asarray(c["tcw"], F64)
        with np.errstate(all="ignore"):
            uv = np.stack([FOCAL * Xc[:, 0] / Xc[:, 2] + CX, FOCAL * Xc[:, 1] / Xc[:, 2] + CY], 1)
        return Xc[:, 2], uv + rng.normal(0, noise, (n, 2)) if noise else uv
    z1, uv1 = view(c1)
    z2, uv2 = view(c2)
    perm = rng.permutation(n2)[:n] if n else np.zeros(0, int)  # feature of frame 2 that sees point i

    def frame(uv, z, where):
        x, y = rng.uniform(5, W - 5, n1), rng.uniform(5, H - 5, n1)
        depth = rng.uniform(1, 20, n1)
        x[where], y[where], depth[where] = uv[:, 0], uv[:, 1], z
        x, y = x.astype(F32), y.astype(F32)
        is_stereo = rng.random(n1) < stereo_frac
        with np.errstate(all="ignore"):
            ur = np.where(is_stereo, x - MBF / depth + (rng.normal(0, noise, n1) if noise else 0), -1.0).astype(F32)
        depth = np.where(is_stereo, depth, -1.0).astype(F32)  # mvDepth of a mono keypoint is -1
        return x, y, ur, stereo_values(x, y, depth)
    x1, y1, ur1, st1 = frame(uv1, z1, np.arange(n))
    x2, y2, ur2, st2 = frame(uv2, z2, perm)
    oct1 = rng.integers(0, NLEVELS, n1) if octaves is None else np.full(n1, octaves[0])
    oct2 = rng.integers(0, NLEVELS, n2) if octaves is None else np.full(n2, octaves[1])
    ang1 = rng.uniform(0, 360, n1).astype(F32)
    ang2 = rng.uniform(0, 360, n2).astype(F32)
    ang2[perm] = np.mod(ang1[:n] + rng.uniform(-25, 25, n).astype(F32), F32(360)).astype(F32)
    if rotated:
        ang2[perm[:rotated]] = np.mod(ang1[:rotated] + F32(90), F32(360)).astype(F32)
    d1 = rng.integers(0, 256, (n1, 32)).astype(U8)
    d2 = rng.integers(0, 256, (n2, 32)).astype(U8)
    flips = np.zeros((n, 256), U8)
    for i in range(n):
        flips[i, rng.choice(256, int(rng.integers(0, 9)), replace=False)] = 1
    d2[perm] = d1[:n] ^ np.packbits(flips, axis=1)
    matches = np.full(n1, -1, I32)
    matches[:n] = perm
    if outliers:
        who = np.arange(n - outliers, n)
        matches[who] = perm[(who + rng.integers(1, max(n - 1, 2), outliers)) % n]
    # FeatureVectors: a true pair shares its node; 12 nodes, two of them on one side only
    node1 = rng.integers(0, 10, n1)
    node2 = rng.integers(0, 10, n2)
    node2[perm] = node1[:n]
    node1[n:], node2[np.setdiff1d(np.arange(n2), perm)] = 10, 11
    ids = [2, 5, 9, 14, 15, 22, 31, 40, 41, 57, 60, 77]
    fv1 = _fv({ids[s]: np.flatnonzero(node1 == s).astype(I32) for s in range(12) if (node1 == s).any()})
    fv2 = _fv({ids[s]: np.flatnonzero(node2 == s).astype(I32) for s in range(12) if (node2 == s).any()})
    F12, ep = fundamental(c1, c2)
    P = tr.params(c1, c2, F32(1.5) * SF[1], **(P_kw or {}))
    return dict(k1=_keys(x1, y1, oct1, ang1), k2=_keys(x2, y2, oct2, ang2), d1=d1, d2=d2, ur1=ur1, ur2=ur2, stereo1=st1, stereo2=st2,
                sf1=SF, sigma2_1=SIGMA2, sf2=SF, sigma2_2=SIGMA2, nlevels=NLEVELS, P=P, matches=matches, truth=perm, fv1=fv1, fv2=fv2,
                no_mp1=np.ones(n1, U8), no_mp2=np.ones(n2, U8), F12=F12, ep=ep, n_points=n)


def cameras(baseline=0.25, yaw=2.0, mbf=MBF):
    c1 = tr.camera(rot(1, 1.0) @ rot(0, -0.5), [0.02, -0.01, 0.03], FOCAL, FOCAL, CX, CY, mbf)
    R2 = rot(1, -yaw) @ rot(2, 1.5)
    c2 = tr.camera(R2, -R2 @ np.array([baseline, 0.03, 0.02]), FOCAL, FOCAL, CX, CY, mbf)
    return c1, c2


def cloud(rng, n, zmin, zmax):
    """n points in front of camera 1 (about the world frame), log-uniform in depth, inside both images."""
    z = np.exp(rng.uniform(np.log(zmin), np.log(zmax), n))
    return np.stack([rng.uniform(-0.35, 0.35, n) * z + 0.12, rng.uniform(-0.3, 0.3, n) * z, z], 1)


@functools.lru_cache(maxsize=None)
def parity(seed=7, kf2_first=False):
    rng = np.random.default_rng(seed)
    c1, c2 = cameras(baseline=0.09)
    return build(cloud(rng, 300, 0.4, 80.0), c1, c2, rng, outliers=60, extra=24, rotated=30,
                 P_kw=dict(far_points=True, th_far_points=50.0, kf2_first=kf2_first))


@functools.lru_cache(maxsize=None)
def edge(n, seed=11):
    """n features, every one a good mono or stereo pair at depth 2 .. 6 (far inside every gate)."""
    rng = np.random.default_rng(seed + n)
    c1, c2 = cameras()
    return build(cloud(rng, n, 2.0, 6.0), c1, c2, rng, noise=0.05, octaves=(1, 1))


def edge_sets(n):
    """name -> the features of edge(n) that carry a match: none, all, and the neighbours of every wave and chunk boundary."""
    sets = {"none": np.zeros(0, int), "all": np.arange(n)}
    b = sorted({i for e in range(WAVE, n + WAVE, WAVE) for i in (e - 2, e - 1, e, e + 1) if 0 <= i < n} | {0, n - 1} - {-1})
    if n > 1:
        sets["boundaries"] = np.array(b, int)
        sets["chunk_boundaries"] = np.array([i for i in b if min(abs(i - c) for c in range(0, n + CHUNK, CHUNK)) <= 2], int)
    return sets


def with_matches(s, which):
    m = np.full(len(s["k1"]), -1, I32)
    m[which] = s["matches"][which]
    return m


def _one(P_kw=None, c=None, X=(0.3, -0.2, 4.0), **kw):
    """A scene of ONE noise-free pair."""
    c1, c2 = c or cameras()
    return build([X], c1, c2, np.random.default_rng(5), noise=0.0, P_kw=P_kw, **kw)


@functools.lru_cache(maxsize=None)
def directed():
    """name -> (scene, expected reason, expected source); every scene has one matched pair: feature 0 of frame 1."""
    out = {}

    def put(name, s, reason, source=tr.FROM_TRIANGULATE):
        out[name] = (s, reason, source)

    def mono(s):
        for t in ("1", "2"):
            s["ur" + t] = np.full(len(s["k" + t]), -1, F32)
            s["stereo" + t] = stereo_values(s["k" + t]["x"], s["k" + t]["y"], np.full(len(s["k" + t]), -1, F32))
        return s

    def stereo(s, t, i, depth, ur=None):
        k = s["k" + t]
        s["ur" + t][i] = k["x"][i] - F32(MBF) / F32(depth) if ur is None else ur
        d = np.where(s["ur" + t] >= 0, 1.0, -1.0).astype(F32)
        d[i] = depth
        old = s["stereo" + t].copy()
        s["stereo" + t] = stereo_values(k["x"], k["y"], d)
        keep = np.arange(len(k)) != i
        s["stereo" + t][keep] = old[keep]
        return s
    j = lambda s: int(s["matches"][0])  # noqa: E731  the partner of feature 0
    put("accepted_triangulate", mono(_one()), tr.ACCEPTED)
    put("accepted_triangulate_inertial", mono(_one(dict(inertial=True))), tr.ACCEPTED)
    # depth 60 against a baseline of 0.25: cos parallax about 0.99999, mono: low parallax
    put("low_parallax_mono", mono(_one(X=(1.0, -0.5, 60.0))), tr.LOW_PARALLAX)
    # the same pair, kf1's keypoint stereo at its true depth: the stereo parallax of mb = 0.1 is larger still -> Triangulate (:582)
    s = stereo(mono(_one(X=(1.0, -0.5, 60.0))), "1", 0, 60.0)
    put("far_stereo1_still_triangulates", s, tr.ACCEPTED)
    # kf1 stereo at depth 4 with a baseline of 0.02 < mb: UnprojectStereo of kf1
    near = cameras(baseline=0.02)
    put("stereo1", stereo(mono(_one(c=near)), "1", 0, 3.97), tr.ACCEPTED, tr.FROM_STEREO1)
    s = mono(_one(c=near))
    put("stereo2", stereo(s, "2", j(s), 4.0), tr.ACCEPTED, tr.FROM_STEREO2)
    # mvDepth <= 0 with mvuRight >= 0 cannot come out of ComputeStereoMatches, but the branch exists (KeyFrame.cc:888)
    s = stereo(mono(_one(c=near)), "1", 0, 4.0)
    s["stereo1"][0, 2], s["stereo1"][0, 3] = -1.0, 0.5
    put("stereo_depth", s, tr.STEREO_DEPTH, tr.FROM_STEREO1)
    # w == 0: see the module docstring
    Rx = np.array([[0, 0, 1.0], [0, 1.0, 0], [-1.0, 0, 0]])  # exact: the first column of Rz(30) Rx is (0, 0, -1) too
    cw = (tr.camera(Rx, [0, 0, 0], FOCAL, FOCAL, CX, CY, MBF), tr.camera(rot(2, 30.0) @ Rx, [0.3, 0.1, 0], FOCAL, FOCAL, CX, CY, MBF))
    s = mono(_one(c=cw))
    for t, i in (("1", 0), ("2", j(s))):
        s["k" + t]["x"][i], s["k" + t]["y"][i] = CX, CY
    s = stereo(s, "1", 0, 5.0)
    s["stereo1"][0, 3] = 2.0
    put("w_zero", s, tr.W_ZERO)
    # outliers: a partner on the other side of the image puts the intersection behind a camera
    s = mono(_one(X=(0.3, -0.2, 4.0)))
    s["k2"]["x"][j(s)] += 60.0
    put("z1_negative", s, tr.Z1)
    # kf2 stands one unit AHEAD of kf1 on its axis and the point lies between them: both rays point forward (cos > 0), the
    # intersection is in front of kf1 and behind kf2
    cz = (tr.camera(np.eye(3), [0, 0, 0], FOCAL, FOCAL, CX, CY, MBF), tr.camera(np.eye(3), [0, 0, -1.0], FOCAL, FOCAL, CX, CY, MBF))
    s = mono(_one(c=cz, X=(0.1, 0.05, 0.5)))
    put("z2_negative", s, tr.Z2)
    # reprojection: the triangulated point of a pair 8 px off the epipolar line misses both keypoints by about 4 px; a stereo
    # keypoint whose mvuRight is 12 px off fails the three-term gate of its own frame only
    s = mono(_one())
    s["k2"]["y"][j(s)] += 8.0
    put("reproj1_mono", s, tr.REPROJ1)
    s = stereo(mono(_one()), "1", 0, 4.0, ur=F32(_one()["k1"]["x"][0] - MBF / 4.0 + 12.0))
    put("reproj1_stereo", s, tr.REPROJ1)
    s = mono(_one())
    s = stereo(s, "2", j(s), 4.0, ur=F32(s["k2"]["x"][j(s)] - MBF / 4.0 + 12.0))
    put("reproj2_stereo", s, tr.REPROJ2)
    s = mono(_one(octaves=(3, 0)))  # kf1's level tolerates the 4 px that kf2's level 0 does not
    s["k2"]["y"][j(s)] += 5.0
    put("reproj2_mono", s, tr.REPROJ2)
    s = mono(_one(dict(far_points=True, th_far_points=3.0)))
    put("far", s, tr.FAR)
    put("octaves_3_0_accepted", mono(_one(octaves=(3, 0))), tr.ACCEPTED)
    s = mono(_one(octaves=(3, 0)))
    s["P"]["ratio_factor"] = F32(1.05)  # ratioDist about 1 against ratioOctave 1.728
    put("scale_ratio", s, tr.SCALE_RATIO)
    # dist == 0: Ow is an INPUT the gates read beside Rcw / tcw (the reference stores mOw).  The stereo1 pair with kf2's centre
    # handed in as the very point UnprojectStereo gives (no SVD on the way: the same bits everywhere) reaches :679 with every
    # earlier gate passed, none of which reads Ow
    s = stereo(mono(_one(c=near)), "1", 0, 3.97)
    r = restate(s, s["matches"])
    assert r["source"][0] == tr.FROM_STEREO1
    s["P"]["kf2"] = dict(s["P"]["kf2"], Ow=r["x3d"][0].copy())
    put("dist_zero", s, tr.DIST_ZERO, tr.FROM_STEREO1)
    return out


def features_of(s, t, idx):
    k = s["k" + t]
    ur = s["ur" + t]
    return [tr.feature(k["x"][i], k["y"][i], -1.0 if ur is None else ur[i], s["sf" + t][k["octave"][i]],
                       s["sigma2_" + t][k["octave"][i]], s["stereo" + t][i, 3], s["stereo" + t][i, :3]) for i in idx]


def restate(s, matches, svd="f64"):
    """The restatement over a scene's match list: per feature reason / source / x3d (255 / 0 / zeros without a match) and the
    list of per-pair results."""
    n1 = len(s["k1"])
    reason, source, x3d = np.full(n1, tr.NO_MATCH, U8), np.zeros(n1, U8), np.zeros((n1, 3), F32)
    idx = np.flatnonzero(np.asarray(matches) >= 0)
    f1, f2 = features_of(s, "1", idx), features_of(s, "2", np.asarray(matches)[idx])
    res = [tr.pair(s["P"], a, b, svd) for a, b in zip(f1, f2)]
    for i, r in zip(idx, res):
        reason[i], source[i], x3d[i] = r["reason"], r["source"], r["x3D"]
    return dict(reason=reason, source=source, x3d=x3d, idx=idx, pairs=res, f1=f1, f2=f2)


def triangulated(r):
    """Positions (into r["idx"]) of the pairs whose x3D came out of the SVD."""
    return [p for p, q in enumerate(r["pairs"]) if q["source"] == tr.FROM_TRIANGULATE and q["reason"] not in (tr.LOW_PARALLAX, tr.W_ZERO)]


def exact_x3d(A):
    """x3D of the float64 SVD of the float32 A, NOT rounded: what the deviations are measured from."""
    h = np.linalg.svd(np.asarray(A, F64))[2][3]
    return h[:3] / h[3]


def deviation(r, x3d):
    """Per triangulated pair of restate()'s r: |x3d - exact| / |exact| for per-feature float32 results x3d."""
    at = triangulated(r)
    exact = np.array([exact_x3d(r["pairs"][p]["A"]) for p in at], F64).reshape(-1, 3)
    got = np.asarray(x3d, F64)[r["idx"][at]].reshape(-1, 3)
    return np.linalg.norm(got - exact, axis=1) / np.linalg.norm(exact, axis=1)


def all_scenes():
    """(name, scene, matches) of everything the tolerance is measured over."""
    yield "parity", parity(), parity()["matches"]
    for name, (s, _, _) in directed().items():
        yield "directed/" + name, s, s["matches"]
    for n in EDGE_COUNTS:
        if n:
            yield "edge/%d" % n, edge(n), edge(n)["matches"]


@functools.lru_cache(maxsize=None)
def tolerance():
    """TOL of the module docstring and its median over the pairs."""
    dev = np.concatenate([deviation(restate(s, m), restate(s, m, "f32")["x3d"]) for _, s, m in all_scenes()])
    return float(dev.max()), float(np.median(dev))


def near(s, r, tol):
    """Per pair of restate()'s result: does a move of x3D by tol * |x3D| change the gates' reason?"""
    dirs = [np.array(d, F64) for d in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1), (1, 1, -1), (1, -1, 1), (-1, 1, 1))]
    dirs = [sg * d / np.linalg.norm(d) for d in dirs for sg in (1, -1)]
    out = np.zeros(len(r["pairs"]), bool)
    with np.errstate(all="ignore"):
        for p, q in enumerate(r["pairs"]):
            if q["source"] != tr.FROM_TRIANGULATE or q["reason"] in (tr.LOW_PARALLAX, tr.W_ZERO):
                continue
            X = q["x3D"].astype(F64)
            step = tol * np.linalg.norm(X)
            out[p] = any(tr.gates(s["P"], r["f1"][p], r["f2"][p], (X + step * d).astype(F32), {}) != q["reason"] for d in dirs)
    return out


if __name__ == "__main__":
    import sys
    from pathlib import Path
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    import triangulation_hostcore as hc
    tol, med = tolerance()
    worst, worst_double, pairs = 0.0, 0.0, 0
    for name, s, m in all_scenes():
        r, h = restate(s, m), hc.loop(s, m)
        at = triangulated(r)
        if at:
            worst = max(worst, float(deviation(r, h["x3d"]).max()))
            v = hc.null_vectors(np.stack([r["pairs"][p]["A"] for p in at]))
            exact = np.array([exact_x3d(r["pairs"][p]["A"]) for p in at])
            d = np.linalg.norm(v[:, :3] / v[:, 3:] - exact, axis=1) / np.linalg.norm(exact, axis=1)
            worst_double, pairs = max(worst_double, float(d.max())), pairs + len(at)
    print("triangulated pairs: %d" % pairs)
    print("TOL (float32 SVD against the unrounded float64 SVD): %.3g of |x3D| (median %.3g)" % (tol, med))
    print("header's x3D against the same:                      %.3g of |x3D|" % worst)
    print("header's double null vector, before rounding:       %.3g of |x3D|" % worst_double)
