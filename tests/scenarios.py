"""Seeded search scenarios for the routine-level matcher tests (CPU: oracle vs oracle, GPU: HIP vs oracle).

Features come from the CPU oracle extractor on synthetic frames (cached per process); the "projections" are the
keypoints of a neighbouring frame moved by the known translation plus noise -- what Tracking's geometry would hand the
matcher -- with every knob of the routines exercised: blocked features, stereo coordinates, level windows, empty
windows, far-off points, duplicate targets."""
import functools

import numpy as np

import oracle_lib as ol
from visual_sgraphs_amd import synth

SCALE = np.float32(1.2) ** np.arange(8, dtype=np.float32)
_T = ol.OracleExtractor(1000, 1.2, 8, 20, 7).tables()
SCALE_FACTORS = _T["scale"]          # mvScaleFactors
INV_SIGMA2 = _T["inv_sigma2"]        # mvInvLevelSigma2
# The camera the scenario frames are seen through: "image" = no distortion (mDistCoef(0) == 0: mvKeysUn =
# mvKeys, bounds = the image rectangle), "tum1" / "d435i" = the two BASELINE cameras whose Frame constructor really
# undistorts (config/RGB-D/TUM1.yaml, config/RGB-D-Inertial/RealSense_D435i.yaml, scaled to the 320x240 scenario frames):
# keys = mvKeysUn through oracle/undistort_oracle.cpp, BOUNDS = Frame::ComputeImageBounds -- fractional, negative
# (D435i) or inside the image (TUM1: features near the edge fall outside the grid).  use_camera() switches all of it.
W, H = 320, 240
CAMERA_NAMES = ("image", "tum1", "d435i")
CAMERA = "image"
CAM = None                        # oracle_lib camera dict of the current camera (None: no distortion)
BOUNDS = (0.0, 0.0, float(W), float(H))


def use_camera(name, w=W, h=H):
    """(w, h): the size of the frames the camera is scaled to (the builders below take the same pair)."""
    global CAMERA, CAM, BOUNDS
    assert name in CAMERA_NAMES
    CAMERA = name
    CAM = None if name == "image" else ol.scaled_camera(name, w, h)
    BOUNDS = (0.0, 0.0, float(w), float(h)) if CAM is None else ol.image_bounds(CAM)


@functools.lru_cache(maxsize=None)
def features_raw(seed, t, w=W, h=H, nfeat=600):
    """(mvKeys, mDescriptors) of the oracle extractor on a scenario frame."""
    ex = ol.OracleExtractor(nfeat, 1.2, 8, 20, 7)
    _, k, d = ex(synth.sequence_frame(w, h, seed, t))
    return k, d


@functools.lru_cache(maxsize=None)
def _features_un(camera, seed, t, w, h, nfeat):
    k, d = features_raw(seed, t, w, h, nfeat)
    return ol.undistort_keypoints(k, ol.scaled_camera(camera, w, h)), d


def features(seed, t, w=W, h=H, nfeat=600):
    """(mvKeysUn, mDescriptors) under the current camera (Frame::UndistortKeyPoints, Frame.cc:891-921)."""
    if CAMERA == "image":
        return features_raw(seed, t, w, h, nfeat)
    return _features_un(CAMERA, seed, t, w, h, nfeat)


def stereo_pair(seed, w=W, h=H, nfeat=600):
    """Fisheye-stereo style frame: mvKeys || mvKeysRight, descriptors vconcat'ed, Nleft (Frame.cc:296)."""
    kl, dl = features(seed, 0, w, h, nfeat)
    kr, dr = features(seed, 1, w, h, nfeat)
    return np.concatenate([kl, kr]), np.concatenate([dl, dr]), len(kl)


def u_right_for(kps, rng, frac=0.6):
    """mvuRight: -1 for monocular points, x - disparity for the rest."""
    ur = np.full(len(kps), -1.0, np.float32)
    m = rng.random(len(kps)) < frac
    ur[m] = kps["x"][m] - rng.uniform(1.0, 30.0, m.sum()).astype(np.float32)
    return ur


def projections(rng, src_kps, shift=(-3.0, -2.0), noise=1.5, n_far=20, bounds=None):
    """(u, v) of the source keypoints in the target frame + a few points far from any feature / outside the image."""
    bounds = BOUNDS if bounds is None else bounds
    n = len(src_kps)
    u = src_kps["x"] + np.float32(shift[0]) + rng.normal(0, noise, n).astype(np.float32)
    v = src_kps["y"] + np.float32(shift[1]) + rng.normal(0, noise, n).astype(np.float32)
    far = rng.choice(n, min(n_far, n), replace=False)
    u[far] = rng.uniform(bounds[0] - 40, bounds[2] + 40, len(far)).astype(np.float32)
    v[far] = rng.uniform(bounds[1] - 40, bounds[3] + 40, len(far)).astype(np.float32)
    return u.astype(np.float32), v.astype(np.float32)


def noisy_desc(rng, desc, flip_bits=12):
    """Map-point descriptors: the source frame's descriptors with a few bits flipped."""
    d = desc.copy()
    for _ in range(flip_bits):
        rows = np.arange(len(d))
        byte = rng.integers(0, 32, len(d))
        bit = rng.integers(0, 8, len(d))
        flip = rng.random(len(d)) < 0.5
        d[rows[flip], byte[flip]] ^= (1 << bit[flip]).astype(np.uint8)
    return d


def local_map_scenario(seed, stereo2=False, w=W, h=H, nfeat=600):
    """Inputs of SearchByProjection(F, vpMapPoints, th) (ORBmatcher.cc:42-216)."""
    rng = np.random.default_rng(seed)
    if stereo2:
        keys, desc, nleft = stereo_pair(seed, w, h, nfeat)
        ur = None
    else:
        keys, desc = features(seed, 1, w, h, nfeat)
        nleft = -1
        ur = u_right_for(keys, rng)
    src_k, src_d = features(seed, 0, w, h, nfeat)
    n = len(src_k)
    u, v = projections(rng, src_k)
    mp = dict(desc=noisy_desc(rng, src_d), observed=(rng.random(n) < 0.8).astype(np.uint8),
              in_view=(rng.random(n) < 0.9).astype(np.uint8), proj_x=u, proj_y=v,
              proj_xr=(u - rng.uniform(1, 30, n)).astype(np.float32),
              scale_level=np.clip(src_k["octave"] + rng.integers(-1, 2, n), 0, 7).astype(np.int32),
              view_cos=rng.choice(np.array([0.9, 0.9985, 0.9999], np.float32), n))
    ltr = rtl = None
    if stereo2:
        ur2, vr2 = projections(rng, src_k, shift=(-3.0 + 8.0, -2.0))
        lvl_r = np.clip(src_k["octave"] + rng.integers(-1, 2, n), 0, 7).astype(np.int32)
        lvl_r[rng.random(n) < 0.05] = -1
        mp.update(in_view_r=(rng.random(n) < 0.7).astype(np.uint8), proj_x_r=ur2, proj_y_r=vr2, scale_level_r=lvl_r,
                  view_cos_r=rng.choice(np.array([0.9, 0.9999], np.float32), n))
        nr = len(keys) - nleft
        ltr = np.full(nleft, -1, np.int32)
        rtl = np.full(nr, -1, np.int32)
        pairs = rng.choice(min(nleft, nr), min(nleft, nr) // 3, replace=False)
        perm = rng.permutation(pairs)
        ltr[pairs] = perm
        rtl[perm] = pairs
    blocked = (rng.random(len(keys)) < 0.1).astype(np.uint8)
    th = float(rng.choice([1.0, 3.0, 5.0]))
    return dict(keys=keys, desc=desc, nleft=nleft, u_right=ur, mp=mp, th=th, nnratio=0.8, blocked=blocked, ltr=ltr,
                rtl=rtl)


def last_frame_scenario(seed, stereo2=False, w=W, h=H, nfeat=600):
    """Inputs of SearchByProjection(CurrentFrame, LastFrame, th, bMono) (ORBmatcher.cc:1667-1878)."""
    rng = np.random.default_rng(seed + 1000)
    if stereo2:
        keys, desc, nleft = stereo_pair(seed, w, h, nfeat)
        ur_frame = None
    else:
        keys, desc = features(seed, 1, w, h, nfeat)
        nleft = -1
        ur_frame = u_right_for(keys, rng)
    src_k, src_d = features(seed, 0, w, h, nfeat)
    n = len(src_k)
    u, v = projections(rng, src_k)
    out = dict(keys=keys, desc=desc, nleft=nleft, u_right=ur_frame, q_desc=noisy_desc(rng, src_d),
               observed=(rng.random(n) < 0.7).astype(np.uint8), u=u, v=v,
               ur=(u - rng.uniform(1, 30, n)).astype(np.float32), octave=src_k["octave"].astype(np.int32),
               angle=src_k["angle"].astype(np.float32), th=float(rng.choice([7.0, 15.0])),
               direction=int(rng.integers(0, 3)), blocked=(rng.random(len(keys)) < 0.1).astype(np.uint8), u_r=None,
               v_r=None)
    if stereo2:
        out["u_r"], out["v_r"] = projections(rng, src_k, shift=(-3.0 + 8.0, -2.0))
    return out


def kf_projection_scenario(seed, w=W, h=H, nfeat=600):
    """Per-point inputs shared by the best-only routines: SearchByProjection(KF, Sim3) x2, (F, KF, sAlreadyFound),
    SearchBySim3, Fuse x2."""
    rng = np.random.default_rng(seed + 2000)
    keys, desc = features(seed, 1, w, h, nfeat)
    src_k, src_d = features(seed, 0, w, h, nfeat)
    n = len(src_k)
    u, v = projections(rng, src_k)
    level = np.clip(src_k["octave"] + rng.integers(-1, 2, n), 0, 7).astype(np.int32)
    th = float(rng.choice([3.0, 4.0, 10.0]))
    radius = (np.float32(th) * SCALE_FACTORS[level]).astype(np.float32)
    return dict(keys=keys, desc=desc, u_right=u_right_for(keys, rng), q_desc=noisy_desc(rng, src_d, 8), u=u, v=v,
                ur=(u - rng.uniform(1, 30, n)).astype(np.float32), level=level, radius=radius,
                angle=src_k["angle"].astype(np.float32), src_k=src_k, src_d=src_d, rng=rng)


# ---------------------------------------------------------------------------------------------- synthetic frames
# Frames that do not go through the extractor: sizes, cell occupancies, octaves and descriptors are chosen, so that the
# size-dependent paths of k_frame_grid_build / k_window_search are reached on purpose (tests/test_gpu_frame_edges.py;
# tests/test_frame_edge_scenarios.py asserts on the CPU that they are).
GRID_COLS, GRID_ROWS = 64, 48        # FRAME_GRID_COLS / ROWS (Frame.h:49-50)
_T16 = ol.OracleExtractor(1000, 1.2, 16, 20, 7).tables()
SCALE_FACTORS16 = _T16["scale"]      # a 16-level pyramid: octaves 0-15 fill the 4-bit field of the packed candidates
INV_SIGMA2_16 = _T16["inv_sigma2"]
HD_BOUNDS = (0.0, 0.0, 1280.0, 720.0)
TUM1_LIKE = (11.5, 9.25, 1268.75, 707.5)     # inside the image (TUM1 at 1280x720 undistorts inwards)
D435I_LIKE = (-14.375, -9.5, 1297.25, 731.125)  # negative minima (D435i)


def cell_size(bounds):
    return (bounds[2] - bounds[0]) / GRID_COLS, (bounds[3] - bounds[1]) / GRID_ROWS


def cell_centre(bounds, px, py):
    """PosInGrid rounds (x - mnMinX) * inv: cell px collects x in [mnMinX + (px - .5) cw, mnMinX + (px + .5) cw)."""
    cw, ch = cell_size(bounds)
    return bounds[0] + px * cw, bounds[1] + py * ch


def _in_cells(rng, bounds, cells, counts):
    cw, ch = cell_size(bounds)
    xs, ys = [], []
    for (px, py), m in zip(cells, counts):
        cx, cy = cell_centre(bounds, px, py)
        xs.append(cx + rng.uniform(-0.45, 0.45, m) * cw)
        ys.append(cy + rng.uniform(-0.45, 0.45, m) * ch)
    return np.concatenate(xs) if xs else np.zeros(0), np.concatenate(ys) if ys else np.zeros(0)


def cluster_cells(rng, k):
    """k cells at least 3 apart from each other and 2 from the border."""
    cells = []
    while len(cells) < k:
        c = (int(rng.integers(2, GRID_COLS - 2)), int(rng.integers(2, GRID_ROWS - 2)))
        if all(max(abs(c[0] - d[0]), abs(c[1] - d[1])) >= 3 for d in cells):
            cells.append(c)
    return cells


def synthetic_frame(seed, n, law="uniform", bounds=HD_BOUNDS, max_octave=15, ur_share=None, nleft=-1, clusters=12,
                    cluster_sizes=(33, 200)):
    """n keypoints under a spatial law, octaves 0..max_octave, random angles and descriptors.
    law: "uniform" (a few per cent outside the bounds); "clustered": `clusters` cells of cluster_sizes entries, at least three
    cells apart (the first of exactly 33, the second of exactly 32: the two sides of the kernel's per-cell survivor mask,
    far enough apart for a window to hold the 32-entry cell without any larger one), their 8 neighbours 0-3 each, the rest
    uniform elsewhere; "one_cell"; "lattice": on cell boundaries (PosInGrid's round-half-away) and on the four bounds
    (px == 64 / py == 48 are rejected).  ur_share = (share of -1, share of exact 0.0) of mvuRight (None: no mvuRight).
    nleft != -1: the first nleft are the left camera's, the rest the right's (each under the same law).
    Returns dict(keys, desc, u_right, nleft, bounds, cells) -- cells: the cluster cells."""
    rng = np.random.default_rng(seed)
    cw, ch = cell_size(bounds)
    cells = []

    def place(m):
        if m == 0:
            return np.zeros(0), np.zeros(0)
        if law == "uniform":
            return (rng.uniform(bounds[0] - 0.02 * cw * GRID_COLS, bounds[2] + 0.02 * cw * GRID_COLS, m),
                    rng.uniform(bounds[1] - 0.02 * ch * GRID_ROWS, bounds[3] + 0.02 * ch * GRID_ROWS, m))
        if law == "one_cell":
            return _in_cells(rng, bounds, [(20, 17)], [m])
        if law == "lattice":
            # half-cell lattice: every second value is a cell boundary; the last column / row are the maxima
            ix, iy = rng.integers(-1, 2 * GRID_COLS + 1, m), rng.integers(-1, 2 * GRID_ROWS + 1, m)
            return bounds[0] + ix * (cw / 2), bounds[1] + iy * (ch / 2)
        assert law == "clustered"
        cs = cluster_cells(rng, clusters)
        cells.append(cs)
        sizes = rng.integers(cluster_sizes[0], cluster_sizes[1] + 1, len(cs))
        sizes[0], sizes[1] = 33, 32
        sizes[-1] = cluster_sizes[1]
        while sizes.sum() > 0.8 * m and sizes.max() > 40:   # small frames: shrink the largest cluster
            sizes[np.argmax(sizes)] = 40
        near = [(c[0] + dx, c[1] + dy) for c in cs for dx in (-1, 0, 1) for dy in (-1, 0, 1) if (dx, dy) != (0, 0)]
        near_counts = rng.integers(0, 4, len(near))
        near_counts[0:8] = np.maximum(near_counts[0:8], 1)
        x0, y0 = _in_cells(rng, bounds, cs, sizes)
        x1, y1 = _in_cells(rng, bounds, near, near_counts)
        rest = m - len(x0) - len(x1)
        assert rest >= 0, "frame too small for its clusters"
        taken = set(cs) | set(near)
        free = [(a, b) for a in range(GRID_COLS) for b in range(GRID_ROWS) if (a, b) not in taken]
        pick = rng.integers(0, len(free), rest)
        x2, y2 = _in_cells(rng, bounds, [free[i] for i in pick], [1] * rest)
        order = rng.permutation(m)   # cluster members are spread over the index range
        return np.concatenate([x0, x1, x2])[order], np.concatenate([y0, y1, y2])[order]

    nl = n if nleft == -1 else nleft
    xl, yl = place(nl)
    xr, yr = place(n - nl)
    k = np.zeros(n, ol.KP_DTYPE)
    k["x"], k["y"] = np.concatenate([xl, xr]), np.concatenate([yl, yr])
    k["octave"] = rng.integers(0, max_octave + 1, n)
    k["angle"] = rng.uniform(0, 360, n)
    k["size"] = 31.0
    k["response"] = rng.uniform(10, 100, n)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    ur = None
    if ur_share is not None:
        ur = (k["x"] - rng.uniform(1.0, 30.0, n)).astype(np.float32)
        p = rng.random(n)
        ur[p < ur_share[0]] = -1.0
        ur[(p >= ur_share[0]) & (p < ur_share[0] + ur_share[1])] = 0.0
    return dict(keys=k, desc=desc, u_right=ur, nleft=nleft, bounds=tuple(float(b) for b in bounds),
                cells=cells[0] if cells else [])


def flipped_desc(rng, desc, kind):
    """kind >= 0: that many distinct bits flipped; -1: the complement (distance 256); -2: the complement with one bit
    restored (255)."""
    d = desc.copy()
    if kind < 0:
        d = ~d
        if kind == -2:
            d[int(rng.integers(0, 32))] ^= np.uint8(1 << int(rng.integers(0, 8)))
        return d
    for b in rng.choice(256, kind, replace=False):
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def synthetic_queries(seed, fr, nq, radius=(0.3, 60.0), right=False, max_level=15, on_keys=0.6):
    """nq window queries against a synthetic_frame: centres on keypoints (share on_keys: on the clusters where the frame
    has them), between them, on the bounds and outside; radii log-uniform in `radius`; predicted levels near the source
    keypoint's octave; descriptors = the source keypoint's with 0-40 bits flipped, its complement or complement + 1 bit."""
    rng = np.random.default_rng(seed + 5000)
    k, d, b = fr["keys"], fr["desc"], fr["bounds"]
    lo_i, hi_i = (0, len(k)) if fr["nleft"] == -1 else ((fr["nleft"], len(k)) if right else (0, fr["nleft"]))
    have = hi_i > lo_i
    src = rng.integers(lo_i, hi_i, nq) if have else np.zeros(nq, np.int64)
    kind = rng.random(nq)
    u = rng.uniform(b[0], b[2], nq)
    v = rng.uniform(b[1], b[3], nq)
    if have:
        on = kind < on_keys
        u[on] = k["x"][src[on]] + rng.normal(0, 2.0, on.sum())
        v[on] = k["y"][src[on]] + rng.normal(0, 2.0, on.sum())
    edge = kind > 0.92
    u[edge] = rng.choice([b[0], b[2], b[0] - 25.0, b[2] + 25.0], edge.sum())
    r = np.exp(rng.uniform(np.log(radius[0]), np.log(radius[1]), nq))
    level = np.clip((k["octave"][src] if have else 0) + rng.integers(-1, 2, nq), 0, max_level).astype(np.int32)
    level[rng.random(nq) < 0.03] = -1   # nPredictedLevel of a point that is skipped
    qd = np.zeros((nq, 32), np.uint8)
    for i in range(nq):
        base = d[src[i]] if have else rng.integers(0, 256, 32, dtype=np.uint8)
        p = rng.random()
        qd[i] = flipped_desc(rng, base, -1 if p < 0.04 else -2 if p < 0.08 else int(rng.integers(0, 41)))
    uf = u.astype(np.float32)
    return dict(u=uf, v=v.astype(np.float32), radius=r.astype(np.float32), level=level, q_desc=qd, src=src.astype(np.int32),
                ur=(uf - rng.uniform(1, 30, nq)).astype(np.float32), angle=rng.uniform(0, 360, nq).astype(np.float32),
                observed=(rng.random(nq) < 0.7).astype(np.uint8), in_view=(rng.random(nq) < 0.9).astype(np.uint8),
                view_cos=rng.choice(np.array([0.9, 0.9985, 0.9999], np.float32), nq), rng=rng)


def window_cells(bounds, x, y, r):
    """Cells of Frame::GetFeaturesInArea's window (Frame.cc:810-832) in float arithmetic: (count, x0, x1, y0, y1);
    count 0 when the function returns early."""
    f = np.float32
    b = [f(v) for v in bounds]
    iw, ih = f(GRID_COLS) / (b[2] - b[0]), f(GRID_ROWS) / (b[3] - b[1])
    x, y, r = f(x), f(y), f(r)
    with np.errstate(all="ignore"):
        vals = [np.floor((x - b[0] - r) * iw), np.ceil((x - b[0] + r) * iw), np.floor((y - b[1] - r) * ih),
                np.ceil((y - b[1] + r) * ih)]
    if not all(np.isfinite(v) and abs(v) < 2 ** 31 for v in vals):
        return 0, 0, -1, 0, -1
    x0, x1, y0, y1 = max(0, int(vals[0])), min(GRID_COLS - 1, int(vals[1])), max(0, int(vals[2])), min(GRID_ROWS - 1, int(vals[3]))
    if x0 >= GRID_COLS or x1 < 0 or y0 >= GRID_ROWS or y1 < 0 or x1 < x0 or y1 < y0:
        return 0, x0, x1, y0, y1
    return (x1 - x0 + 1) * (y1 - y0 + 1), x0, x1, y0, y1


def cell_of_features(cell_start, entries, n):
    """cell index of every feature of an OracleFrame.grid() (-1: not in the grid)."""
    out = np.full(n, -1, np.int64)
    out[entries] = np.repeat(np.arange(GRID_COLS * GRID_ROWS), np.diff(cell_start))
    return out


def chunk_mix(bounds, cell_start, cell_of, x, y, r, survivors):
    """How one window walks the grid in chunks of 64 cells (ix outer, iy inner): returns (passes_big, mixed) --
    survivors in a cell of more than 32 entries; a chunk holding such a cell AND cells of 1-32 entries, survivors in both."""
    cnt, x0, x1, y0, y1 = window_cells(bounds, x, y, r)
    if cnt == 0 or len(survivors) == 0:
        return False, False
    occ = np.diff(cell_start)
    cells = np.array([ix * GRID_ROWS + iy for ix in range(x0, x1 + 1) for iy in range(y0, y1 + 1)])
    alive = np.zeros(GRID_COLS * GRID_ROWS, bool)
    alive[cell_of[survivors]] = True
    big_any = mixed = False
    for c0 in range(0, len(cells), 64):
        ch = cells[c0:c0 + 64]
        big = occ[ch] > 32
        b_alive = bool(np.any(alive[ch] & big))
        s_alive = bool(np.any(alive[ch] & ~big))
        big_any |= b_alive
        mixed |= b_alive and s_alive and bool(big.any())
    return big_any, mixed


# ---------------------------------------------------------------------------------------------- edge cases + reach
# Every case of tests/test_gpu_frame_edges.py is built here together with its reach condition: reach_*() asserts, on the
# oracle's grid() / features_in_area() alone, that the inputs really hit the kernel path the case is named after.  The GPU
# test calls it before comparing; tests/test_frame_edge_scenarios.py calls it on the CPU.
def oracle_of(fr):
    return ol.OracleFrame(fr["keys"], fr["desc"], fr["bounds"], fr["u_right"], fr["nleft"])


def occupancy(o, right=False):
    return np.diff(o.grid(right)[0])


@functools.lru_cache(maxsize=None)
def device_image_features(w=1280, h=720, nfeat=6000, seq=21):
    """(image, mvKeys, descriptors) of a frame that yields more than kGridLdsMax + 100 keypoints."""
    img = synth.sequence_frame(w, h, seq, 0)
    _, k, d = ol.OracleExtractor(nfeat, 1.2, 8, 20, 7)(img)
    return img, k, d


DEVICE_NS = (1, 1023, 1024, 1025, 4095, 4096, 4097, None)   # None: every keypoint of the image


def reach_device_grid(o, n):
    """n > 4096: the global-memory insertion sort has work to do."""
    occ = occupancy(o)
    if n > 4096:
        assert (occ >= 2).sum() >= 30 and occ.max() >= 8, (n, int((occ >= 2).sum()), int(occ.max()))
    return occ


def densest_windows(o, bounds, nq=24):
    """windows over the densest cells of a grid: (x, y, r)"""
    occ = occupancy(o)
    top = np.argsort(-occ, kind="stable")[:nq]
    cw, ch = cell_size(bounds)
    xy = np.array([cell_centre(bounds, c // GRID_ROWS, c % GRID_ROWS) for c in top], np.float32)
    r = (np.float32(0.6) + np.arange(nq, dtype=np.float32) % 4) * np.float32(max(cw, ch))
    return xy[:, 0].copy(), xy[:, 1].copy(), r.astype(np.float32)


@functools.lru_cache(maxsize=None)
def dense_case(stereo):
    """(frame, queries) of section b: clustered cells of up to 200 entries; stereo: both halves clustered, no mvuRight."""
    if stereo:
        fr = synthetic_frame(31, 5000, "clustered", nleft=2400)
    else:
        fr = synthetic_frame(30, 3000, "clustered", bounds=TUM1_LIKE, ur_share=(0.3, 0.1))
    q, qr = synthetic_queries(30 + stereo, fr, 400, right=False), synthetic_queries(40 + stereo, fr, 400, right=True)
    # windows over the whole of a cell of exactly 32 entries with no larger cell in them: every entry survives (the routines
    # without a level filter), so bit 31 of the kernel's per-cell survivor mask is used
    cw, ch = cell_size(fr["bounds"])
    for qq, right in ((q, False), (qr, True)):
        full = np.nonzero(occupancy(oracle_of(fr), right) == 32)[0]
        for j in range(4 if len(full) else 0):
            c = int(full[0])
            qq["u"][j], qq["v"][j] = cell_centre(fr["bounds"], c // GRID_ROWS, c % GRID_ROWS)
            qq["radius"][j] = (0.75 + 0.25 * j) * max(cw, ch)
            qq["level"][j] = max(int(qq["level"][j]), 1)
    return fr, q, qr


def reach_dense(fr, q, right):
    o = oracle_of(fr)
    cs, en = o.grid(right)
    nloc = len(fr["keys"]) if fr["nleft"] == -1 else (len(fr["keys"]) - fr["nleft"] if right else fr["nleft"])
    cof = cell_of_features(cs, en, nloc)
    occ = np.diff(cs)
    assert occ.max() >= 100 and (occ == 32).any() and (occ == 33).any()
    nbig = nmix = nfull = 0
    for i in range(len(q["u"])):
        s = o.features_in_area(q["u"][i], q["v"][i], q["radius"][i], right=right, kf_form=True)
        cnt, x0, x1, y0, y1 = window_cells(fr["bounds"], q["u"][i], q["v"][i], q["radius"][i])
        if 0 < cnt <= 64 and len(s):   # one chunk without a cell of more than 32 entries: the mask path
            inwin = [ix * GRID_ROWS + iy for ix in range(x0, x1 + 1) for iy in range(y0, y1 + 1)]
            if occ[inwin].max() == 32:
                kept = np.bincount(cof[s], minlength=len(occ))
                nfull += int(np.any((kept == 32) & (occ == 32)))   # the list holds all 32 entries of such a cell
        big, mixed = chunk_mix(fr["bounds"], cs, cof, q["u"][i], q["v"][i], q["radius"][i], s)
        nbig += big
        nmix += mixed
    assert nbig >= 20 and nmix >= 1 and nfull >= 1, (nbig, nmix, nfull)
    return nbig, nmix


@functools.lru_cache(maxsize=None)
def find_windows(bounds, target, seed, count=3):
    """(x, y, r) of `count` windows of exactly `target` cells (the all-cells window: a radius larger than the image)."""
    rng = np.random.default_rng(seed)
    m = 1000000   # (129 = 43 x 3 cells needs a window clipped by the top or bottom bound: centres far outside)
    x = rng.uniform(bounds[0] - 700, bounds[2] + 700, m).astype(np.float32)
    y = rng.uniform(bounds[1] - 700, bounds[3] + 700, m).astype(np.float32)
    r = np.exp(rng.uniform(np.log(5.0), np.log(3.0 * (bounds[2] - bounds[0])), m)).astype(np.float32)
    f = np.float32
    b = [f(v) for v in bounds]
    iw, ih = f(GRID_COLS) / (b[2] - b[0]), f(GRID_ROWS) / (b[3] - b[1])
    x0 = np.maximum(0, np.floor((x - b[0] - r) * iw)).astype(np.int64)
    x1 = np.minimum(GRID_COLS - 1, np.ceil((x - b[0] + r) * iw)).astype(np.int64)
    y0 = np.maximum(0, np.floor((y - b[1] - r) * ih)).astype(np.int64)
    y1 = np.minimum(GRID_ROWS - 1, np.ceil((y - b[1] + r) * ih)).astype(np.int64)
    ok = (x0 < GRID_COLS) & (x1 >= 0) & (y0 < GRID_ROWS) & (y1 >= 0) & (x1 >= x0) & (y1 >= y0)
    cnt = np.where(ok, (x1 - x0 + 1) * (y1 - y0 + 1), 0)
    hit = np.nonzero(cnt == target)[0][:count]
    assert len(hit) == count, (target, len(hit))
    return x[hit], y[hit], r[hit]


LARGE_WINDOW_CELLS = (65, 128, 129, GRID_COLS * GRID_ROWS)


@functools.lru_cache(maxsize=None)
def large_window_case(n):
    """section c: a uniform frame of n features and windows of 65, 128, 129 and all 3072 cells, between small ones."""
    fr = synthetic_frame(50 + n % 7, n, "uniform", bounds=D435I_LIKE if n > 5000 else HD_BOUNDS)
    q = synthetic_queries(51, fr, 40, radius=(0.5, 30.0))
    at = 3
    for t in LARGE_WINDOW_CELLS:
        x, y, r = find_windows(fr["bounds"], t, 52 + t)
        for j in range(len(x)):
            q["u"][at], q["v"][at], q["radius"][at] = x[j], y[j], r[j]
            q["level"][at] = max(int(q["level"][at]), 0)
            at += 3
    return fr, q


def reach_large_windows(fr, q):
    cells = [window_cells(fr["bounds"], q["u"][i], q["v"][i], q["radius"][i])[0] for i in range(len(q["u"]))]
    for t in LARGE_WINDOW_CELLS:
        assert cells.count(t) >= 3, (t, cells)
    assert max(q["radius"]) > fr["bounds"][2] - fr["bounds"][0]
    return cells


INLINE_LENGTHS = (17, 0, 200, 16, 1, 18, 15, 250, 16, 17, 0, 33, 15, 18, 1, 64)


@functools.lru_cache(maxsize=None)
def inline_case():
    """section d: 16 spots three cells apart holding exactly INLINE_LENGTHS keypoints of octave 3 within a pixel of their
    centre, and one query of radius 3 px per spot: the lists have exactly those lengths, short and long interleaved."""
    rng = np.random.default_rng(60)
    n = sum(INLINE_LENGTHS)
    k = np.zeros(n, ol.KP_DTYPE)
    spot = np.repeat(np.arange(len(INLINE_LENGTHS)), INLINE_LENGTHS)
    order = rng.permutation(n)
    spot = spot[order]
    cx = np.array([cell_centre(HD_BOUNDS, 3 + 3 * j, 5 + 2 * j)[0] for j in range(len(INLINE_LENGTHS))])
    cy = np.array([cell_centre(HD_BOUNDS, 3 + 3 * j, 5 + 2 * j)[1] for j in range(len(INLINE_LENGTHS))])
    k["x"], k["y"] = cx[spot] + rng.uniform(-1, 1, n), cy[spot] + rng.uniform(-1, 1, n)
    k["octave"], k["angle"], k["size"] = 3, rng.uniform(0, 360, n), 31.0
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    fr = dict(keys=k, desc=desc, u_right=None, nleft=-1, bounds=HD_BOUNDS, cells=[])
    nq = len(INLINE_LENGTHS)
    qd = np.zeros((nq, 32), np.uint8)
    for j in range(nq):
        members = np.nonzero(spot == j)[0]
        qd[j] = flipped_desc(rng, desc[members[-1]], 9) if len(members) else desc[0]
    q = dict(u=cx.astype(np.float32), v=cy.astype(np.float32), radius=np.full(nq, 3.0, np.float32),
             level=np.full(nq, 3, np.int32), q_desc=qd, angle=rng.uniform(0, 360, nq).astype(np.float32),
             observed=np.ones(nq, np.uint8))
    return fr, q


def reach_inline(fr, q):
    o = oracle_of(fr)
    lens = [len(o.features_in_area(q["u"][i], q["v"][i], q["radius"][i], kf_form=True)) for i in range(len(q["u"]))]
    assert tuple(lens) == INLINE_LENGTHS
    assert {0, 1, 15, 16, 17, 18} <= set(lens) and max(lens) >= 200
    # the same lists through the level window SearchByProjection_Last gives them (octave 3 +- 1)
    lens2 = [len(o.features_in_area(q["u"][i], q["v"][i], q["radius"][i], 2, 4)) for i in range(len(q["u"]))]
    assert lens2 == lens
    return lens


@functools.lru_cache(maxsize=None)
def packed_case(n):
    """section f: a uniform frame of n (16385 / 32767) features, octaves 0-15, and local-map points aimed at its LAST
    features (index n - 1 ...) at their own octave: complements (256), complements with one bit back (255), near copies."""
    fr = synthetic_frame(70, n, "uniform", bounds=HD_BOUNDS)
    k = fr["keys"]
    k["octave"][n - 1] = 15
    k["octave"][16384] = 15
    rng = np.random.default_rng(71)
    src = np.concatenate([[n - 1, 16384, n - 1, 16384], rng.integers(16384, n, 60), rng.integers(0, n, 60)]).astype(np.int64)
    src[4:34] = src[4:34][np.argsort(-k["octave"][src[4:34]], kind="stable")]
    nq = len(src)
    kinds = [-1, -1, -2, -2] + [(-1, -2, 5, 20)[i % 4] for i in range(nq - 4)]
    qd = np.stack([flipped_desc(rng, fr["desc"][s], kd) for s, kd in zip(src, kinds)])
    inside = (k["x"][src] > 1) & (k["x"][src] < 1279) & (k["y"][src] > 1) & (k["y"][src] < 719)
    mp = dict(desc=qd, observed=(rng.random(nq) < 0.8).astype(np.uint8), in_view=np.ones(nq, np.uint8),
              proj_x=(k["x"][src] + rng.normal(0, 1.0, nq)).astype(np.float32),
              proj_y=(k["y"][src] + rng.normal(0, 1.0, nq)).astype(np.float32),
              proj_xr=np.zeros(nq, np.float32), scale_level=k["octave"][src].astype(np.int32),
              view_cos=np.full(nq, 0.9, np.float32))
    return fr, mp, src, np.array(kinds), inside


def reach_packed(fr, mp, src, kinds, inside):
    """per the oracle: one list holds index n - 1, an index >= 16384, octave 15 and the source at distance 255 / 256"""
    o = oracle_of(fr)
    n = len(fr["keys"])
    hit = 0
    for i in range(4):
        r = np.float32(4.0) * np.float32(3.0) * SCALE_FACTORS16[mp["scale_level"][i]]
        lvl = int(mp["scale_level"][i])
        lst = o.features_in_area(mp["proj_x"][i], mp["proj_y"][i], r, lvl - 1, lvl)
        assert src[i] in lst and len(lst) >= 2 and lst.max() >= 16384, (i, lst)
        assert fr["keys"]["octave"][src[i]] == 15 and (fr["keys"]["octave"][lst] == 15).any()
        d = int(np.unpackbits(mp["desc"][i] ^ fr["desc"][src[i]]).sum())
        assert d == (256 if kinds[i] == -1 else 255)
        hit += int(src[i] == n - 1)
    assert hit >= 2
    return True
