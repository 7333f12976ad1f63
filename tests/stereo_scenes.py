"""Directed scenes for Frame::ComputeStereoMatches at 320 x 240, 4 levels at scale 1.2 (the smallest geometry at which
levelL +- 1, the top level and fractional level coordinates all exist).  Checked on the CPU by tests/test_stereo_reference.py
(restatement against the oracle, and every directed case against the reason it was built for) before tests/
test_gpu_stereo_edges.py sends them through the three device entry points.

A scene is a dict: L, R (level-0 images), kl, dl, kr, dr (hand-made or edited keypoints / descriptors), mb, mbf, and `cases`:
a list of (left index, check, argument) the restatement must meet (test_stereo_reference.check_case).

PAINTED scenes: a flat background with one 11 x 11 patch per left keypoint and one 11 x 21 strip per right keypoint whose SAD
profile over the 11 shifts is known by construction; every left keypoint sits in a 12-row slot of its own, so that only the
right keypoints of its slot are in its row band.  MUTATED scenes: the extractor's keypoints of a shifted pair with single
fields moved onto the edges of the row band, the octave gate, the u window, endu and maxD."""
import numpy as np

import oracle_lib as ol
import stereo_reference as sr
from visual_sgraphs_amd import synth

F32 = np.float32
W, H, NLEVELS, SCALE, NFEAT = 320, 240, 4, 1.2, 500
EXTRACTOR = (NFEAT, SCALE, NLEVELS, 20, 7)
BACKGROUND = 128
SLOT = 12  # rows per painted case: the 11-row window, and the +-2-row band of an octave-0 right keypoint inside it
PARK_Y = 234.0  # right keypoints that only fill the array: their band (232..236) holds no left keypoint


def rectified_pair(w, h, seed, disparity):
    """Left frame + a right frame = the left shifted by `disparity` px along x with fresh noise (as test_gpu_stereo)."""
    left = synth.frame(w, h, seed)
    right = np.empty_like(left)
    right[:, :-disparity] = left[:, disparity:]
    right[:, -disparity:] = left[:, -1:]
    nz = synth.splitmix64(seed * 7 + 1, left.size).reshape(left.shape) % np.uint64(5)
    right = np.clip(right.astype(np.int32) + nz.astype(np.int32) - 2, 0, 255).astype(np.uint8)
    return left, right


def keypoints(x, y, octave):
    k = np.zeros(len(x), ol.KP_DTYPE)
    k["x"], k["y"], k["octave"] = np.asarray(x, F32), np.asarray(y, F32), octave
    k["size"], k["angle"], k["response"], k["class_id"] = 31.0, 0.0, 1.0, -1
    return k


def flipped(desc, nbits, rng):
    """`desc` with exactly nbits bits flipped: Hamming distance nbits."""
    out = desc.copy()
    for b in rng.choice(256, nbits, replace=False):
        out[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def oracle_pair(L, R):
    el, er = ol.OracleExtractor(*EXTRACTOR), ol.OracleExtractor(*EXTRACTOR)
    outl, outr = el(L), er(R)
    return el, er, outl, outr


class Painter:
    """Collects painted cases; one case = one slot of 12 rows."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.L = np.full((H, W), BACKGROUND, np.uint8)
        self.R = np.full((H, W), BACKGROUND, np.uint8)
        self.kl, self.dl, self.kr, self.dr, self.cases, self.roct = [], [], [], [], [], []
        self.slot = 0

    def row(self):
        y = 8 + SLOT * self.slot  # window rows y-5 .. y+5 inside 3 .. 229
        self.slot += 1
        assert y + 5 < PARK_Y - 2 - 1
        return y

    def texture(self, h, w):
        return self.rng.integers(30, 200, (h, w)).astype(np.uint8)

    def desc(self):
        return self.rng.integers(0, 256, 32).astype(np.uint8)

    def left(self, x, y, desc, patch, cx=None, cy=None, sad=0):
        """Left keypoint at (x, y) whose 11 x 11 window (centre cx, cy = roundf of x, y) is `patch`; `sad` is added to one
        pixel, which raises the SAD of every shift at which the strip repeats the patch by exactly `sad`."""
        cx, cy = int(sr.roundf(x)) if cx is None else cx, int(sr.roundf(y)) if cy is None else cy
        p = patch.copy()
        if sad:
            assert int(p[3, 5]) + sad <= 255  # the centre column: a symmetric patch stays symmetric in its SADs
            p[3, 5] += sad
        assert 5 <= cx < W - 5 and 5 <= cy < H - 5
        self.L[cy - 5:cy + 6, cx - 5:cx + 6] = p
        self.kl.append((x, y)), self.dl.append(desc)
        return len(self.kl) - 1

    def right(self, x, y, desc, strip=None, cx=None, cy=None, octave=0):
        """Right keypoint at (x, y); `strip` (11 x 21) is painted around column cx = roundf(x)."""
        if strip is not None:
            cx, cy = int(sr.roundf(x)) if cx is None else cx, int(sr.roundf(y)) if cy is None else cy
            assert 10 <= cx < W - 10 and 5 <= cy < H - 5
            self.R[cy - 5:cy + 6, cx - 10:cx + 11] = strip
        self.kr.append((x, y)), self.dr.append(desc), self.roct.append(octave)
        return len(self.kr) - 1

    def park(self, n):
        """n right keypoints nobody sees (array filler: lane and stride positions of the others)."""
        for _ in range(n):
            self.right(float(self.rng.integers(20, 300)), PARK_Y, self.desc())

    def strip_with(self, patch, shift):
        """A random strip that repeats `patch` at shift `shift` (columns shift + 5 .. shift + 15)."""
        s = self.texture(11, 21)
        s[:, shift + 5:shift + 16] = patch
        return s

    def plain(self, xl, xr, shift, ham, sad, check, arg=None, yl=None, yr=None, roct=0):
        """One left / one right keypoint, Hamming distance `ham`, the patch repeated at `shift` of the strip."""
        y = self.row()
        yl, yr = (y if yl is None else y + yl), (y if yr is None else y + yr)
        d, patch = self.desc(), self.texture(11, 11)
        patch[3, 5] = 100  # room for the SAD pixel
        cy = int(sr.roundf(yl))  # the rows of BOTH windows are the left keypoint's
        i = self.left(xl, yl, d, patch, cy=cy, sad=sad)
        j = self.right(xr, yr, flipped(d, ham, self.rng), self.strip_with(patch, shift), cy=cy, octave=roct)
        self.cases.append((i, check, arg if arg is not None else j))
        return i, j

    def scene(self, name, mb=1.0, mbf=64.0):
        kl = keypoints([p[0] for p in self.kl], [p[1] for p in self.kl], 0)
        kr = keypoints([p[0] for p in self.kr], [p[1] for p in self.kr], np.array(self.roct, np.int32))
        return dict(name=name, L=self.L, R=self.R, kl=kl, dl=np.array(self.dl, np.uint8).reshape(-1, 32), kr=kr,
                    dr=np.array(self.dr, np.uint8).reshape(-1, 32), mb=mb, mbf=mbf, cases=self.cases)


def periodic(p, zero_shifts_from):
    """Patch and strip of column period 5: the SAD is 0 at `zero_shifts_from` + 5 k."""
    v = p.texture(11, 5)
    v[:, 1:] = (v[:, :1].astype(np.int32) + np.array([37, 71, 113, 151])[None, :]) % 170 + 30  # five distinct columns
    patch = v[:, np.arange(11) % 5]
    strip = v[:, (np.arange(21) - 5 - zero_shifts_from) % 5]
    return patch, strip


def symmetric(p):
    """Patch and strip symmetric about their centre columns: SAD(-s) == SAD(s), SAD(0) == 0."""
    h = p.texture(11, 11)
    return h[:, np.abs(np.arange(11) - 5)], h[:, np.abs(np.arange(21) - 10)]


def painted_main():
    """maxD = 64.  Most patches carry SAD 40: the median, so that the cut (thDist = 84) takes nobody here."""
    p = Painter(2024)
    S = 40
    # ---- descriptor thresholds: dist < 100 enters, bestDist < 75 matches
    p.plain(150.0, 140.0, 0, 74, S, "matched")
    p.plain(150.0, 140.0, 0, 75, S, "reason", sr.BEST_HAMMING)
    p.plain(150.0, 140.0, 0, 99, S, "reason", sr.BEST_HAMMING)
    p.plain(150.0, 140.0, 0, 100, S, "reason", sr.HAMMING_HIGH)
    # ---- descriptor ties, the duplicates 3 px apart; the patch is in reach (|shift| <= 4) of the FIRST of them only
    for order, gap in (("left_first", 1), ("right_first", 1), ("left_first", 64), ("right_first", 64)):
        y, d, patch = p.row(), p.desc(), p.texture(11, 11)
        i = p.left(200.0, y, d, patch, sad=S)
        dup = flipped(d, 10, p.rng)
        xa, xb = (150.0, 153.0) if order == "left_first" else (153.0, 150.0)
        centre = 147 if order == "left_first" else 156  # shift -3 of 150 / +3 of 153, out of reach of the other
        strip = p.texture(11, 27)  # columns 140 .. 166: both keypoints' strips
        strip[:, centre - 5 - 140:centre + 6 - 140] = patch
        p.R[y - 5:y + 6, 140:167] = strip
        a = p.right(xa, y, dup)
        p.park(gap - 1)  # gap 64: the two sit in ONE lane of the scan (iR and iR + 64)
        p.right(xb, y, dup.copy())
        p.cases.append((i, "tie", a))
    # ---- SAD ties over the shifts: the first minimum wins
    y, d = p.row(), p.desc()
    patch, strip = periodic(p, 1)  # zeros at -4 and +1
    i = p.left(180.0, y, d, patch, sad=S)
    p.right(150.0, y, flipped(d, 5, p.rng), strip)
    p.cases.append((i, "sad_tie", (-4, [-4, 1])))
    y, d = p.row(), p.desc()
    patch, strip = periodic(p, 0)  # zeros at -5, 0, +5: the first minimum is at -L
    i = p.left(180.0, y, d, patch, sad=S)
    p.right(150.0, y, flipped(d, 5, p.rng), strip)
    p.cases.append((i, "sad_tie", (-5, [-5, 0, 5])))
    # ---- best shift at +-L alone, and the shifts next to them
    p.plain(180.0, 150.0, 5, 5, S, "reason", sr.SHIFT_EDGE)
    p.plain(180.0, 150.0, -5, 5, S, "reason", sr.SHIFT_EDGE)
    p.plain(180.0, 150.0, 4, 5, S, "shift", 4)
    p.plain(180.0, 150.0, -4, 5, S, "shift", -4)
    p.park(140 - len(p.kr))  # the launch-shape cases slice this scene to 129 right keypoints
    return p.scene("painted_main")


def painted_clamp():
    """dist1 == dist3 and disparity exactly 0 at several magnitudes of uL; disparity < 0; roundf on k + 0.5."""
    p = Painter(2025)
    S = 40
    for x in (12.0, 31.0, 100.0, 255.0, 256.0, 301.0):
        y, d = p.row(), p.desc()
        patch, strip = symmetric(p)
        i = p.left(x, y, d, patch, sad=S)
        p.right(x, y, flipped(d, 5, p.rng), strip)
        p.cases.append((i, "clamp", None))
    # ---- disparity < 0 (the patch lies right of uL) -> out of range
    p.plain(150.0, 150.0, 3, 5, S, "reason", sr.DISPARITY_RANGE)
    # ---- the only keypoint of the band is two octaves up
    p.plain(150.0, 140.0, 0, 5, S, "reason", sr.OCTAVE_GATE, roct=2)
    p.plain(150.0, 140.0, 0, 5, S, "matched", roct=1)
    # ---- roundf: x * invScale = k + 0.5 with k even (round-half-even would go down), both eyes and y
    p.plain(160.5, 130.5, 0, 5, S, "matched", yl=0.5, yr=0.5)
    p.plain(162.5, 140.0, 0, 5, S, "matched")
    p.plain(170.0, 132.5, 0, 5, S, "matched")
    return p.scene("painted_clamp")


def painted_median(name, sads, cut):
    """One plain case per entry of `sads` (None: a left keypoint that matches nothing); `cut`: the SADs the median takes."""
    p = Painter(77 + len(sads) + sum(s or 0 for s in sads))
    for s in sads:
        if s is None:
            p.plain(150.0, 140.0, 0, 100, 0, "reason", sr.HAMMING_HIGH)
        else:
            p.plain(150.0, 140.0, 0, 5, s, "sad_cut" if s in cut else "sad_kept", s)
    p.park(3)
    return p.scene(name)


def exact_threshold_median():
    """The smallest median m >= 10 at which 1.5f * 1.4f * m is an integer in float: a SAD can sit exactly on thDist."""
    for m in range(10, 120):
        th = F32(F32(F32(1.5) * F32(1.4)) * F32(m))
        if float(th) == int(th):
            return m, int(th)
    raise AssertionError("no integral threshold")


def painted_nr65():
    """One left keypoint, 65 right keypoints in its band and window: the only one below 75 is index 64."""
    p = Painter(65)
    y, d, patch = p.row(), p.desc(), p.texture(11, 11)
    i = p.left(200.0, y, d, patch, sad=20)
    for k in range(64):
        p.right(100.0 + k, y, flipped(d, 80 + k % 19, p.rng))
    j = p.right(180.0, y, flipped(d, 30, p.rng), p.strip_with(patch, 0))
    p.cases.append((i, "matched", j))
    return p.scene("painted_nr65", mbf=128.0)


def painted_scenes():
    m, th = exact_threshold_median()
    return [painted_main(), painted_clamp(),
            painted_median("median_odd", [10, 20, 30, 50, 63], {63}),        # median 30, thDist 63 (exactly: 62.999996)
            painted_median("median_even", [10, 20, 30, 62, 63, 64], set()),  # median = element 3 = 62: nobody is cut
            painted_median("median_one", [25, None], set()),                 # 25 < 52.5: kept
            painted_median("median_equal", [33, 33, 33, 33], set()),
            painted_median("median_zero", [0, 0, 0, 7, 9], {0, 7, 9}),       # thDist 0: `0 < 0` is false, everything is cut
            painted_median("median_exact", [1, m, m, th - 1, th], {th}),     # a SAD exactly on thDist is cut, thDist - 1 is not
            painted_nr65()]


# ---------------------------------------------------------------------------------------------------- mutated scenes

def base_pair(seed=9, disparity=11, mb=1.0, mbf=40.0):
    L, R = rectified_pair(W, H, seed, disparity)
    el, er, (_, kl, dl), (_, kr, dr) = oracle_pair(L, R)
    t = el.tables()
    got = sr.compute(sr.pyramids(el), sr.pyramids(er), t["scale"], t["inv_scale"], kl, dl, kr, dr, mb, mbf)
    return dict(L=L, R=R, kl=kl, dl=dl, kr=kr, dr=dr, mb=mb, mbf=mbf, scale=t["scale"], inv_scale=t["inv_scale"],
                level_cols=[el.level_size(l)[0] for l in range(NLEVELS)]), got


def take_pairs(base, got, used, level, n, right_octave=None):
    """n matched (iL, jR) of left level `level` whose right keypoint nobody has taken yet."""
    out = []
    for i in np.flatnonzero((got["reason"] == sr.MATCHED) & (base["kl"]["octave"] == level)):
        j = int(got["best_idx"][i])
        if j in used or (right_octave is not None and base["kr"]["octave"][j] != right_octave):
            continue
        used.add(j), out.append((int(i), j))
        if len(out) == n:
            return out
    raise AssertionError(f"the base pair has fewer than {n} free matches at level {level}")


def band_y(row, r, which):
    """A right y for which `row` is the first / last row of the band, or the nearest row outside it."""
    r = F32(r)
    if which in ("first", "below"):  # minr = floor(y - r) == row (first) or row + 1 (the band starts one row below)
        want = row if which == "first" else row + 1
        y = F32(F32(want) + r)
        while int(np.floor(F32(y - r))) < want:
            y = np.nextafter(y, F32(np.inf))
        assert int(np.floor(F32(y - r))) == want
    else:  # maxr = ceil(y + r) == row (last) or row - 1
        want = row if which == "last" else row - 1
        y = F32(F32(want) - r)
        while int(np.ceil(F32(y + r))) > want:
            y = np.nextafter(y, F32(-np.inf))
        assert int(np.ceil(F32(y + r))) == want
    return y


def mutated_scenes():
    base, got = base_pair()
    scale = base["scale"]
    used = set()
    kr, kl = base["kr"].copy(), base["kl"].copy()
    cases = []
    # ---- the row band of every octave: first row, last row, one row outside each way (fractional y above level 0)
    for o in range(NLEVELS):
        for (i, j), which in zip(take_pairs(base, got, used, o, 4, right_octave=o), ("first", "last", "below", "above")):
            kr["y"][j] = band_y(int(kl["y"][i]), F32(2.0) * scale[o], which)
            cases.append((i, "winner" if which in ("first", "last") else "not_winner", j))
    # ---- the octave gate at level 0, at the top level and between
    for level, inside, outside in ((0, (1,), (2,)), (3, (2,), (1,)), (1, (0, 2), (3,)), (2, (1, 3), (0,))):
        pairs = take_pairs(base, got, used, level, len(inside) + len(outside))
        for (i, j), o in zip(pairs, inside + outside):
            kr["octave"][j] = o
            cases.append((i, "winner" if o in inside else "not_winner", j))
    # ---- the u window: uR == minU, uR == maxU, one ulp outside each
    max_d = got["max_d"]
    for (i, j), which in zip(take_pairs(base, got, used, 0, 2) + take_pairs(base, got, used, 1, 2),
                             ("min", "below_min", "max", "above_max")):
        ul = F32(kl["x"][i])
        x = F32(ul - max_d) if which in ("min", "below_min") else ul
        if which == "below_min":
            x = np.nextafter(x, F32(-np.inf))
        if which == "above_max":
            x = np.nextafter(x, F32(np.inf))
        kr["x"][j] = x
        cases.append((i, "winner" if which in ("min", "max") else "not_winner", j))
    # ---- endu == cols (skipped) and endu == cols - 1 (searched) on levels above 0; the left keypoint moves along so that
    # uR <= uL holds, every window stays inside the level
    for level in (1, 3):
        cols = base["level_cols"][level]
        for (i, j), endu in zip(take_pairs(base, got, used, level, 2), (cols, cols - 1)):
            x = F32(F32(endu - 11) * scale[level])
            assert sr.roundf(F32(x * base["inv_scale"][level])) == endu - 11
            kr["x"][j], kl["x"][i] = x, np.nextafter(x, F32(np.inf))
            cases.append((i, "reason" if endu == cols else "searched", sr.ENDU))
    edges = dict(base, name="mutated_edges", kl=kl, kr=kr, cases=cases)
    # ---- disparity < maxD at its edge: maxD = mbf / 1 is the true disparity of one match, and the next float above it
    ok = np.flatnonzero((got["reason"] == sr.MATCHED))
    disp = (base["kl"]["x"][ok] - got["u_right"][ok]).astype(F32)
    room = base["kr"]["x"][got["best_idx"][ok]] >= (base["kl"]["x"][ok] - disp).astype(F32)  # uR0 stays inside [minU, maxU]
    k = ok[room][np.argmax(disp[room])]
    d = F32(base["kl"]["x"][k] - got["u_right"][k])
    at = dict(base, name="maxd_at", mb=1.0, mbf=float(d), cases=[(int(k), "reason", sr.DISPARITY_RANGE)])
    above = dict(base, name="maxd_above", mb=1.0, mbf=float(np.nextafter(d, F32(np.inf))), cases=[(int(k), "kept", None)])
    return [dict(base, name="mutated_base", cases=[]), edges, at, above]


def guard_scene():
    """Hand-made keypoints on levels 1 and 2 of a shifted pair whose SAD windows leave the level by COLUMNS only: the device
    gives them no match; the reference reads its border.  (left index, what leaves) in `cases`."""
    L, R = rectified_pair(W, H, 21, 9)
    rng = np.random.default_rng(5)
    el = ol.OracleExtractor(*EXTRACTOR)
    el(L)
    t = el.tables()
    xs_l, xs_r, ys, octs, cases = [], [], [], [], []
    for level in (1, 2):
        cols, sc = el.level_size(level)[0], t["scale"][level]
        for k, (sl, srr, what) in enumerate(((3, 3, "left and right"), (14, 6, "right strip"), (cols - 3, cols - 14, "left window"),
                                            (30, 20, None), (cols - 6, cols - 16, None), (cols - 5, cols - 16, "left window"),
                                            (20, 9, "right strip"), (20, 10, None))):
            xs_l.append(F32(sl * sc)), xs_r.append(F32(srr * sc)), ys.append(F32(20 + 9 * k + 100 * (level - 1))), octs.append(level)
            cases.append((len(xs_l) - 1, "window" if what else "searched", sr.WINDOW))
    kl, kr = keypoints(xs_l, ys, np.array(octs)), keypoints(xs_r, ys, np.array(octs))
    dl = rng.integers(0, 256, (len(kl), 32)).astype(np.uint8)
    dr = np.array([flipped(d, 7, rng) for d in dl])
    return dict(name="guard", L=L, R=R, kl=kl, dl=dl, kr=kr, dr=dr, mb=1.0, mbf=300.0, cases=cases)


_cache = {}


def all_scenes():
    """Every parity scene (all windows inside the image), built once."""
    if "all" not in _cache:
        _cache["all"] = painted_scenes() + mutated_scenes()
    return _cache["all"]


def expected(scene, window_guard=False):
    """The restatement's result on a scene (cached) and the two oracle extractors that carry its pyramids."""
    key = (scene["name"], window_guard)
    if key not in _cache:
        el, er, _, _ = oracle_pair(scene["L"], scene["R"])
        t = el.tables()
        res = sr.compute(sr.pyramids(el), sr.pyramids(er), t["scale"], t["inv_scale"], scene["kl"], scene["dl"], scene["kr"],
                         scene["dr"], scene["mb"], scene["mbf"], window_guard)
        _cache[key] = (res, el, er)
    return _cache[key]
