"""Scenes for the batched device matcher (vsg_hamming_block_best2_device -> k_block_best2_mfma), as plain data, and a plain
restatement of what it computes.  No GPU is needed here: tests/test_match_scenes.py proves the scenes on the CPU,
tests/test_gpu_match_batched.py runs them on the device.

Two kinds of data:
  * BLOCKS BY CONSTRUCTION (placed_block): one query x and nb train rows that are x with a CHOSEN number of bits flipped,
    so (best, second, arg) is known before any code runs.  The case lists put the best and the second best on chosen rows
    of the kernel's C/D layout: a lane of the 32 x 32 tile holds, for column c and half h, the rows
    (g & 3) + 8 * (g >> 2) + 4 * h of registers g = 0..15; a workgroup walks 32-row tiles in prefetch groups of 8 tiles;
    full tiles fold on float keys, the partial tail tile on integer keys.
  * COUNT SCENES: tie-heavy random rows (a few base descriptors, one or two bits flipped) under the row counts at which
    the launch geometry changes, side by side in one launch.

A case is a dict: name, seam (what it is aimed at), a [rows, 32], na, b [rows, 32], nb, expect {A row: (best, second,
arg)} for the rows whose answer is known by construction."""
import functools
import itertools

import numpy as np

SENTINEL = 0x5A5A5A5A
TILE, GROUP_TILES, WG_ROWS = 32, 8, 256  # train rows per tile, tiles per prefetch group, A rows per workgroup


# ---- the restatement
def unpack(rows):
    return np.unpackbits(np.ascontiguousarray(rows, dtype=np.uint8).reshape(-1, 32), axis=1)


def best2_reference(a, na, b, nb):
    """Rows [:na] of a against rows [:nb] of b: best = least Hamming distance, arg = first index that attains it, second =
    second smallest with duplicates counted (a tie gives second == best).  The scan is a strict '<' from 256: distance 256
    is never selected, so all-256 or nb <= 0 gives (256, 256, -1).  Integer-exact; returns three int32 arrays [max(na, 0)]."""
    na, nb = max(int(na), 0), max(int(nb), 0)
    best, second, arg = np.full(na, 256, np.int32), np.full(na, 256, np.int32), np.full(na, -1, np.int32)
    if na == 0 or nb == 0:
        return best, second, arg
    # bits that differ, [na, nb]: counts of at most 256 ones, exact in float32 (which lets the product run in BLAS)
    ab, bb = unpack(a[:na]).astype(np.float32), unpack(b[:nb]).astype(np.float32)
    dist = (ab @ (1 - bb).T + (1 - ab) @ bb.T).astype(np.int32)
    arg0 = dist.argmin(axis=1)  # first index of the minimum
    best[:] = dist[np.arange(na), arg0]
    if nb >= 2:
        second[:] = np.partition(dist, 1, axis=1)[:, 1]
    arg[:] = np.where(best < 256, arg0, -1)
    return best, second, arg


def scan_distances(dists):
    """(best, second, arg) of the reference's scan over a list of CHOSEN distances: what a block built by placed_block must
    give, worked out from the numbers that went into it and from nothing else."""
    best, second, arg = 256, 256, -1
    for j, d in enumerate(dists):
        if d < best:
            best, second, arg = d, best, j
        elif d < second:
            second = d
    return best, second, arg


# ---- rows by construction
def masks_of_popcount(rng, pops):
    """[len(pops), 32] uint8 masks, row i with exactly pops[i] bits set at random places."""
    pops = np.asarray(pops, dtype=np.int64)
    order = np.argsort(rng.random((len(pops), 256)), axis=1)
    bits = np.zeros((len(pops), 256), np.uint8)
    np.put_along_axis(bits, order, (np.arange(256)[None, :] < pops[:, None]).astype(np.uint8), axis=1)
    return np.packbits(bits, axis=1)


def placed_block(rng, nb, placed, background=(100, 156)):
    """One query x and nb train rows: row r of `placed` = {row: dist} is x with exactly dist bits flipped, every other row
    is x xor a mask whose popcount is drawn from background[0]..background[1] (inclusive).  Returns x [32], b [nb, 32] and
    the expected (best, second, arg), known from the chosen distances alone."""
    x = rng.integers(0, 256, 32, dtype=np.uint8)
    pops = rng.integers(background[0], background[1] + 1, nb)
    for r, d in placed.items():
        assert 0 <= r < nb and 0 <= d <= 256
        pops[r] = d
    b = masks_of_popcount(rng, pops) ^ x[None, :]
    return x, b, scan_distances(pops.tolist())


def near_duplicates(rng, base, n, flips):
    """n rows drawn from the few `base` descriptors with up to `flips` bits flipped (0..flips, so exact duplicates stay
    frequent): many exact ties and many second == best."""
    rows = base[rng.integers(0, len(base), n)]
    return rows ^ masks_of_popcount(rng, rng.integers(0, flips + 1, n))


# ---- where a train row sits in the kernel's layout
def layout(row):
    """(prefetch group, tile, half h, register g) of a train row."""
    o = row % TILE
    return row // (TILE * GROUP_TILES), row // TILE, (o >> 2) & 1, (o & 3) + 4 * (o >> 3)


def seams(p, q, nb):
    """What a pair of train rows p < q of an nb-row block lies across, as a sorted list of names."""
    (gp, tp, hp, _), (gq, tq, hq, _) = layout(p), layout(q)
    tail = nb // TILE if nb % TILE else -1  # the partial tile (integer-key path), if any
    out = []
    if tp == tq:
        out.append("same_lane" if hp == hq else "other_half")
    elif tq == tp + 1:
        out.append("adjacent_tiles")
    else:
        out.append("distant_tiles")
    if gq == gp + 1:
        out.append("adjacent_groups")
    elif gq > gp + 1:
        out.append("distant_groups")
    if (tp == tail) != (tq == tail):
        out.append("full_vs_tail")
    elif tp == tail:
        out.append("both_in_tail")
    return sorted(out)


# ---- the case lists
P = [0, 1, 3, 4, 8, 27, 28, 31, 32, 36, 255, 256, 259, 287, 288, 291, 299]
SEAM_NB = 300  # rows 288..299: the partial tail tile; row 256 opens the second prefetch group
D_CYCLE = [0, 1, 17, 49, 50, 99]
TRIPLES = [(0, 1, 4), (3, 4, 32), (31, 32, 288), (255, 256, 299), (27, 259, 291), (288, 291, 299)]
PLACEMENT_PAIRS = [(0, 4), (255, 256), (287, 288)]
PLACEMENT_ROWS = [0, 31, 32, 63, 64, 127, 128, 255, 256, 319]
PLACEMENT_MAX_ROWS = 320
WIDE_NB = 544  # 17 full tiles: groups [0, 256), [256, 512), [512, 544)
WIDE_PAIRS = [(255, 512), (511, 512)]


def _case(rng, name, nb, placed, stated, query_row=0, background=(100, 156)):
    """A block with the directed query at A row `query_row` (random rows before it, na = query_row + 1).  `stated` is the
    expectation as the case list states it; tests/test_match_scenes.py holds it against placed_block's and the restatement."""
    x, b, expect = placed_block(rng, nb, placed, background)
    a = rng.integers(0, 256, (query_row + 1, 32), dtype=np.uint8)
    a[query_row] = x
    rows = sorted(placed)
    return dict(name=name, seam=seams(rows[0], rows[1], nb) if len(rows) >= 2 else [], placed=dict(placed), a=a,
                na=query_row + 1, b=b, nb=nb, expect={query_row: expect}, stated=stated)


def _three_orders(rng, p, q, d, nb, tag="", query_row=0):
    t = f"{tag}p={p} q={q} d={d}"
    return [_case(rng, f"tie {t}", nb, {p: d, q: d}, (d, d, p), query_row),
            _case(rng, f"second before best {t}", nb, {p: d + 1, q: d}, (d, d + 1, q), query_row),
            _case(rng, f"second after best {t}", nb, {p: d, q: d + 1}, (d, d + 1, p), query_row)]


@functools.lru_cache(maxsize=None)
def tie_cases():
    """Every pair p < q of P as tie / second before best / second after best, d cycling through D_CYCLE, plus triples."""
    rng = np.random.default_rng(20)
    out = []
    for k, (p, q) in enumerate(itertools.combinations(P, 2)):
        out += _three_orders(rng, p, q, D_CYCLE[k % len(D_CYCLE)], SEAM_NB)
    for k, (p, q, r) in enumerate(TRIPLES):
        d = D_CYCLE[k % len(D_CYCLE)]
        out.append(_case(rng, f"triple p={p} q={q} r={r} d={d}", SEAM_NB, {p: d, q: d, r: d}, (d, d, p)))
    return out


@functools.lru_cache(maxsize=None)
def extreme_cases():
    """The accumulator's end values: 2 * dist - 256 = +256 (complement), +254, and -256 (equal)."""
    rng = np.random.default_rng(21)
    out = [_case(rng, "every row the complement", SEAM_NB, {}, (256, 256, -1), background=(256, 256))]
    for r in (0, 31, 36, 255, 256, 288, 299):
        out.append(_case(rng, f"one row at 255 among complements, row {r}", SEAM_NB, {r: 255}, (255, 256, r),
                         background=(256, 256)))
    out.append(_case(rng, "every row equals the query", SEAM_NB, {}, (0, 0, 0), background=(0, 0)))
    return out


@functools.lru_cache(maxsize=None)
def placement_cases():
    """The tie blocks of three position pairs with the query at chosen A rows: every wave (64 rows each), both query sets u
    of a wave (32 rows each) and the second x-workgroup (rows 256..) own one directed column."""
    rng = np.random.default_rng(22)
    out = []
    for k, ((p, q), row) in enumerate(itertools.product(PLACEMENT_PAIRS, PLACEMENT_ROWS)):
        d = D_CYCLE[k % len(D_CYCLE)]
        out.append(_case(rng, f"tie p={p} q={q} d={d}, query at A row {row}", SEAM_NB, {p: d, q: d}, (d, d, p), row))
    return out


@functools.lru_cache(maxsize=None)
def wide_cases():
    """nb = 544: pairs across the SECOND prefetch-group edge (row 512), in the three orders each; a launch of its own with
    max_rows = 544."""
    rng = np.random.default_rng(23)
    out = []
    for k, (p, q) in enumerate(WIDE_PAIRS):
        out += _three_orders(rng, p, q, D_CYCLE[(3 * k + 1) % len(D_CYCLE)], WIDE_NB, tag="nb=544 ")
    return out


CASE_LISTS = {"ties": (tie_cases, SEAM_NB), "extremes": (extreme_cases, SEAM_NB),
              "placement": (placement_cases, PLACEMENT_MAX_ROWS), "wide": (wide_cases, WIDE_NB)}  # name: (list, max_rows)


def pack_cases(cases, max_rows):
    """The blocks of one launch: a, b [nblocks, max_rows, 32] (rows past a case's own are zero) and int32 na, nb."""
    n = len(cases)
    a, b = np.zeros((n, max_rows, 32), np.uint8), np.zeros((n, max_rows, 32), np.uint8)
    for i, c in enumerate(cases):
        a[i, :c["na"]], b[i, :c["nb"]] = c["a"], c["b"]
    return a, b, np.array([c["na"] for c in cases], np.int32), np.array([c["nb"] for c in cases], np.int32)


# ---- the count scenes
COUNT_MAX_ROWS = 320
INT_MAX = 2 ** 31 - 1
COUNT_PAIRS = ([(0, 300), (300, 0), (0, 0), (1, 1), (1, 320), (320, 1), (320, 320)]
               + [(na, 289) for na in (31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257)]
               + [(65, nb) for nb in (31, 32, 33, 255, 256, 257, 287, 288, 289)]
               + [(321, 289), (400, 289), (INT_MAX, 289), (65, 321), (65, 400), (65, INT_MAX), (INT_MAX, INT_MAX)]
               + [(-1, 289), (65, -1), (-1, -1)])


def clamp(n, max_rows):
    return min(max(int(n), 0), max_rows)


@functools.lru_cache(maxsize=None)
def count_scene():
    """a, b [nblocks, COUNT_MAX_ROWS, 32] with EVERY row tie-heavy data (so a count read wrongly, too large or from the
    neighbouring block changes the answer) and the int32 counts na, nb of COUNT_PAIRS."""
    rng = np.random.default_rng(24)
    n = len(COUNT_PAIRS)
    base = rng.integers(0, 256, (9, 32), dtype=np.uint8)
    a = near_duplicates(rng, base, n * COUNT_MAX_ROWS, 2).reshape(n, COUNT_MAX_ROWS, 32)
    b = near_duplicates(rng, base, n * COUNT_MAX_ROWS, 1).reshape(n, COUNT_MAX_ROWS, 32)
    for v in (a, b):
        v.setflags(write=False)
    return a, b, np.array([p[0] for p in COUNT_PAIRS], np.int32), np.array([p[1] for p in COUNT_PAIRS], np.int32)


def with_stale_rows(a, b, na, nb, max_rows):
    """Copies of a, b in which every A row >= na[i] and every B row >= nb[i] (clamped) is an exact copy of one of that
    block's queries, the first stale row a copy of query 0 and so on: a stale B row that took part would win at distance 0."""
    a, b = a.copy(), b.copy()
    rows = a.shape[1]
    for i in range(len(a)):
        n, m = clamp(na[i], max_rows), clamp(nb[i], max_rows)
        q = a[i, :n].copy() if n else a[i, :1].copy()
        a[i, n:] = q[np.arange(rows - n) % len(q)]
        b[i, m:] = q[np.arange(rows - m) % len(q)]
    return a, b
