"""Seeded keyframes, map points and observation lists for the tests of vsg_mappoints_refresh_from_observations
(tests/test_gpu_mappoints_refresh.py, tests/test_abi_observations.py).  Nothing here needs a device.

Five keyframes of n = 1, 7, 64, 300 and 300 features, octaves 0 .. 7 (tests/obs_cases.py: the refusals run on the same
frames).  A point's observations of three or more keyframes own their features: their descriptors are a base row with each
bit flipped with a per-row probability drawn from [0.02, 0.25], so that the distinctive descriptor is usually not row 0 and
least medians tie now and then.  Points of fewer observations pick any feature (with one or two rows every median is 0)."""
import numpy as np

import obs_cases as oc
import observations_reference as obr
from visual_sgraphs_amd import orb

F32 = np.float32
SF = (F32(1.2) ** np.arange(8, dtype=F32)).astype(F32)
KP_DTYPE = orb.KP_DTYPE
BOUNDS = (0.0, 0.0, 640.0, 480.0)


def keyframes(seed=1):
    """[(kps, desc)] of the five keyframes: random positions and descriptors, obs_cases' octaves."""
    rng = np.random.default_rng(seed)
    out = []
    for n, o in zip(oc.KF_N, oc.octaves()):
        k = np.zeros(n, KP_DTYPE)
        k["x"], k["y"] = rng.uniform(0, 640, n), rng.uniform(0, 480, n)
        k["size"], k["octave"] = 31.0, o
        out.append((k, rng.integers(0, 256, (n, 32), dtype=np.uint8)))
    return out


def noisy_rows(rng, m):
    """m descriptors of one point: a base row, each bit of row j flipped with probability p_j from [0.02, 0.25]."""
    base = rng.integers(0, 2, 256, dtype=np.uint8)
    flip = rng.random((m, 256)) < rng.uniform(0.02, 0.25, (m, 1))
    return np.packbits(base[None, :] ^ flip.astype(np.uint8), axis=1)


class Owner:
    """Hands out features of the keyframes that no other point's list holds."""

    def __init__(self, frames, table, rng):
        self.rng, self.table = rng, np.asarray(table)
        self.free = {f: list(rng.permutation(len(frames[f][0]))) for f in set(table)}

    def take(self, entry):
        pool = self.free[int(self.table[entry])]
        return int(pool.pop()) if pool else None


def store_fields(rng, capacity, centres):
    """A whole store of random fields; the positions keep 0.5 away from every camera centre (no 0 / 0 here)."""
    P = rng.uniform(-5, 5, (capacity, 3)).astype(F32)
    while True:
        close = (np.linalg.norm(P[:, None, :] - centres[None, :, :], axis=2) < 0.5).any(axis=1)
        if not close.any():
            break
        P[close] = rng.uniform(-5, 5, (int(close.sum()), 3)).astype(F32)
    nrm = rng.normal(0, 1, (capacity, 3)).astype(F32)
    return dict(world_pos=P, normal=nrm, min_dist=rng.uniform(0.1, 1, capacity).astype(F32),
                max_dist=rng.uniform(2, 9, capacity).astype(F32), desc=rng.integers(0, 256, (capacity, 32), dtype=np.uint8),
                observed=(rng.random(capacity) < 0.8).astype(np.uint8))


def problem(frames, table, lists, bad, ref_pos, slots, Ow):
    """The arguments of one call from per-point lists of (table entry, idx)."""
    off = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int32)
    flat = [o for l in lists for o in l]
    return dict(slots=np.asarray(slots, np.int32), off=off, kf=np.array([o[0] for o in flat], np.int32),
                idx=np.array([o[1] for o in flat], np.int32),
                bad=None if bad is None else np.concatenate([np.asarray(b, np.uint8) for b in bad] + [np.zeros(0, np.uint8)]),
                ref_pos=np.asarray(ref_pos, np.int32), frames=[frames[f] for f in table], table=list(table),
                Ow=np.asarray(Ow, F32), scale_factors=SF)


def main_scene(seed=2, n_points=400, capacity=1000):
    """About 400 points in a store of 1000, slots a random subset; nine keyframe-table entries over the five frames (a
    keyframe of 300 features stands for several keyframes: the entries differ in their camera centre), lists of 0 to 9
    observations (the longest: the list of the ends) with about 8 % of them bad.  Returns (frames, store fields, problem);
    the frames' descriptors are edited in place for the points that own their rows."""
    rng = np.random.default_rng(seed)
    frames = keyframes(seed)
    table = [0, 1, 2, 3, 4, 3, 4, 3, 4]
    Ow = rng.normal(0, 2.5, (len(table), 3)).astype(F32)
    store = store_fields(rng, capacity, Ow)
    slots = rng.choice(capacity, n_points, replace=False).astype(np.int32)
    own = Owner(frames, table, rng)
    lists = []
    for i in range(n_points):
        rich = i % 4 == 0
        m = int(rng.integers(3, 8)) if rich else int(rng.integers(0, 3))
        entries = np.sort(rng.choice(np.arange(2, len(table)) if rich else len(table), m, replace=False))
        obs = []
        for e in entries:
            j = own.take(e) if rich else int(rng.integers(0, len(frames[table[e]][0])))
            if j is not None:
                obs.append((int(e), j))
        if rich and len(obs) >= 3:
            rows = noisy_rows(rng, len(obs))
            for (e, j), r in zip(obs, rows):
                frames[table[e]][1][j] = r
        lists.append(obs)
    # the ends: idx = n - 1 of every keyframe, the n = 1 keyframe and kf = n_kf - 1 in one list (features are shared)
    lists[1] = [(e, len(frames[table[e]][0]) - 1) for e in range(len(table))]
    bad = [(rng.random(len(l)) < 0.08).astype(np.uint8) for l in lists]
    ref_pos = [int(rng.integers(0, len(l))) if l else int(rng.integers(-5, 50)) for l in lists]
    return frames, store, problem(frames, table, lists, bad, ref_pos, slots, Ow)


def edge_scene(seed=3, capacity=1000, counts=(1, 2, 3, 63, 64, 65, 128), padded=True):
    """Points whose counts of good observations sit at the kernel's edges.  More observations than keyframes: a keyframe
    table of 140 entries in which the entries name the two 300-feature frames in turn (the choice the issue leaves: several
    entries name the same frame, every entry with a camera centre of its own).  padded: every other point also has bad
    observations in between, so that a list is longer than its candidates (64 good of 71: more than one 64-chunk)."""
    rng = np.random.default_rng(seed)
    frames = keyframes(seed)
    table = [3 + (e & 1) for e in range(140)]
    Ow = rng.normal(0, 2.5, (len(table), 3)).astype(F32)
    store = store_fields(rng, capacity, Ow)
    own = Owner(frames, table, rng)
    lists, bad = [], []
    for k, c in enumerate(counts):
        extra = 7 if (padded and k % 2 == 0) else 0
        flags = np.zeros(c + extra, np.uint8)
        flags[rng.choice(c + extra, extra, replace=False)] = 1
        obs = [(e, own.take(e)) for e in range(c + extra)]
        rows = noisy_rows(rng, c)
        for (e, j), r in zip([o for o, f in zip(obs, flags) if not f], rows):
            frames[table[e]][1][j] = r
        lists.append(obs), bad.append(flags)
    slots = rng.choice(capacity, len(counts), replace=False).astype(np.int32)
    ref_pos = [int(rng.integers(0, len(l))) for l in lists]
    return frames, store, problem(frames, table, lists, bad, ref_pos, slots, Ow)


def fixture_conditions(prob):
    """(share of points with >= 3 good observations whose best != 0 among the good rows, share with a tie of the least
    median, number of such points) -- from the restatement alone."""
    off, n = prob["off"], len(prob["slots"])
    moved = ties = count = 0
    for i in range(n):
        o, e = off[i], off[i + 1]
        good = np.arange(o, e) if prob["bad"] is None else o + np.flatnonzero(prob["bad"][o:e] == 0)
        if len(good) < 3:
            continue
        rows = np.stack([prob["frames"][prob["kf"][g]][1][prob["idx"][g]] for g in good])
        med = obr.medians(rows)
        count += 1
        moved += int(np.argmin(med) != 0)
        ties += int((med == med.min()).sum() > 1)
    return moved / max(count, 1), ties / max(count, 1), count
