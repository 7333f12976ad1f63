"""Candidate lists for the ordered walks (csrc/vsg_walks.h, csrc/vsg_walks_dev.h) in the layout k_window_search writes:
every query owns an inline slot of 16 entries, a longer list lies whole in the overflow area behind the slots, segments in
no particular order.  Shared by tests/test_walk_rounds.py, tests/test_sanitizers_walk.py and tests/test_gpu_track_walk.py
(the same case dictionaries feed k_track_walk on the device); run() walks one case through the host build
tests/_walkcore, by the serial definition and by the round form."""
import ctypes as C
import functools
import subprocess
from pathlib import Path

import numpy as np

F32, I32, U32, U8 = np.float32, np.int32, np.uint32, np.uint8
DIR = Path(__file__).resolve().parent / "_walkcore"
INLINE = 16
LAST, LOCAL = 0, 1


@functools.lru_cache(maxsize=None)
def lib():
    subprocess.check_call(["make", "-C", str(DIR)], stdout=subprocess.DEVNULL)
    L = C.CDLL(str(DIR / "libvsg_walkcore.so"))
    L.walkcore_case.restype = None
    L.walkcore_case.argtypes = [C.c_int] * 4 + [C.c_void_p] * 10 + [C.c_int, C.c_float] + [C.c_void_p] * 8
    L.walkcore_overflow.restype = None
    L.walkcore_overflow.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    return L


def entry(idx, dist, octave=0):
    return (np.asarray(idx, np.int64) | (np.asarray(dist, np.int64) << 15) | (np.asarray(octave, np.int64) << 24)).astype(U32)


def layout(lists, rng=None):
    """lists: one uint32 array per query -> ent, off, cnt as the device lays them out."""
    nq = len(lists)
    cnt = np.array([len(l) for l in lists], I32).reshape(nq)
    off = (np.arange(nq) * INLINE).astype(I32)
    long_ones = [q for q in range(nq) if cnt[q] > INLINE]
    if rng is not None:
        rng.shuffle(long_ones)
    at = nq * INLINE
    for q in long_ones:
        off[q] = at
        at += int(cnt[q])
    ent = np.full(max(at, 1), 0xFFFFFFFF, U32)  # unwritten entries: index 32767, distance 511
    for q, l in enumerate(lists):
        ent[off[q]:off[q] + len(l)] = l
    return ent, off, cnt, at


def case(form, lists, nf, observed=None, blocked=None, q_angle=None, t_angle=None, q_slot=None, slots_in=None,
         q_valid=None, check=1, nnratio=0.8, rng=None):
    nq = len(lists)
    ent, off, cnt, n_ent = layout(lists, rng)
    return dict(form=form, nq=nq, nf=nf, n_ent=n_ent, ent=ent, off=off, cnt=cnt,
                q_valid=None if q_valid is None else np.ascontiguousarray(q_valid, U8),
                observed=None if observed is None else np.ascontiguousarray(observed, U8),
                blocked=None if blocked is None else np.ascontiguousarray(blocked, U8),
                q_angle=np.zeros(nq, F32) if q_angle is None else np.ascontiguousarray(q_angle, F32),
                t_angle=np.zeros(nf, F32) if t_angle is None else np.ascontiguousarray(t_angle, F32),
                q_slot=(np.arange(nq) + 1000).astype(I32) if q_slot is None else np.ascontiguousarray(q_slot, I32),
                slots_in=None if slots_in is None else np.ascontiguousarray(slots_in, I32),
                check=int(check), nnratio=float(nnratio))


def _p(a):
    return None if a is None or a.size == 0 else a.ctypes.data_as(C.c_void_p)


def run(c):
    nf = c["nf"]
    out = {}
    for side in ("ref", "dev"):
        out[side] = dict(tm=np.full(max(nf, 1), 0x55555555, I32), tb=np.full(max(nf, 1), 0x55, U8),
                         edges=np.zeros(max(2 * nf, 1), I32), info=np.zeros(34, I32))
    r, d = out["ref"], out["dev"]
    lib().walkcore_case(c["form"], c["nq"], nf, c["n_ent"], _p(c["ent"]), _p(c["off"]), _p(c["cnt"]), _p(c["q_valid"]),
                        _p(c["observed"]), _p(c["blocked"]), _p(c["q_angle"]), _p(c["t_angle"]), _p(c["q_slot"]),
                        _p(c["slots_in"]), c["check"], c["nnratio"], _p(r["tm"]), _p(r["tb"]), _p(r["edges"]), _p(r["info"]),
                        _p(d["tm"]), _p(d["tb"]), _p(d["edges"]), _p(d["info"]))
    for s in (r, d):
        s["tm"], s["tb"], s["nmatches"], s["n_edges"] = s["tm"][:nf], s["tb"][:nf], int(s["info"][0]), int(s["info"][1])
        s["bins"] = s["info"][4:].copy()
        s["edge_feat"], s["edge_slot"] = s["edges"][:s["n_edges"]].copy(), s["edges"][nf:nf + s["n_edges"]].copy()
    r["overwrites"], r["dropped"] = int(r["info"][2]), int(r["info"][3])
    d["rounds"], d["flags"] = int(d["info"][2]), int(d["info"][3])
    return r, d


def overflow_status(off, cnt, cap):
    """(flags, overflow_sum, nmatches) of the round form for lists laid out in an array with `cap` overflow entries."""
    off, cnt, out = np.ascontiguousarray(off, I32), np.ascontiguousarray(cnt, I32), np.zeros(3, I32)
    lib().walkcore_overflow(len(cnt), _p(off), _p(cnt), int(cap), len(cnt) * INLINE + int(cap), _p(out))
    return tuple(int(v) for v in out)


def same(r, d):
    """What of the round form's result differs from the definition's ([] = nothing)."""
    bad = [k for k in ("nmatches", "n_edges") if r[k] != d[k]]
    bad += [k for k in ("tm", "tb", "edge_feat", "edge_slot", "bins") if r[k].tobytes() != d[k].tobytes()]
    if d["flags"] & 1:
        bad.append("overflow flag")
    return bad


ANGLES = np.array([0.0, 3.0, 14.9, 15.0, 29.0, 95.0, 200.0, 344.9, 345.0, 359.9], F32)
DISTS = np.array([0, 20, 40, 40, 60, 60, 80, 80, 90, 100, 100, 101, 120, 255])


def random_case(seed):
    rng = np.random.default_rng(seed)
    form = int(rng.integers(0, 2))
    nq = int(rng.integers(0, 301))
    nf = int(rng.integers(41, 401))
    spread = int(rng.choice([41, 60, 120]))  # how far around its centre a window reaches: small = colliding windows
    n_centres = int(rng.choice([1, 3, 20, 200]))
    centres = rng.integers(0, nf, n_centres)
    lists = []
    for q in range(nq):
        n = int(rng.integers(0, 41)) if rng.random() > 0.15 else 0
        idx = (centres[rng.integers(0, n_centres)] + rng.permutation(spread)[:n]) % nf
        lists.append(entry(idx, rng.choice(DISTS, n), rng.integers(0, 3, n)))
    p_obs, p_blk = rng.choice([0.0, 0.3, 0.7, 1.0]), rng.choice([0.0, 0.1, 0.5])
    return case(form, lists, nf, observed=None if rng.random() < 0.05 else rng.random(nq) < p_obs,
                blocked=None if p_blk == 0.0 and rng.random() < 0.5 else rng.random(nf) < p_blk,
                q_angle=rng.choice(ANGLES, nq), t_angle=rng.choice(ANGLES[:int(rng.integers(1, 11))], nf),
                q_slot=rng.integers(0, 5000, nq),
                slots_in=None if rng.random() < 0.5 else np.where(rng.random(nf) < 0.3, rng.integers(0, 5000, nf), -1),
                q_valid=None if form == LAST or rng.random() < 0.5 else rng.random(nq) < 0.9,
                check=int(rng.random() < 0.8), nnratio=float(rng.choice([0.6, 0.8, 1.0])), rng=rng)


N_RANDOM = 2000


@functools.lru_cache(maxsize=None)
def random_cases():
    """The seeded set, generated once per process; nobody writes to a case."""
    return tuple(random_case(seed) for seed in range(N_RANDOM))


def directed():
    """name -> case; the serial definition's outcome that makes each one what its name says is asserted by the tests."""
    D = {}
    D["no_queries"] = case(LAST, [], 50, slots_in=np.where(np.arange(50) % 7 == 0, np.arange(50), -1))
    D["no_queries_local"] = case(LOCAL, [], 50, slots_in=np.where(np.arange(50) % 7 == 0, np.arange(50), -1))
    D["empty_lists"] = case(LAST, [entry([], [])] * 37, 50, observed=np.ones(37))
    D["empty_lists_local"] = case(LOCAL, [entry([], [])] * 37, 50, observed=np.ones(37))
    # 64 observed queries on one shared list of 70 features with ascending distances: query k ends on feature k
    shared = entry(np.arange(70), np.arange(70))
    D["pile_up_64"] = case(LAST, [shared] * 64, 80, observed=np.ones(64))
    D["pile_up_64_local"] = case(LOCAL, [entry(np.arange(70), np.arange(70), np.arange(70) % 2)] * 64, 80,
                                 observed=np.ones(64))
    # two unobserved claimants, then an observed one, then a query that finds the feature blocked
    one = entry([5, 6], [10, 30])
    D["last_writer"] = case(LAST, [one, one, one, one], 10, observed=[0, 0, 1, 1], check=0)
    # feature 3 is claimed in a losing bin (query 0, unobserved) and in a winning one (query 1): it ends unmatched
    lists = [entry([3], [10]), entry([3], [10])] + [entry([10 + k], [10]) for k in range(12)]
    D["win_and_lose"] = case(LAST, lists, 30, observed=[0] + [1] * 13, q_angle=[95.0] + [0.0] * 13, check=1)
    # max2 < 0.1 * max1: 21 claims in bin 0, 2 in bin 3, 1 in bin 7 -> only bin 0 survives
    lists = [entry([k], [10]) for k in range(24)]
    D["one_maximum"] = case(LAST, lists, 30, observed=np.ones(24), q_angle=[0.0] * 21 + [95.0] * 2 + [200.0], check=1)
    # angles inside [0, 360) never reach bin 30 (factor = 1 / 30); rot = 900 does: bin == 30 wraps to 0 and joins the ten
    # claims there
    D["bin_wrap"] = case(LAST, lists, 30, observed=np.ones(24), q_angle=[0.0] * 10 + [900.0] * 11 + [95.0] * 3, check=1)
    # local form: equal levels with the best exactly at nnratio * second (0.5f * 80 = 40), accepted; one above, refused
    D["ratio_edge"] = case(LOCAL, [entry([1, 2], [40, 80], [1, 1]), entry([3, 4], [41, 80], [1, 1]),
                                   entry([5, 6], [41, 80], [1, 2])], 10, observed=[1, 1, 1], nnratio=0.5)
    # the second best of query 1 is blocked by query 0's claim: without feature 1 its ratio test passes
    D["second_blocked"] = case(LOCAL, [entry([1], [30]), entry([2, 1, 3], [50, 55, 90], [1, 1, 1])], 10, observed=[1, 1],
                               nnratio=0.8)
    D["second_open"] = case(LOCAL, [entry([1], [30]), entry([2, 1, 3], [50, 55, 90], [1, 1, 1])], 10, observed=[0, 1],
                            nnratio=0.8)
    return D


# ---- cases past one trip of the workgroup's loops (k_track_walk: 1024 lanes) and at its LDS cap.  A case may carry two
# keys more than case() gives it: "min_matches" (Args::min_matches, else 0) and "slot_observed" (the store's flags per slot:
# with them and without a blocked array the kernel derives "blocked on entry" itself; reference() restates that).
N_STORE = 5000
LANES = 1024  # kWalkThreads of csrc/vsg_track.hip
ST_OVERFLOW, ST_FEW_MATCHES, ST_FEW_EDGES = 1, 2, 4  # walkdev::kSt*


def lds_bytes(nq, nf):
    """walk_lds_bytes of csrc/vsg_track.hip: claim[nf], tm[nf], choice[nq] and kScratchInts = 40 words, then the bytes
    observed[nq], q_valid[nq], blocked[nf]."""
    return (2 * nf + nq + 40) * 4 + 2 * nq + nf


LDS_STATIC, LDS_MAX = 64, 64 * 1024  # kWalkStaticLds (wsum: one word per wave of 64), kWalkLdsMax


def over_cap(nq, nf):
    """the refusal of the chain calls and of the hook: VSG_ERR_CAPACITY"""
    return lds_bytes(nq, nf) + LDS_STATIC > LDS_MAX


# the largest accepted shapes with many queries and with many features (65534 bytes each), and one query more (65540)
CAP_SHAPES = {"cap_queries": (7885, 2000), "cap_features": (385, 7000)}
OVER_CAP_SHAPES = {"over_cap_queries": (7886, 2000), "over_cap_features": (386, 7000)}
BIG_SHAPES = ((1500, 1023), (1500, 1024), (1500, 1025), (3000, 2049))


def _windows(rng, nq, nf):
    """random_case's lists without its size limits: 0 .. 40 entries (15 % of the lists empty) out of a window of 60
    features around the query's own centre, modulo nf"""
    lists = []
    for _ in range(nq):
        n = int(rng.integers(0, 41)) if rng.random() > 0.15 else 0
        idx = (int(rng.integers(0, nf)) + rng.permutation(60)[:n]) % nf
        lists.append(entry(idx, rng.choice(DISTS, n), rng.integers(0, 3, n)))
    return lists


def big_case(form, nq, nf, seed):
    rng = np.random.default_rng(seed)
    lists = _windows(rng, nq, nf)
    blocked = rng.random(nf) < 0.1
    slots_in = np.where(rng.random(nf) < 0.3, rng.integers(0, N_STORE, nf), -1)
    blocked[nf - 1], slots_in[nf - 1] = True, 4999  # the last feature is always in the edge list, and nobody claims it
    return case(form, lists, nf, observed=rng.random(nq) < 0.7, blocked=blocked, q_angle=rng.choice(ANGLES, nq),
                t_angle=rng.choice(ANGLES, nf), q_slot=rng.integers(0, N_STORE, nq), slots_in=slots_in,
                q_valid=None if form == LAST else rng.random(nq) < 0.9, check=1, nnratio=0.8, rng=rng)


@functools.lru_cache(maxsize=None)
def big_cases():
    """name -> case: both forms at BIG_SHAPES; nobody writes to a case."""
    return {"big_%s_%d_%d" % ("last" if form == LAST else "local", nq, nf): big_case(form, nq, nf, 7 + nf)
            for form in (LAST, LOCAL) for nq, nf in BIG_SHAPES}


@functools.lru_cache(maxsize=None)
def cap_cases():
    """name -> case, local form: CAP_SHAPES (accepted) and OVER_CAP_SHAPES (refused)."""
    return {name: big_case(LOCAL, nq, nf, 11 + nf) for name, (nq, nf) in {**CAP_SHAPES, **OVER_CAP_SHAPES}.items()}


def from_slots(nf):
    """Local form without a blocked array: the features' entry slots and the store's observed flags (about half set) stand
    for it.  The queries' observed flags are their own points'."""
    rng = np.random.default_rng(500 + nf)
    nq = 40 if nf < 1000 else 3000
    slot_observed = (rng.random(N_STORE) < 0.5).astype(U8)
    q_slot = rng.integers(0, N_STORE, nq)
    c = case(LOCAL, _windows(rng, nq, nf), nf, observed=slot_observed[q_slot] != 0, q_slot=q_slot,
             slots_in=np.where(rng.random(nf) < 0.6, rng.integers(0, N_STORE, nf), -1), q_valid=rng.random(nq) < 0.9,
             check=0, nnratio=0.8, rng=rng)
    c["slot_observed"] = slot_observed
    return c


def blocked_from_slots(c):
    """what k_track_walk's prologue derives (ORBmatcher.cc:86-88): the entry slot's point is observed"""
    si = c["slots_in"]
    return ((si >= 0) & (c["slot_observed"][np.maximum(si, 0)] != 0)).astype(U8)


def single_claims(form, n, min_matches=0):
    """n queries with one candidate each, query k on feature k: n matches and n edges"""
    c = case(form, [entry([k], [10]) for k in range(n)], 30, observed=np.ones(n), check=0)
    c["min_matches"] = min_matches
    return c


@functools.lru_cache(maxsize=None)
def directed_high():
    """name -> case: the directed cases that need the hook's extra arguments or more than one trip of the workgroup's loops."""
    D = {}
    # pile_up_64 behind 1024 queries with empty lists: the claimants are lanes 0 .. 63 of the loops' SECOND trip
    empty = [entry([], [])] * LANES
    observed = np.arange(LANES + 64) >= LANES
    D["pile_up_high"] = case(LAST, empty + [entry(np.arange(70), np.arange(70))] * 64, 80, observed=observed)
    D["pile_up_high_local"] = case(LOCAL, empty + [entry(np.arange(70), np.arange(70), np.arange(70) % 2)] * 64, 80,
                                   observed=observed)
    D["from_slots_50"], D["from_slots_2049"] = from_slots(50), from_slots(2049)
    D["few_matches_19"], D["few_matches_20"] = single_claims(LAST, 19, 20), single_claims(LAST, 20, 20)
    D["few_edges_2"], D["few_edges_3"] = single_claims(LOCAL, 2), single_claims(LOCAL, 3)
    return D


def reference(c):
    """run() on the case as the serial definition has to be given it: (ref, dev)"""
    if c.get("slot_observed") is not None and c["blocked"] is None:
        c = dict(c, blocked=blocked_from_slots(c))
    return run(c)


def status_flags(ref, c):
    """the flags of walkdev::Status from the definition's counts (no overflow)"""
    return (ST_FEW_MATCHES if ref["nmatches"] < c.get("min_matches", 0) else 0) | (ST_FEW_EDGES if ref["n_edges"] < 3 else 0)


def feat_slots_of(ref, c):
    """the caller-side rule per feature: the claimant's q_slot, else slots_in, else -1"""
    tm = ref["tm"]
    qs = np.append(c["q_slot"], -1) if c["q_slot"] is not None else np.full(c["nq"] + 1, -1, I32)
    si = c["slots_in"] if c["slots_in"] is not None else np.full(c["nf"], -1, I32)
    return np.where(tm >= 0, qs[np.maximum(tm, 0)], si).astype(I32)


def record(c):
    """One case as tests/_walkcore/walk_sanitized.cpp reads it."""
    def pad(b):
        return b + b"\0" * (-len(b) % 4)
    has = (1 if c["q_valid"] is not None else 0) | (2 if c["blocked"] is not None else 0) | \
        (4 if c["slots_in"] is not None else 0) | (8 if c["observed"] is not None else 0)
    head = np.array([c["form"], c["nq"], c["nf"], c["n_ent"], c["check"], has,
                     np.array([c["nnratio"]], F32).view(I32)[0], 0], I32)
    parts = [head.tobytes(), c["ent"][:c["n_ent"]].tobytes(), c["off"].tobytes(), c["cnt"].tobytes()]
    for k in ("q_valid", "observed", "blocked"):
        if c[k] is not None:
            parts.append(pad(c[k].tobytes()))
    parts += [c["q_angle"].tobytes(), c["t_angle"].tobytes(), c["q_slot"].tobytes()]
    if c["slots_in"] is not None:
        parts.append(c["slots_in"].tobytes())
    return b"".join(parts)
