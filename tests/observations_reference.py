"""MapPoint::UpdateNormalAndDepth (MapPoint.cc:440-513, keyframes with NLeft == -1) restated in NumPy float32, and
MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:340-417) through the oracle, for the tests of
vsg_mappoints_refresh_from_observations.  Written from those lines: every operation below is one float32 operation with one
rounding, in the order DESIGN.md section 2 pins ((a0 b0 + a1 b1) + a2 b2 for a dot product, the sum over the observations
serial in list order, vector / scalar as a quotient per component)."""
import numpy as np

F32 = np.float32
DESC, NORMAL = 1, 2  # include/vsg_orb.h VSG_REFRESH_*


def _norm(d):
    return np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])  # float32 throughout: d is float32


def update_normal_and_depth(P, Ow_list, ref, ref_level, scale_factors, nlevels):
    """P [3], Ow_list [m, 3] = GetCameraCenter() of the observing keyframes in list order (m >= 1), ref = the position of
    mpRefKF in that list, ref_level = its keypoint's octave.  Returns (mNormalVector [3], mfMinDistance, mfMaxDistance)."""
    P, Ow_list, sf = np.asarray(P, F32), np.asarray(Ow_list, F32).reshape(-1, 3), np.asarray(scale_factors, F32)
    with np.errstate(invalid="ignore", divide="ignore"):
        normal = np.zeros(3, F32)                    # :459
        for Ow in Ow_list:                           # :461-474
            normali = P - Ow
            normal = normal + normali / _norm(normali)
        PC = P - Ow_list[ref]                        # :484
        dist = _norm(PC)                             # :485
        max_d = dist * sf[ref_level]                 # :509
        min_d = max_d / sf[nlevels - 1]              # :510
        normal = normal / F32(len(Ow_list))          # :511
    assert normal.dtype == F32 and max_d.dtype == F32 and min_d.dtype == F32
    return normal, F32(min_d), F32(max_d)


def distinctive_positions(desc_rows, off, bad=None):
    """desc_rows [total, 32]: the descriptor of every observation, CSR off [n + 1], bad [total] or None.  The oracle's
    ComputeDistinctiveDescriptors on every point's rows that are not bad (:363), mapped back to positions inside the
    point's list; -1 where no row is left (:379) or the list is empty (:354)."""
    import oracle_lib
    desc_rows, off = np.ascontiguousarray(desc_rows, np.uint8).reshape(-1, 32), np.asarray(off, np.int64)
    n = len(off) - 1
    good = np.ones(len(desc_rows), bool) if bad is None else np.asarray(bad) == 0
    keep = np.flatnonzero(good[:off[-1]])
    goff = np.concatenate([[0], np.cumsum([int(good[off[i]:off[i + 1]].sum()) for i in range(n)])]).astype(np.int32)
    chosen = oracle_lib.distinctive_descriptors(desc_rows[keep], goff)
    best = np.full(n, -1, np.int32)
    for i in range(n):
        if goff[i + 1] > goff[i]:
            best[i] = keep[goff[i] + chosen[i]] - off[i]
    return best


def medians(desc_rows):
    """The median every row of one point competes with (:400-404), for the conditions on a fixture."""
    d = np.unpackbits(np.ascontiguousarray(desc_rows, np.uint8).reshape(-1, 32), axis=1).astype(np.int32)
    D = (d[:, None, :] != d[None, :, :]).sum(axis=2)
    N = len(d)
    return np.sort(D, axis=1)[:, int(0.5 * (N - 1))]


def refresh(store, prob, what):
    """What vsg_mappoints_refresh_from_observations must leave behind.  store: dict of the WHOLE store's arrays before the
    call (world_pos, normal, min_dist, max_dist, desc); prob: slots, off, kf, idx, bad (or None), ref_pos, frames = list of
    (kps, desc) per keyframe, Ow [n_kf, 3], scale_factors.  Returns (store after, outs = dict(best, normal, min_dist,
    max_dist))."""
    after = {k: np.array(v, copy=True) for k, v in store.items()}
    off, kf, idx = (np.asarray(prob[k], np.int64) for k in ("off", "kf", "idx"))
    slots, sf = np.asarray(prob["slots"], np.int64), np.asarray(prob["scale_factors"], F32)
    n = len(slots)
    best = np.full(n, -1, np.int32)
    if what & DESC:
        rows = np.stack([prob["frames"][k][1][i] for k, i in zip(kf, idx)]) if len(kf) else np.zeros((0, 32), np.uint8)
        best = distinctive_positions(rows, off, prob.get("bad"))
        for i in np.flatnonzero(best >= 0):
            after["desc"][slots[i]] = rows[off[i] + best[i]]
    if what & NORMAL:
        for i in range(n):
            o, m = off[i], off[i + 1] - off[i]
            if m == 0:
                continue  # :455
            r = o + prob["ref_pos"][i]
            level = int(prob["frames"][kf[r]][0]["octave"][idx[r]])
            nrm, mn, mx = update_normal_and_depth(store["world_pos"][slots[i]], prob["Ow"][kf[o:o + m]], int(prob["ref_pos"][i]),
                                                  level, sf, len(sf))
            after["normal"][slots[i]], after["min_dist"][slots[i]], after["max_dist"][slots[i]] = nrm, mn, mx
    outs = {"best": best, "normal": after["normal"][slots], "min_dist": after["min_dist"][slots],
            "max_dist": after["max_dist"][slots]}
    return after, outs
