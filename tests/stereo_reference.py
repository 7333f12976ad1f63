"""NumPy restatement of Frame::ComputeStereoMatches (orb_slam3/src/Frame.cc:957-1127), the yardstick of k_stereo and of the
host median cut behind vsg_stereo_matches, vsg_frame_stereo_matches and vsg_frame_stereo_bow_search.

Written from those lines, one correctly rounded float32 operation where the reference has a float operation:

  the row band of every right keypoint                    Frame.cc:975-990   floor / ceil of y -+ 2 * mvScaleFactors[octave]
  octave gate, [minU, maxU], Hamming < TH_HIGH, first min Frame.cc:1000-1042
  best Hamming < (TH_HIGH + TH_LOW) / 2                   Frame.cc:1045
  roundf (half away from zero) of the scaled coordinates  Frame.cc:1049-1053  (np.round is round-half-even: not used)
  iniu / endu, 11 shifts of an 11 x 11 L1 SAD, first min  Frame.cc:1055-1085
  best shift at -L or +L, the parabola, deltaR in [-1, 1] Frame.cc:1087-1097
  disparity in [0, maxD); disparity <= 0 -> 0.01 and bestuR = uL - 0.01 IN DOUBLE, then float      Frame.cc:1100-1110
  the median cut: thDist = 1.5f * 1.4f * median, `<`      Frame.cc:1113-1126

Beside mvuRight and mvDepth it says WHY each left keypoint ended as it did (the reason codes below), which right keypoint, which
shift and which SAD were chosen -- what the directed scenes of tests/stereo_scenes.py are checked against.

Pyramid levels are those of OracleExtractor.pyramid_level(l, with_border=True): the reference's mvImagePyramid with its 19 px
reflected border.  window_guard=True adds the one deviation of the device (stereo section): a keypoint whose left
11 x 11 window or right 11 x 21 strip leaves the un-bordered level gets no match (reason WINDOW) and no say in the median."""
import numpy as np

F32 = np.float32
BORDER = 19
(NO_CANDIDATE, OCTAVE_GATE, U_WINDOW, HAMMING_HIGH, BEST_HAMMING, ENDU, SHIFT_EDGE, DELTA_R, DISPARITY_RANGE, CLAMPED,
 MEDIAN_CUT, MATCHED, WINDOW) = range(13)
REFERENCE_REASONS = tuple(range(12))  # every outcome the reference has; WINDOW is the device's own
REASON_NAMES = ("no candidate in the row band", "octave gate", "u window", "Hamming >= 100", "best Hamming >= 75", "endu",
                "best shift at +-L", "deltaR", "disparity range", "clamped to 0.01", "cut by the median", "matched", "window")
TH_HIGH, TH_LOW = 100, 50
TH_ORB = (TH_HIGH + TH_LOW) // 2
W, L = 5, 5


def roundf(v):
    """C roundf of a float32: half away from zero.  |v| + 0.5 is exact in float64 for every float32 of image size."""
    v = np.float64(F32(v))
    return F32(np.copysign(np.floor(np.abs(v) + 0.5), v))


def pyramids(extractor):
    """The bordered levels of an OracleExtractor that has just run."""
    return [extractor.pyramid_level(l, with_border=True) for l in range(extractor.nlevels)]


def hamming(d, D):
    return np.unpackbits(np.bitwise_xor(np.asarray(D, np.uint8), np.asarray(d, np.uint8)), axis=-1).sum(-1).astype(np.int64)


def row_band(kr, scale):
    """(minr, maxr) of every right keypoint (Frame.cc:981-985)."""
    y = kr["y"].astype(F32)
    r = (F32(2.0) * np.asarray(scale, F32)[kr["octave"]]).astype(F32)
    return np.floor((y - r).astype(F32)).astype(np.int64), np.ceil((y + r).astype(F32)).astype(np.int64)


def sad_profile(img_l, img_r, ily, ilx, scaled_ur0):
    """The 11 float SADs of Frame.cc:1067-1085 on bordered levels (ily, ilx, irx are un-bordered coordinates)."""
    b = BORDER
    il = img_l[b + ily:b + ily + 2 * W + 1, b + ilx:b + ilx + 2 * W + 1].astype(np.int64)
    out = np.zeros(2 * L + 1, F32)
    for inc in range(-L, L + 1):
        irx = int(F32(F32(scaled_ur0 + F32(inc)) - F32(W)))
        ir = img_r[b + ily:b + ily + 2 * W + 1, b + irx:b + irx + 2 * W + 1].astype(np.int64)
        out[L + inc] = F32(int(np.abs(il - ir).sum()))
    return out


def median_cut(sads):
    """Frame.cc:1113-1126 on [(sad, iL)]: the iL that are cut."""
    if not sads:
        return []
    order = sorted(sads)
    median = F32(order[len(order) // 2][0])
    th = F32(F32(F32(1.5) * F32(1.4)) * median)
    cut = []
    for sad, i in reversed(order):
        if F32(sad) < th:
            break
        cut.append(i)
    return cut


def compute(pyr_l, pyr_r, scale, inv_scale, kl, dl, kr, dr, mb, mbf, window_guard=False):
    scale, inv_scale = np.asarray(scale, F32), np.asarray(inv_scale, F32)
    nl, nr = len(kl), len(kr)
    dl, dr = np.asarray(dl, np.uint8).reshape(-1, 32), np.asarray(dr, np.uint8).reshape(-1, 32)
    mb, mbf = F32(mb), F32(mbf)
    n_rows = pyr_l[0].shape[0] - 2 * BORDER
    u_right, depth = np.full(nl, -1, F32), np.full(nl, -1, F32)
    reason = np.full(nl, NO_CANDIDATE, np.uint8)
    best_idx, best_inc, best_sad = np.full(nl, -1, np.int64), np.zeros(nl, np.int64), np.full(nl, -1, np.int64)
    best_ham, n_at_min, last_at_min = np.full(nl, -1, np.int64), np.zeros(nl, np.int64), np.full(nl, -1, np.int64)
    clamped = np.zeros(nl, bool)
    profiles = np.full((nl, 2 * L + 1), -1, F32)
    assert nr == 0 or (kr["octave"].min() >= 0 and kr["octave"].max() < len(scale))
    assert nl == 0 or (kl["octave"].min() >= 0 and kl["octave"].max() < len(scale))
    minr, maxr = row_band(kr, scale) if nr else (np.zeros(0, np.int64), np.zeros(0, np.int64))
    with np.errstate(all="ignore"):
        max_d = F32(mbf / mb)
        sads = []
        for i in range(nl):
            level = int(kl["octave"][i])
            vl, ul = F32(kl["y"][i]), F32(kl["x"][i])
            row = int(vl)  # (int)vL: truncation
            if row < 0 or row >= n_rows or nr == 0:
                continue
            in_band = (minr <= row) & (row <= maxr)
            if not in_band.any():
                continue
            min_u, max_u = F32(ul - max_d), F32(ul - F32(0))
            if max_u < 0:
                reason[i] = U_WINDOW
                continue
            octave_ok = in_band & (kr["octave"] >= level - 1) & (kr["octave"] <= level + 1)
            if not octave_ok.any():
                reason[i] = OCTAVE_GATE
                continue
            ur = kr["x"].astype(F32)
            cand = octave_ok & (ur >= min_u) & (ur <= max_u)
            if not cand.any():
                reason[i] = U_WINDOW
                continue
            idx = np.flatnonzero(cand)
            dist = hamming(dl[i], dr[idx])
            best = int(dist.min())
            if best >= TH_HIGH:
                reason[i] = HAMMING_HIGH
                continue
            at_min = idx[dist == best]
            j = int(at_min[0])  # `dist < bestDist`: the first minimum in index order
            best_idx[i], best_ham[i], n_at_min[i], last_at_min[i] = j, best, len(at_min), int(at_min[-1])
            if best >= TH_ORB:
                reason[i] = BEST_HAMMING
                continue
            sf = inv_scale[level]
            su_l, sv_l, su_r0 = roundf(F32(ul * sf)), roundf(F32(vl * sf)), roundf(F32(ur[j] * sf))
            ily, ilx = int(F32(sv_l - F32(W))), int(F32(su_l - F32(W)))
            iniu = F32(F32(su_r0 + F32(L)) - F32(W))
            endu = F32(F32(F32(su_r0 + F32(L)) + F32(W)) + F32(1))
            cols, rows = pyr_r[level].shape[1] - 2 * BORDER, pyr_r[level].shape[0] - 2 * BORDER
            if window_guard:
                iur = int(su_r0)
                if not (0 <= ily <= rows - 11 and 0 <= ilx <= cols - 11 and 10 <= iur <= cols - 11):
                    reason[i] = WINDOW
                    continue
            if iniu < 0 or endu >= cols:
                reason[i] = ENDU
                continue
            prof = sad_profile(pyr_l[level], pyr_r[level], ily, ilx, su_r0)
            profiles[i] = prof
            best_s, inc_best = 2 ** 31 - 1, 0
            for inc in range(-L, L + 1):
                if float(prof[L + inc]) < float(F32(best_s)):  # `dist < bestDistS`: float against an int
                    best_s, inc_best = int(prof[L + inc]), inc
            best_inc[i], best_sad[i] = inc_best, best_s
            if inc_best in (-L, L):
                reason[i] = SHIFT_EDGE
                continue
            d1, d2, d3 = prof[L + inc_best - 1], prof[L + inc_best], prof[L + inc_best + 1]
            delta = F32(F32(d1 - d3) / F32(F32(2.0) * F32(F32(d1 + d3) - F32(F32(2.0) * d2))))
            if delta < -1 or delta > 1:
                reason[i] = DELTA_R
                continue
            best_ur = F32(scale[level] * F32(F32(su_r0 + F32(inc_best)) + delta))
            disparity = F32(ul - best_ur)
            if not (disparity >= 0 and disparity < max_d):
                reason[i] = DISPARITY_RANGE
                continue
            reason[i] = MATCHED
            if disparity <= 0:
                disparity = F32(0.01)
                best_ur = F32(np.float64(ul) - np.float64(0.01))
                clamped[i], reason[i] = True, CLAMPED
            depth[i], u_right[i] = F32(mbf / disparity), best_ur
            sads.append((best_s, i))
    uncut_u, uncut_d = u_right.copy(), depth.copy()
    cut = median_cut(sads)
    for i in cut:
        u_right[i], depth[i], reason[i] = -1, -1, MEDIAN_CUT
    return dict(u_right=u_right, depth=depth, reason=reason, best_idx=best_idx, best_inc=best_inc, sad=best_sad,
                hamming=best_ham, n_at_min=n_at_min, last_at_min=last_at_min, clamped=clamped, profile=profiles,
                uncut_u_right=uncut_u, uncut_depth=uncut_d, count=len(sads) - len(cut), max_d=max_d)
