"""The cases of the argument check of vsg_mappoints_refresh_from_observations (visual_sgraphs_amd/csrc/vsg_obs_args.h), shared
by tests/test_observations_args.py (the host core loaded into Python), tests/test_sanitizers_observations.py (the same core as
a sanitized program) and the refusals of tests/test_gpu_mappoints_refresh.py (the library itself)."""
import numpy as np

I32 = np.int32
OK, UNSUPPORTED, INVALID = 0, -3, -6
KF_N = (1, 7, 64, 300, 300)  # features per keyframe
NLEVELS = 8
CAPACITY = 1000


def octaves():
    """Per keyframe: octaves that cover 0 .. 7, feature n - 1 of every keyframe at level 7."""
    out = []
    for k, n in enumerate(KF_N):
        o = ((np.arange(n) + k) % NLEVELS).astype(I32)
        o[n - 1] = NLEVELS - 1
        out.append(o)
    out[1][0] = 0
    return out


def base():
    """A valid call: 6 points; point 2 has no observation, point 4 one, point 5 observes idx = n - 1 of every keyframe and
    has kf = n_kf - 1 last."""
    lists = [[(1, 0), (2, 5), (3, 10)], [(0, 0), (4, 299)], [], [(2, 63), (3, 7), (4, 8), (1, 6)], [(3, 299)],
             [(0, 0), (1, 6), (2, 63), (3, 299), (4, 299)]]
    off = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(I32)
    kf = np.array([o[0] for l in lists for o in l], I32)
    idx = np.array([o[1] for l in lists for o in l], I32)
    return dict(slots=np.array([5, 0, 17, CAPACITY - 1, 400, 3], I32), off=off, kf=kf, idx=idx,
                bad=np.zeros(len(kf), np.uint8), ref_pos=np.array([0, 1, 0, 3, 0, 2], I32), kf_n=np.array(KF_N, I32),
                oct=octaves(), capacity=CAPACITY, nlevels=NLEVELS, use_bad=True)


def _long_list(count, n_bad=0):
    """One point with `count` observations that cycle through the keyframes, the last n_bad of them bad."""
    c = base()
    kf = (np.arange(count) % len(KF_N)).astype(I32)
    idx = (np.arange(count) % np.array(KF_N)[kf]).astype(I32)
    bad = np.zeros(count, np.uint8)
    if n_bad:
        bad[-n_bad:] = 1
    c.update(slots=np.array([9], I32), off=np.array([0, count], I32), kf=kf, idx=idx, bad=bad, ref_pos=np.array([0], I32))
    return c


def cases():
    """name -> (arguments, expected return code).  One accepted and one refused case per rule of the header."""
    out = {"valid": (base(), OK)}

    def variant(name, rc, **changes):
        c = base()
        for k, v in changes.items():
            if isinstance(v, tuple):  # (position, value) inside the array of that name
                a = c[k].copy()
                a[v[0]] = v[1]
                c[k] = a
            else:
                c[k] = v
        out[name] = (c, rc)

    b = base()
    # off starts at 0 and never descends (point 2's empty list, equal offsets, is part of "valid")
    variant("off0_is_1", INVALID, off=(0, 1))
    variant("off_descends", INVALID, off=(2, 6))
    # (kf, idx): kf in [0, n_kf), idx in [0, frames[kf].n)
    variant("kf_last", OK, kf=(0, 4), idx=(0, 299))
    variant("kf_is_n_kf", INVALID, kf=(0, 5))
    variant("kf_negative", INVALID, kf=(0, -1))
    variant("idx_last", OK, idx=(1, 63))
    variant("idx_is_n", INVALID, idx=(1, 64))
    variant("idx_is_n_of_the_one_feature_keyframe", INVALID, idx=(3, 1))
    variant("idx_negative", INVALID, idx=(1, -1))
    # slots
    variant("slot_last", OK, slots=(0, CAPACITY - 2))
    variant("slot_is_capacity", INVALID, slots=(0, CAPACITY))
    variant("slot_negative", INVALID, slots=(0, -1))
    variant("slot_twice", INVALID, slots=(4, 5))
    # ref_pos inside the list whenever the list is not empty
    variant("ref_last", OK, ref_pos=(0, 2))
    variant("ref_is_m", INVALID, ref_pos=(0, 3))
    variant("ref_negative", INVALID, ref_pos=(0, -1))
    variant("empty_list_needs_no_ref_pos", OK, ref_pos=(2, 12345))
    variant("empty_list_negative_ref_pos", OK, ref_pos=(2, -7))
    # the reference keypoint's octave < nlevels; another observation's octave is nobody's business
    lo = octaves()
    lo[1][0] = NLEVELS  # point 0's reference observation (kf 1, idx 0)
    variant("ref_octave_is_nlevels", INVALID, oct=lo)
    lo = octaves()
    lo[2][5] = NLEVELS + 3  # point 0's second observation, not the reference
    variant("other_octave_above_nlevels", OK, oct=lo)
    variant("ref_octave_last_level", OK, ref_pos=(4, 0))  # (3, 299): level 7
    # nlevels in [1, 16]
    flat = [np.zeros(n, I32) for n in KF_N]
    variant("nlevels_1", OK, nlevels=1, oct=flat)
    variant("nlevels_16", OK, nlevels=16)
    variant("nlevels_0", INVALID, nlevels=0, oct=flat)
    variant("nlevels_17", INVALID, nlevels=17)
    # at most 128 observations that are not bad
    out["good_128"] = (_long_list(128), OK)
    out["good_129"] = (_long_list(129), UNSUPPORTED)
    out["good_128_of_140"] = (_long_list(140, 12), OK)
    out["good_129_of_140"] = (_long_list(140, 11), UNSUPPORTED)
    c = _long_list(129)
    c["use_bad"] = False
    out["good_129_null_bad"] = (c, UNSUPPORTED)
    c = _long_list(129)
    c["ref_pos"] = np.array([129], I32)
    out["invalid_wins_over_unsupported"] = (c, INVALID)
    # bad == NULL: none is bad
    variant("null_bad", OK, use_bad=False)
    variant("all_bad", OK, bad=np.ones(len(b["kf"]), np.uint8))
    return out


def expected_good(c):
    bad = c["bad"] if c["use_bad"] else np.zeros(len(c["kf"]), np.uint8)
    return np.array([int((bad[c["off"][i]:c["off"][i + 1]] == 0).sum()) for i in range(len(c["slots"]))], I32)
