"""The argument check of vsg_mappoints_refresh_from_observations (vsg::obs_check of visual_sgraphs_amd/csrc/vsg_obs_args.h),
compiled for the host by tests/_obscore: every rule of the header with one accepted and one refused case (tests/obs_cases.py).
What the check accepts is all that ever reaches a device."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import obs_cases as oc

OC_DIR = Path(__file__).resolve().parent / "_obscore"
_i32p, _u8p = C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
CASES = oc.cases()


@pytest.fixture(scope="module")
def core():
    subprocess.check_call(["make", "-C", str(OC_DIR)], stdout=subprocess.DEVNULL)
    L = C.CDLL(str(OC_DIR / "libvsg_obscore.so"))
    L.oc_obs_check.restype = C.c_int
    L.oc_obs_check.argtypes = [C.c_int, _i32p, _i32p, _i32p, _i32p, _u8p, _i32p, C.c_int, _i32p, _i32p, C.c_int, C.c_int,
                               _i32p]
    return L


def run(core, c):
    p = lambda a, t=_i32p: np.ascontiguousarray(a).ctypes.data_as(t)
    keep = [np.ascontiguousarray(c[k], np.int32) for k in ("slots", "off", "kf", "idx", "ref_pos", "kf_n")]
    bad, octs = np.ascontiguousarray(c["bad"], np.uint8), np.ascontiguousarray(np.concatenate(c["oct"]), np.int32)
    good = np.full(len(keep[0]), -1, np.int32)
    rc = core.oc_obs_check(len(keep[0]), p(keep[0]), p(keep[1]), p(keep[2]), p(keep[3]), p(bad, _u8p) if c["use_bad"] else None,
                           p(keep[4]), len(keep[5]), p(keep[5]), p(octs), c["capacity"], c["nlevels"], p(good))
    return rc, good


@pytest.mark.parametrize("name", sorted(CASES))
def test_rule(core, name):
    c, want = CASES[name]
    rc, good = run(core, c)
    assert rc == want, name
    if want != oc.INVALID:
        assert np.array_equal(good, oc.expected_good(c))


def test_every_rule_has_an_accepted_and_a_refused_case():
    names = set(CASES)
    for accepted, refused in (("valid", "off0_is_1"), ("valid", "off_descends"), ("kf_last", "kf_is_n_kf"),
                              ("idx_last", "idx_is_n"), ("slot_last", "slot_is_capacity"), ("valid", "slot_twice"),
                              ("ref_last", "ref_is_m"), ("empty_list_needs_no_ref_pos", "ref_negative"),
                              ("ref_octave_last_level", "ref_octave_is_nlevels"), ("nlevels_1", "nlevels_0"),
                              ("nlevels_16", "nlevels_17"), ("good_128", "good_129")):
        assert {accepted, refused} <= names
        assert CASES[accepted][1] == oc.OK and CASES[refused][1] != oc.OK
    assert CASES["slot_twice"][1] == oc.INVALID and CASES["good_129"][1] == oc.UNSUPPORTED


def test_no_points_is_valid_whatever_the_pointers_are(core):
    assert core.oc_obs_check(0, None, None, None, None, None, None, 0, None, None, 10, 8, None) == oc.OK
    assert core.oc_obs_check(-1, None, None, None, None, None, None, 0, None, None, 10, 8, None) == oc.INVALID
    assert core.oc_obs_check(0, None, None, None, None, None, None, 0, None, None, 10, 0, None) == oc.INVALID
    # points, but no array
    assert core.oc_obs_check(2, None, None, None, None, None, None, 0, None, None, 10, 8, None) == oc.INVALID
