"""CPU tests of the epipolar predicate of SearchForTriangulation: tests/epipolar_reference.py (written from
ORBmatcher.cc:976-1073 and Pinhole.cpp:126-140) against visual_sgraphs_amd/csrc/vsg_epipolar.h compiled for the host by
tests/_epipolarcore, reason code for reason code, and both against cases worked out by hand.  The parity scene of the GPU
tests (tests/epipolar_scenes.py) is checked here against the restatement alone."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import epipolar_reference as er
import epipolar_scenes as es

F32 = np.float32
EC_DIR = Path(__file__).resolve().parent / "_epipolarcore"
_f32p, _u8p, _i32p = (C.POINTER(t) for t in (C.c_float, C.c_uint8, C.c_int32))
SF = (F32(1.2) ** np.arange(8, dtype=F32)).astype(F32)
SIGMA2 = (SF * SF).astype(F32)


@pytest.fixture(scope="module")
def ec():
    subprocess.check_call(["make", "-C", str(EC_DIR)], stdout=subprocess.DEVNULL)
    L = C.CDLL(str(EC_DIR / "libvsg_epipolarcore.so"))
    L.ec_pair_reasons.restype = None
    L.ec_pair_reasons.argtypes = [C.c_int] + [_f32p] * 6 + [_i32p] + [_f32p] * 4 + [C.c_int, C.c_int, _u8p]
    L.ec_gate_radius.restype, L.ec_gate_radius.argtypes = C.c_float, [C.c_float]
    L.ec_chi_square_bound.restype, L.ec_chi_square_bound.argtypes = C.c_double, [C.c_float]
    return L


def host_reasons(ec, x1, y1, ur1, x2, y2, ur2, octave2, F12, ep, sf, sigma2, only_stereo, coarse):
    a = [np.ascontiguousarray(np.broadcast_to(np.asarray(v, F32), np.shape(x2)), F32).reshape(-1)
         for v in (x1, y1, ur1, x2, y2, ur2)]
    o = np.ascontiguousarray(np.broadcast_to(np.asarray(octave2, np.int32), np.shape(x2)), np.int32).reshape(-1)
    F, e = np.ascontiguousarray(F12, F32).reshape(9), np.ascontiguousarray(ep, F32).reshape(2)
    sf, s2 = np.ascontiguousarray(sf, F32), np.ascontiguousarray(sigma2, F32)
    out = np.full(len(o), 255, np.uint8)
    ec.ec_pair_reasons(len(o), *[v.ctypes.data_as(_f32p) for v in a], o.ctypes.data_as(_i32p), F.ctypes.data_as(_f32p),
                       e.ctypes.data_as(_f32p), sf.ctypes.data_as(_f32p), s2.ctypes.data_as(_f32p), int(only_stereo),
                       int(coarse), out.ctypes.data_as(_u8p))
    return out


def both(ec, x1, y1, ur1, x2, y2, ur2, octave2, F12, ep, only_stereo=False, coarse=False, sf=SF, sigma2=SIGMA2):
    """Restatement and host build on the same pairs; they must agree, the restatement's codes are returned."""
    shape = np.shape(x2)
    args = [np.broadcast_to(np.asarray(v, F32), shape) for v in (x1, y1, ur1, x2, y2, ur2)]
    o = np.broadcast_to(np.asarray(octave2), shape)
    ref = er.pair_reasons(*args, o, F12, ep, sf, sigma2, only_stereo, coarse)
    got = host_reasons(ec, *args, o, F12, ep, sf, sigma2, only_stereo, coarse)
    assert ref.dtype == got.dtype == np.uint8 and np.array_equal(ref, got), np.flatnonzero(ref != got)[:10]
    return ref


def neighbours(v, k):
    """The 2k + 1 floats around v, in order."""
    i = np.asarray(v, F32).view(np.int32).astype(np.int64) + np.arange(-k, k + 1)
    return i.astype(np.int32).view(F32)


def test_parity_scene_meets_its_conditions_and_the_host_build_agrees_on_every_pair(ec):
    s = es.frames()
    legs = [es.leg_scene(s, leg) for leg in es.LEGS]
    kept, asked = er.check_scene(legs)
    assert asked >= 100
    for name, ref in zip(es.LEGS, legs):
        key, only_stereo, coarse, u1, u2 = es.LEGS[name]
        ur1 = s["ur1"] if u1 else np.full(len(s["k1"]), -1, F32)
        ur2 = s["ur2"] if u2 else np.full(len(s["k2"]), -1, F32)
        i1, i2 = ref["i1"], ref["i2"]
        got = host_reasons(ec, s["k1"]["x"][i1], s["k1"]["y"][i1], ur1[i1], s["k2"]["x"][i2], s["k2"]["y"][i2], ur2[i2],
                           s["k2"]["octave"][i2], s[key], s["ep"], s["sf"], s["sigma2"], only_stereo, coarse)
        assert np.array_equal(got, ref["reason"]), name
    # the FeatureVector shapes the kernel's paths need
    n1 = dict(zip(s["fv1"][0].tolist(), np.diff(s["fv1"][1]).tolist()))
    n2 = dict(zip(s["fv2"][0].tolist(), np.diff(s["fv2"][1]).tolist()))
    shared = sorted(set(n1) & set(n2))
    assert 8 <= len(n1) <= 16 and 8 <= len(n2) <= 16 and set(n1) - set(n2) and set(n2) - set(n1)
    assert any(n1[i] > es.TILE and n2[i] > es.TILE for i in shared) and any(64 < n2[i] <= es.TILE for i in shared)
    assert any(n1[i] == 1 for i in shared) and any(n2[i] == 1 for i in shared)
    assert 0.2 < (s["ur1"] >= 0).mean() < 0.45 and 0.2 < (s["ur2"] >= 0).mean() < 0.45


@pytest.mark.parametrize("seed", range(4))
def test_host_build_is_bit_equal_to_the_restatement_on_random_geometry(ec, seed):
    """General matrices (rotation included), every flag combination; all five codes must occur over the legs."""
    rng = np.random.default_rng(seed)
    n = 20000
    x1, y1 = rng.uniform(0, 640, n).astype(F32), rng.uniform(0, 480, n).astype(F32)
    ang = rng.normal(0, 0.02, 3)
    R = np.eye(3) + np.array([[0, -ang[2], ang[1]], [ang[2], 0, -ang[0]], [-ang[1], ang[0], 0]])
    t = rng.normal(0, 1, 3)
    K = np.array([[500.0, 0, 320], [0, 500.0, 240], [0, 0, 1]])
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    F12 = (np.linalg.inv(K).T @ tx @ R @ np.linalg.inv(K)).astype(F32)
    # x2 near the line of x1: a point of the line plus noise of a few pixels
    l = np.stack([x1, y1, np.ones(n, F32)], 1).astype(np.float64) @ F12.astype(np.float64)
    nrm = np.hypot(l[:, 0], l[:, 1])
    foot = np.stack([-l[:, 0] * l[:, 2], -l[:, 1] * l[:, 2]], 1) / (nrm ** 2)[:, None]
    along = np.stack([-l[:, 1], l[:, 0]], 1) / nrm[:, None] * rng.uniform(-300, 300, n)[:, None]
    x2 = (foot + along + (l[:, :2] / nrm[:, None]) * rng.normal(0, 2.5, n)[:, None]).astype(F32)
    ep = x2[0] + F32(3)
    ur1 = np.where(rng.random(n) < 0.3, x1 - 5, -1).astype(F32)
    ur2 = np.where(rng.random(n) < 0.3, x2[:, 0] - 5, -1).astype(F32)
    x2[1::50] = x2[0] + rng.normal(0, 6, (len(x2[1::50]), 2)).astype(F32)  # a cluster round the epipole
    ur1[1::50], ur2[1::50] = -1, -1
    octave = rng.integers(0, 8, n)
    seen = set()
    for only_stereo in (False, True):
        for coarse in (False, True):
            seen |= set(both(ec, x1, y1, ur1, x2[:, 0], x2[:, 1], ur2, octave, F12, ep, only_stereo, coarse).tolist())
    zero = both(ec, x1, y1, ur1, x2[:, 0], x2[:, 1], ur2, octave, np.zeros(9, F32), ep)
    assert seen == {er.PASS, er.NOT_STEREO, er.EPIPOLE_GATE, er.CHI_SQUARE} and er.DEN_ZERO in set(zero.tolist())


LINE_Y = np.array([[0, 0, 0], [0, 0, 0], [0, 1, 0]], F32)  # a = 0, b = 1, c = 0: num = y2, den = 1, dsqr = y2 * y2
FAR = np.array([1e6, 1e6], F32)                            # an epipole nowhere near: the gate never fires


def test_zero_matrix_is_den_zero_everywhere(ec):
    x2 = np.linspace(0, 300, 64, dtype=F32)
    r = both(ec, 10.0, 20.0, -1.0, x2, x2, -1.0, 0, np.zeros(9, F32), FAR)
    assert (r == er.DEN_ZERO).all()
    # ... unless coarse: the constraint is not evaluated at all
    assert (both(ec, 10.0, 20.0, -1.0, x2, x2, -1.0, 0, np.zeros(9, F32), FAR, coarse=True) == er.PASS).all()


def test_one_stereo_side_is_exempt_from_the_epipole_gate_which_also_applies_under_coarse(ec):
    ep = np.array([100.0, 50.0], F32)
    x2, y2 = np.array([103.0] * 4, F32), np.array([54.0] * 4, F32)  # 5 px from the epipole: 25 < 100
    ur1 = np.array([-1, 7, -1, 7], F32)
    ur2 = np.array([-1, -1, 9, 9], F32)
    for coarse in (False, True):
        r = both(ec, 0.0, 0.0, ur1, x2, y2, ur2, 0, LINE_Y, ep, coarse=coarse, sigma2=np.full(8, 1e9, F32))
        assert r.tolist() == [er.EPIPOLE_GATE, er.PASS, er.PASS, er.PASS], coarse
    # uright == 0 is stereo (>= 0), -0.0 too; a NaN is mono
    r = both(ec, 0.0, 0.0, np.array([0.0, -0.0, np.nan], F32), x2[:3], y2[:3], -1.0, 0, LINE_Y, ep, sigma2=np.full(8, 1e9, F32))
    assert r.tolist() == [er.PASS, er.PASS, er.EPIPOLE_GATE]


def test_only_stereo_needs_both_sides_stereo_and_comes_first(ec):
    ep = np.array([100.0, 50.0], F32)
    ur1 = np.array([-1, 7, -1, 7], F32)
    ur2 = np.array([-1, -1, 9, 9], F32)
    # on top of the epipole and far from the line: still code 1 for the mono pairs; the stereo pair goes on to the line test
    r = both(ec, 0.0, 0.0, ur1, 100.0 * np.ones(4, F32), 50.0 * np.ones(4, F32), ur2, 0, LINE_Y, ep, only_stereo=True)
    assert r.tolist() == [er.NOT_STEREO] * 3 + [er.CHI_SQUARE]
    r = both(ec, 0.0, 0.0, ur1, 100.0 * np.ones(4, F32), np.ones(4, F32), ur2, 0, LINE_Y, ep, only_stereo=True)
    assert r.tolist() == [er.NOT_STEREO] * 3 + [er.PASS]


def test_nan_in_the_matrix_rejects(ec):
    x2 = np.linspace(0, 300, 16, dtype=F32)
    for at in range(9):
        F = LINE_Y.copy().reshape(9)
        F[at] = np.nan
        r = both(ec, 10.0, 20.0, 5.0, x2, np.zeros(16, F32), 5.0, 0, F, FAR)
        # a NaN never compares below the bound (and never equal to zero): chi-square
        assert (r == er.CHI_SQUARE).all(), at
    r = both(ec, 10.0, 20.0, 5.0, x2, np.zeros(16, F32), 5.0, 0, LINE_Y, FAR)
    assert (r == er.PASS).all()


@pytest.mark.parametrize("level", range(8))
def test_dsqr_one_ulp_either_side_of_the_chi_square_bound(ec, level):
    """dsqr = y2 * y2 (one rounding).  The bound 3.84 * (double)sigma2 is no float: T = the largest float below it passes,
    the next float up fails.  The y2 that square to exactly T and to exactly T's successor are searched for among the
    floats around sqrt(T) for a dozen scales b of the line (num = fl(b * y2), den = fl(b * b)); the
    comparison is in double, so the float just below the bound passes even where (float)bound equals it."""
    bound = np.float64(3.84) * np.float64(SIGMA2[level])
    assert ec.ec_chi_square_bound(float(SIGMA2[level])) == bound
    T = F32(bound)
    if np.float64(T) >= bound:
        T = np.nextafter(T, F32(0))
    up = np.nextafter(T, F32(np.inf))
    assert np.float64(T) < bound <= np.float64(up)
    found = {}
    for b in (1.0, 1.25, 1.5, 1.75, 0.7, 0.9, 1.1, 1.3, 1.7, 2.3, 3.1, 5.3):
        F = np.array([[0, 0, 0], [0, 0, 0], [0, 0, 0]], F32)
        F[2, 1] = b   # a = 0, b = b, c = 0: num = fl(b * y2), den = fl(b * b), dsqr = fl(fl(num * num) / den)
        y2 = neighbours(F32(np.sqrt(np.float64(T))), 4000)
        num = (F32(b) * y2).astype(F32)
        dsqr = ((num * num).astype(F32) / F32(F32(b) * F32(b))).astype(F32)
        r = both(ec, 3.0, 4.0, 5.0, np.zeros_like(y2), y2, 5.0, level, F, FAR)
        assert np.array_equal(r == er.PASS, dsqr.astype(np.float64) < bound)
        for want, code in ((T, er.PASS), (up, er.CHI_SQUARE)):
            hit = np.flatnonzero(dsqr == want)
            if len(hit):
                assert (r[hit] == code).all()
                found[code] = True
    assert found == {er.PASS: True, er.CHI_SQUARE: True}


@pytest.mark.parametrize("level", range(8))
def test_gate_distance_one_ulp_either_side_of_the_radius(ec, level):
    """distex^2 + distey^2 < 100 * sf: the float just below the radius is gated, the radius itself is not."""
    gate = F32(F32(100) * SF[level])
    assert ec.ec_gate_radius(float(SF[level])) == gate
    below = np.nextafter(gate, F32(0))
    # dy takes most of the distance and the epipole sits near x = 0, so that dx and x2 are small numbers: one step of x2
    # moves dx * dx by less than an ulp of the sum, and every float round the radius is reached
    ep = np.array([4.0, 100.0], F32)
    found = {}
    top = np.floor(np.sqrt(np.float64(gate) - 1.0) * 4) / 4
    for dy in (top, top - 0.25, top - 0.5):   # dy * dy is exact
        dx0 = np.sqrt(np.float64(gate) - dy * dy)
        x2 = neighbours(F32(4.0 - dx0), 3000)
        dx = (ep[0] - x2).astype(F32)
        d2 = ((dx * dx).astype(F32) + F32(dy * dy)).astype(F32)
        r = both(ec, 0.0, 0.0, -1.0, x2, np.full_like(x2, 100.0 - dy), -1.0, level, LINE_Y, ep, coarse=True)
        assert np.array_equal(r == er.EPIPOLE_GATE, d2 < gate)
        for want, code in ((below, er.EPIPOLE_GATE), (gate, er.PASS)):
            hit = np.flatnonzero(d2 == want)
            if len(hit):
                assert (r[hit] == code).all()
                found[code] = True
    assert found == {er.EPIPOLE_GATE: True, er.PASS: True}


def test_bitmask_layout_is_that_of_the_existing_search():
    """bit pair_off[s] + i1 * n2(s) + i2 of the s-th shared node, nodes in ascending id."""
    k = np.zeros(5, [("x", F32), ("y", F32), ("octave", np.int32)])
    k["y"] = [0, 1, 1.5, 50, 60]   # dsqr = y2^2 against 3.84: rows 0, 1 and 2 pass
    fv1 = (np.array([2, 5, 9]), np.array([0, 2, 3, 5]), np.array([4, 0, 1, 2, 3]))
    fv2 = (np.array([5, 9]), np.array([0, 3, 5]), np.array([3, 1, 0, 2, 4]))
    d = np.zeros((5, 32), np.uint8)
    ref = er.scene(k, None, np.ones(5), fv1, d, k, np.full(5, 5.0, F32), np.ones(5), fv2, d, LINE_Y, FAR, SF, SIGMA2, False, False)
    assert ref["pair_off"].tolist() == [0, 3, 7]            # node 5: 1 x 3 pairs, node 9: 2 x 2
    assert ref["i1"].tolist() == [1, 1, 1, 2, 2, 3, 3] and ref["i2"].tolist() == [3, 1, 0, 2, 4, 2, 4]
    assert ref["reason"].tolist() == [4, 0, 0, 0, 4, 0, 4]
    assert ref["pair_ok"][0] == 0b0101110 and not ref["pair_ok"][1:].any()
