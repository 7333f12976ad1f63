"""CPU tests of tests/frustum_reference.py, the yardstick of the resident map-point path: Frame::isInFrustum
(Frame.cc:656-719) against cases worked out by hand, and the conditions the seeded scenarios of the GPU tests must meet."""
import numpy as np
import pytest

import frustum_reference as fr

F32 = np.float32
BOUNDS = (0.0, 0.0, 640.0, 480.0)
SEEDS = tuple(range(8))  # tests/test_gpu_frustum.py uses the same seeds and cameras


def pose(**kw):
    # powers of two: u = 512 X / Z + 320, v = 512 Y / Z + 240 are exact for the points below
    return fr.make_pose(np.eye(3), np.zeros(3), 512.0, 512.0, 320.0, 240.0, 40.0, **kw)


def one(P, Pn=(0, 0, 1), mf_min=0.5, mf_max=6.0, p=None, limit=0.5):
    r = fr.is_in_frustum(p or pose(), BOUNDS, [P], [Pn], [mf_min], [mf_max], limit)
    return {k: v[0] for k, v in r.items()}


def test_point_on_the_optical_axis():
    r = one((0, 0, 4))
    assert r["in_view"] == 1 and r["why"] == 0
    assert r["proj_x"] == F32(320) and r["proj_y"] == F32(240)
    assert r["proj_xr"] == F32(310)          # 320 - 40 * (1 / 4)
    assert r["depth"] == F32(4) and r["view_cos"] == F32(1)
    # mfMaxDistance / dist = 1.5: log(1.5) / log(1.2) = 2.22 -> level 3
    assert r["scale_level"] == 3
    # the ratio uses the MEMBER mfMaxDistance (MapPoint.cc:555): 4 / 4 = 1 -> log 0 -> level 0, inside the band 1.2 * 4
    assert one((0, 0, 4), mf_max=4.0)["scale_level"] == 0
    # far above the pyramid: clamped to n_levels - 1
    assert one((0, 0, 4), mf_max=400.0, mf_min=0.01)["in_view"] == 1
    assert one((0, 0, 4), mf_max=400.0, mf_min=0.01)["scale_level"] == 7


@pytest.mark.parametrize("P,u,v", [((-2.5, 0, 4), 0, 240), ((2.5, 0, 4), 640, 240), ((0, -1.875, 4), 320, 0),
                                   ((0, 1.875, 4), 320, 480)])
def test_points_exactly_on_the_image_bounds_are_in_view(P, u, v):
    n = np.asarray(P, np.float64) / np.linalg.norm(P)
    r = one(P, Pn=n)
    assert (r["proj_x"], r["proj_y"]) == (F32(u), F32(v))
    assert r["in_view"] == 1
    # a thousandth further out (an ulp of the point is below an ulp of u = 640): rejected at Frame.cc:679-682 with
    # mTrackProjX / Y still -1
    Q = np.asarray(P, F32)
    k = 0 if P[0] else 1
    Q[k] = Q[k] * F32(1.001)
    r = one(Q, Pn=n)
    assert r["in_view"] == 0 and r["why"] == fr.OUTSIDE_IMAGE and r["proj_x"] == F32(-1) and r["proj_y"] == F32(-1)


def test_distance_band_is_closed():
    # dist == GetMinDistanceInvariance() = 0.8f * mfMinDistance
    assert F32(0.8) * F32(5) == F32(4)
    r = one((0, 0, 4), mf_min=5.0, mf_max=20.0)
    assert r["in_view"] == 1
    r = one((0, 0, 4), mf_min=np.nextafter(F32(5), F32(6)), mf_max=20.0)
    assert r["in_view"] == 0 and r["why"] == fr.OUTSIDE_DISTANCE
    assert (r["proj_x"], r["proj_y"]) == (F32(320), F32(240))  # rejected after Frame.cc:684: u, v stay
    # dist == GetMaxDistanceInvariance() = 1.2f * mfMaxDistance
    z = F32(1.2) * F32(5)
    r = one((0, 0, z), mf_min=0.5, mf_max=5.0)
    assert r["in_view"] == 1 and r["scale_level"] == 0  # ratio 5 / 6 < 1: negative log, clamped to 0
    r = one((0, 0, np.nextafter(z, F32(7))), mf_min=0.5, mf_max=5.0)
    assert r["in_view"] == 0 and r["why"] == fr.OUTSIDE_DISTANCE


def test_view_cos_equal_to_the_limit_is_in_view():
    r = one((0, 0, 4), Pn=(0, np.sqrt(0.75), 0.5))
    assert r["view_cos"] == F32(0.5) and r["in_view"] == 1
    r = one((0, 0, 4), Pn=(0, np.sqrt(0.75), np.nextafter(F32(0.5), F32(0))))
    assert r["in_view"] == 0 and r["why"] == fr.VIEW_COS and r["proj_x"] == F32(320)
    r = one((0, 0, -4), Pn=(0, 0, -1))
    assert r["in_view"] == 0 and r["why"] == fr.BEHIND and r["proj_x"] == F32(-1)


def test_zero_depth_goes_on_to_the_comparisons():
    # PcZ == 0 is not < 0 (Frame.cc:674): u = 512 / 0 = +inf is outside the image
    r = one((1, 0, 0), Pn=(1, 0, 0))
    assert r["in_view"] == 0 and r["why"] == fr.OUTSIDE_IMAGE and r["proj_x"] == F32(-1)
    # the camera centre itself: u = v = 0 / 0 = NaN passes every comparison of :679-682; dist == 0, so viewCos = 0 / 0 passes
    # :701 too, and the ratio mfMax / 0 = inf has an infinite level whose x86 conversion is INT_MIN -> clamped to 0
    r = one((0, 0, 0), mf_min=0.0)
    assert r["in_view"] == 1 and np.isnan(r["proj_x"]) and np.isnan(r["proj_y"]) and np.isnan(r["view_cos"])
    assert r["depth"] == F32(0) and r["scale_level"] == 0


def test_zero_distance_to_the_camera_centre():
    # Ow is what the caller passes: a point at mOw but in front of the camera (dist == 0, PcZ == 4)
    p = pose(Ow=(0, 0, 4))
    r = one((0, 0, 4), mf_min=0.0, p=p)
    assert r["in_view"] == 1 and r["proj_x"] == F32(320) and np.isnan(r["view_cos"]) and r["scale_level"] == 0
    assert fr.predict_scale(F32(1), F32(0), fr.logf(1.2), 8) == 0
    assert fr.predict_scale(F32(0), F32(0), fr.logf(1.2), 8) == 0      # NaN ratio
    assert fr.cvt_int_x86(np.float32("nan")) == -2**31 and fr.cvt_int_x86(F32(3e9)) == -2**31
    assert fr.cvt_int_x86(F32(-2.7)) == -2


def test_skip_is_never_projected():
    pz, b, f = fr.scenario(0, "tum1", n=200)
    skip = (np.arange(200) % 5 == 0).astype(np.uint8)
    a = fr.is_in_frustum(pz, b, f["world_pos"], f["normal"], f["min_dist"], f["max_dist"])
    s = fr.is_in_frustum(pz, b, f["world_pos"], f["normal"], f["min_dist"], f["max_dist"], skip=skip)
    assert not s["in_view"][skip != 0].any() and (s["proj_x"][skip != 0] == -1).all()
    assert (s["in_view"][skip == 0] == a["in_view"][skip == 0]).all()


@pytest.mark.parametrize("camera", sorted(fr.CAMERAS))
def test_scenarios_meet_their_conditions(camera):
    """in view >= 10 %, each rejection >= 2 %, >= 6 predicted levels among the in-view points, for every scenario the GPU
    parity tests use; level 0 and level n_levels - 1 both occur in at least one of them."""
    seen = set()
    for seed in SEEDS:
        pz, b, f = fr.scenario(seed, camera)
        ref = fr.is_in_frustum(pz, b, f["world_pos"], f["normal"], f["min_dist"], f["max_dist"])
        shares, levels = fr.check_scenario(ref)
        print(camera, seed, {k: round(v, 3) for k, v in shares.items()}, levels)
        seen |= set(levels)
        iv = ref["in_view"] != 0
        for k in ("proj_x", "proj_y", "proj_xr", "depth", "view_cos"):
            assert np.isfinite(ref[k][iv]).all()
    assert 0 in seen and 7 in seen
