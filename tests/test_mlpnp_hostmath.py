"""The elementary functions csrc/vsg_mlpnp.h writes out, and the host-only set-up of the solver, without a device.

acos and the cube root have no rounding that IEEE 754 defines, so the header states them in a fixed number of steps (the fdlibm
rational form of acos; a bit-level start and five Newton steps for the cube root) and both sides run those.  Against NumPy over a
dense sweep and the edges.  MEASURED: acos at most 1 ulp from numpy.arccos over 200001 points of [-1, 1] and the edges; the cube
root at most 1 ulp from numpy.cbrt over 200001 points of [1e-320, 1e308] and the edges.  The bound asserted is the doubled
figure, 2 ulp each.  Out of range and NaN agree exactly (NaN), +-1 and 0 exactly.
vsg_mlpnp_ransac_parameters and vsg_mlpnp_draw_sets run against the restatement (tests/mlpnp_reference.py)."""
import ctypes as C

import numpy as np
import pytest

import mlpnp_hostcore as hc
import mlpnp_reference as mr
from visual_sgraphs_amd import orb

ULP_ACOS, ULP_CBRT = 2.0, 2.0
I32 = np.int32


def ulps(got, want):
    return np.abs(got - want) / np.spacing(np.abs(want))


def test_acos_against_numpy():
    x = np.concatenate([np.linspace(-1, 1, 200001), np.nextafter(1.0, 0) * np.array([1, -1]), [0.5, -0.5, np.nextafter(0.5, 1), 2.0 ** -57,
                        2.0 ** -58, 5e-324, -5e-324, 1e-300, 0.0, -0.0]])
    want, got = np.arccos(x), hc.acos(x)
    u = ulps(got, want)
    print("\nacos: max %.2f ulp" % u.max())
    assert u.max() <= ULP_ACOS
    assert hc.acos([1.0])[0] == 0.0 and hc.acos([-1.0])[0] == np.pi and hc.acos([0.0])[0] == np.pi / 2
    beyond = hc.acos([np.nextafter(1.0, 2), -np.nextafter(1.0, 2), 1.5, -3.0, 1e300, np.inf, -np.inf, np.nan])
    assert np.isnan(beyond).all()


def test_cube_root_against_numpy():
    x = np.concatenate([np.logspace(-320, 308, 200001), [5e-324, 1e-310, 2.2250738585072014e-308, 1.0, 8.0, 27.0, 1e-3, 1.7976931348623157e308,
                        0.3, 3.0, 1e15]])
    want, got = np.cbrt(x), hc.cbrt(x)
    u = ulps(got, want)
    print("\ncbrt: max %.2f ulp" % u.max())
    assert u.max() <= ULP_CBRT
    assert hc.cbrt([0.0])[0] == 0.0 and hc.cbrt([np.inf])[0] == np.inf and hc.cbrt([8.0])[0] == 2.0 and hc.cbrt([27.0])[0] == 3.0
    assert np.isnan(hc.cbrt([np.nan, -1.0])).all()  # the solver takes it of an absolute value


@pytest.mark.parametrize("n", (0, 1, 5, 6, 7, 10, 19, 20, 21, 30, 100, 300, 1000, 5000))
def test_ransac_parameters(n):
    for args in ((0.99, 10, 300, 6, 0.5), (0.99, 15, 300, 6, 0.5), (0.999, 10, 50, 6, 0.3), (0.5, 6, 300, 6, 0.9), (0.99, 10, 300, 6, 1.0)):
        want = mr.ransac_parameters(*args, n)
        assert hc.parameters(*args, n) == want, (args, n)
        if n > 0:
            assert orb.mlpnp_ransac_parameters(n, *args) == want, (args, n)
    # pow(epsilon, 3) although the minimal set is 6: n = 100 gives 35 iterations, the sixth power would give 293
    assert hc.parameters(0.99, 10, 300, 6, 0.5, 100) == (50, 35)
    L = orb.load_library()
    o = np.full(2, -9, I32)
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    assert L.vsg_mlpnp_ransac_parameters(0.99, 10, 300, 6, 0.5, -1, p(o[:1]), p(o[1:])) == -6 and (o == -9).all()
    assert L.vsg_mlpnp_ransac_parameters(0.99, 10, 300, 6, 0.5, 10, None, p(o[1:])) == -6 and (o == -9).all()


def test_draw_sets():
    state = [12345]

    def lcg(lo, hi):
        state[0] = (state[0] * 1103515245 + 12345) & 0x7fffffff
        return lo + state[0] % (hi - lo + 1)
    for n in (6, 7, 30, 300):
        state[0] = 12345
        got = orb.mlpnp_draw_sets(n, 40, lcg)
        state[0] = 12345
        want = mr.draw_sets(n, 40, lcg)
        assert np.array_equal(got, want)
        assert all(len(set(r)) == 6 and min(r) >= 0 and max(r) < n for r in got)
    assert sorted(orb.mlpnp_draw_sets(6, 1, lcg)[0]) == [0, 1, 2, 3, 4, 5]
    assert len(orb.mlpnp_draw_sets(30, 0)) == 0 and orb.mlpnp_draw_sets(30, 5).shape == (5, 6)  # rand()'s formula
    L = orb.load_library()
    out = np.full(12, -9, I32)
    p = out.ctypes.data_as(C.POINTER(C.c_int32))
    assert L.vsg_mlpnp_draw_sets(5, 2, orb._RANDOM_INT(), None, p) == -6 and (out == -9).all()  # n below the minimal set
    assert L.vsg_mlpnp_draw_sets(30, -1, orb._RANDOM_INT(), None, p) == -6 and L.vsg_mlpnp_draw_sets(30, 2, orb._RANDOM_INT(), None, None) == -6
    bad = orb._RANDOM_INT(lambda lo, hi, _ctx: hi + 1)
    assert L.vsg_mlpnp_draw_sets(30, 2, bad, None, p) == -6
