"""The exact integer algebra of k_pyramid's row loop against the reference's formula ([OCV] resize INTER_LINEAR 8U)

    v = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2

1. Horizontal pass: pixels in the high byte of a 16-bit half, weights times 16, so v_dot2_u32_u16 yields S << 12 and the
   truncated S >> 4 is the high half of the register as it lies.
2. Vertical pass: two 16-bit multiply-adds.  P0 = b0 * H0 + (2 << 16) with its low 16 bits cleared is a multiple of 2^16,
   so Q = b1 * H1 + P0 has Q >> 16 = (b0 * H0 >> 16) + (b1 * H1 >> 16) + 2 with each product truncated separately.
   (The same two truncated products as the high half of a 24-bit multiply -- ((b << 12) * (S & ~15)) >> 32 -- is
   checked too: it is the identity the multiply-add form was chosen over.)
3. Packing: two 10-bit sums in the halves of one dword, shifted together, bytes picked.
build_geometry refuses the fused kernel for tables outside the weight range these need."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

S_MAX = 255 * 2048
HC_DIR = Path(__file__).resolve().parent / "_hostcore"
U = np.uint64
M32 = U(0xFFFFFFFF)


def _s_values():
    def near(c):
        return [c + 16 * k + d for k in range(-4, 5) for d in (-1, 0, 1)]
    s = set(near(0)) | set(near(S_MAX)) | set(near(S_MAX // 2))
    for d in (-1, 0, 1):  # multiples of 16 on a coarse stride, and the values next to them
        s.update(range(16 * 61 + d, S_MAX + 1, 16 * 61))
    s.update(range(0, S_MAX + 1, 997))  # every residue mod 16 in between
    return np.array(sorted(v for v in s if 0 <= v <= S_MAX), dtype=np.uint64)


def mad_u32_u16(a, b, c):
    """v_mad_u32_u16: the low 16 bits of a and b multiplied, plus the 32-bit c, modulo 2^32."""
    return ((a & U(0xFFFF)) * (b & U(0xFFFF)) + c) & M32


def mul_hi_u32_u24(a, b):
    """v_mul_hi_u32_u24: bits [63:32] of the product of the operands' low 24 bits."""
    return ((a & U(0xFFFFFF)) * (b & U(0xFFFFFF))) >> U(32)


def test_s_values_cover_the_edges():
    S = _s_values()
    assert S.min() == 0 and S.max() == S_MAX and len(S) > 2000
    for c in (0, 16, 32, S_MAX & ~15, (S_MAX & ~15) - 16):
        for d in (-1, 0, 1):
            assert not (0 <= c + d <= S_MAX) or (c + d) in S


def test_truncated_product_every_weight():
    """One product: the multiply-add form with nothing added, and the 24-bit high-half form, against (b * (S >> 4)) >> 16."""
    S = _s_values()[None, :]
    b = np.arange(0, 2049, dtype=np.uint64)[:, None]
    want = (b * (S >> U(4))) >> U(16)
    H = ((S << U(12)) & M32) >> U(16)  # what op_sel reads of the horizontal sum
    assert np.array_equal(H, S >> U(4))
    assert np.array_equal(mad_u32_u16(b, H, U(0)) >> U(16), want)
    assert (2048 << 12) < (1 << 24) and (S_MAX & ~15) < (1 << 24)
    assert np.array_equal(mul_hi_u32_u24(b << U(12), S & ~U(15)), want)


def test_two_products_truncated_separately():
    """Every weight 0..2048 as b0 with b1 = 2048 - b0 and its two rounded neighbours, S0 over the whole set, S1 a
    permutation of it: Q >> 16 is the reference's sum, and it fits 10 bits (the result is a byte)."""
    S0 = _s_values()
    S1 = S0[::-1].copy()
    S1[::3] = S0[::3]  # equal rows too (flat content: the largest sums)
    H0, H1 = (S0 >> U(4))[None, :], (S1 >> U(4))[None, :]
    for db in (-1, 0, 1):
        b0 = np.arange(0, 2049, dtype=np.int64)
        b1 = np.clip(2048 - b0 + db, 0, 2048)
        b0, b1 = b0.astype(np.uint64)[:, None], b1.astype(np.uint64)[:, None]
        wy = b0 | (b1 << U(16))  # the table word: op_sel picks the half
        want = ((b0 * H0) >> U(16)) + ((b1 * H1) >> U(16)) + U(2)
        p = mad_u32_u16(wy, H0, U(2 << 16)) & U(0xFFFF0000)
        q = mad_u32_u16(wy >> U(16), H1, p)
        assert np.array_equal(q >> U(16), want)
        assert want.max() <= 1023


def test_horizontal_sum_times_4096():
    """(p0 << 8) * (16 a0) + (p1 << 8) * (16 a1) = S << 12 stays below 2^31 and its high half is S >> 4."""
    p = np.arange(256, dtype=np.uint64)
    for a0, a1 in ((2048, 0), (0, 2048), (1024, 1024), (1025, 1024), (1, 2047), (683, 1365), (2048, 1)):
        a0, a1 = U(a0), U(a1)
        S = p[:, None] * a0 + p[None, :] * a1
        d = (p[:, None] << U(8)) * (a0 << U(4)) + (p[None, :] << U(8)) * (a1 << U(4))
        assert d.max() < (1 << 31) and (a0 << U(4)) <= 0xFFFF and (a1 << U(4)) <= 0xFFFF
        assert np.array_equal(d >> U(16), S >> U(4))


def test_two_pixels_shifted_in_one_dword():
    """Two sums <= 1023 in the 16-bit halves of one dword, shifted right by 2 together: bytes 0 and 2 are the two pixels."""
    s = np.arange(0, 1024, dtype=np.uint64)
    lo, hi = np.meshgrid(s, s)
    t = (lo | (hi << U(16))) >> U(2)
    assert np.array_equal(t & U(0xFF), lo >> U(2)) and np.array_equal((t >> U(16)) & U(0xFF), hi >> U(2))


@pytest.fixture(scope="module")
def hc():
    subprocess.check_call(["make", "-C", str(HC_DIR)], stdout=subprocess.DEVNULL)
    L = C.CDLL(str(HC_DIR / "libvsg_hostcore.so"))
    L.hc_build.argtypes = [C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.hc_level.argtypes = [C.c_int, C.POINTER(C.c_int32)]
    L.hc_pyr_tiling.argtypes = [C.c_int, C.POINTER(C.c_int32)]
    L.hc_resize_tables.argtypes = [C.c_int, C.POINTER(C.c_int16), C.POINTER(C.c_int16)]
    return L


@pytest.mark.parametrize("kind", ["noise", "checker", "full"])
def test_row_arithmetic_on_the_builders_tables_equals_oracle_resize(hc, kind):
    """The row loop's operations, restated in numpy on the tables build_geometry makes, against the oracle's cv::resize
    restatement, level after level."""
    import oracle_lib as ol
    w, h, nl = 322, 241, 5
    assert hc.hc_build(500, 1.2, nl, 20, 7, h, w) == 0
    if kind == "noise":
        src = np.random.default_rng(5).integers(0, 256, (h, w), dtype=np.uint8)
    elif kind == "checker":
        y, x = np.mgrid[0:h, 0:w]
        src = (((x + y) & 1) * 255).astype(np.uint8)
    else:
        src = np.full((h, w), 255, np.uint8)
    for l in range(1, nl):
        info = np.zeros(16, np.int32)
        hc.hc_level(l, info.ctypes.data_as(C.POINTER(C.c_int32)))
        dw, dh = int(info[0]), int(info[1])
        xs, ys = np.zeros((dw, 4), np.int16), np.zeros((dh, 4), np.int16)
        hc.hc_resize_tables(l, xs.ctypes.data_as(C.POINTER(C.c_int16)), ys.ctypes.data_as(C.POINTER(C.c_int16)))
        P = src.astype(np.uint64)
        sx, a0, a1 = xs[:, 0].astype(np.int64), xs[:, 1].astype(np.uint64), xs[:, 2].astype(np.uint64)
        sx1 = np.minimum(sx + 1, P.shape[1] - 1)  # the kernel reads sx + 1 (its weight is 0 where the reference clamps)
        dot = (P[:, sx] << U(8)) * (a0 << U(4))[None, :] + (P[:, sx1] << U(8)) * (a1 << U(4))[None, :]
        assert dot.max() < (1 << 31)
        H = dot >> U(16)
        wy = ys[:, 2].astype(np.uint64) | (ys[:, 3].astype(np.uint64) << U(16))
        p = mad_u32_u16(wy[:, None], H[ys[:, 0]], U(2 << 16)) & U(0xFFFF0000)
        q = mad_u32_u16((wy >> U(16))[:, None], H[ys[:, 1]], p)
        out = (q >> U(18)).astype(np.uint8)
        assert (q >> U(18)).max() <= 255
        assert np.array_equal(out, ol.resize_linear(src, dw, dh)), l
        src = out


@pytest.mark.parametrize("w,h,nl,sf", [(640, 480, 8, 1.2), (1280, 720, 8, 1.2), (322, 241, 5, 1.2), (376, 240, 8, 1.2),
                                       (400, 300, 3, 2.0)])
def test_builder_tables_are_in_the_operand_range(hc, w, h, nl, sf):
    """Every weight build_geometry makes is in [0, 2048] (x pairs sum to <= 2049), so its range check leaves the fused
    tilings usable."""
    assert hc.hc_build(1000, sf, nl, 20, 7, h, w) == 0
    for l in range(1, nl):
        info = np.zeros(16, np.int32)
        hc.hc_level(l, info.ctypes.data_as(C.POINTER(C.c_int32)))
        xs, ys = np.zeros((info[0], 4), np.int16), np.zeros((info[1], 4), np.int16)
        hc.hc_resize_tables(l, xs.ctypes.data_as(C.POINTER(C.c_int16)), ys.ctypes.data_as(C.POINTER(C.c_int16)))
        assert 0 <= ys[:, 2:].min() and ys[:, 2:].max() <= 2048
        assert 0 <= xs[:, 1:3].min() and xs[:, 1:3].max() <= 2048 and (xs[:, 1].astype(int) + xs[:, 2]).max() <= 2049
    for i in range(3):
        out = np.zeros(6, np.int32)
        hc.hc_pyr_tiling(i, out.ctypes.data_as(C.POINTER(C.c_int32)))
        assert out[2] == 1, f"tiling {i} not usable"
