"""Directed colour frames and the definition of the gray conversion for the colour entry points
(vsg_orb_extract_batch_color / vsg_orb_extract_batch_device_color, k_cvt_gray).  Plain NumPy, no GPU.

`gray_reference` is cv::cvtColor(COLOR_{RGB,BGR,RGBA,BGRA}2GRAY) for 8-bit images written out as its definition in int64,
independently of oracle_lib.cvt_gray (tests/test_colour_scenes.py compares the two, and both with the OpenCV 4.2 fixture).

k_cvt_gray converts 4 pixels per thread and 1024 pixels per block; a width that is no multiple of 4 ends in a partial
group whose 32-bit store reaches into the row pad.  The position classes of a column are therefore: column 0, the last
column, the last `cols % 4` columns and the columns on both sides of every 1024-pixel block edge.  `palette` puts every
directed pixel on every column, `textured` gives the extractor something to find."""
import numpy as np

from visual_sgraphs_amd import synth

DEFAULT_COEFFS = (4899, 9617, 1868)  # OpenCV 4.2 R2Y, G2Y, B2Y
DEFAULT_SHIFT = 14

# The tables vsg_orb_set_gray_coeffs is tested with: one channel alone, OpenCV's 15-bit table, the smallest shift, and a
# table at shift 20, where 255 << 20 plus the rounding half is the largest sum the kernel's int32 still holds.
ALT_TABLES = [((16384, 0, 0), 14), ((0, 0, 16384), 14), ((9798, 19235, 3735), 15), ((1, 1, 0), 1),
              ((313524, 615514, 119538), 20)]

# (R, G, B) whose weighted sum with the default table lies exactly on the rounding boundary of (sum + 8192) >> 14:
# sum % 16384 == 8192 rounds up, 8191 rounds down
BOUNDARY_UP = [(0, 56, 102), (194, 78, 129), (130, 186, 232), (242, 246, 103), (35, 91, 137), (9, 185, 37)]
BOUNDARY_DOWN = [(0, 47, 8), (194, 69, 35), (129, 56, 211), (245, 180, 49), (35, 254, 210), (9, 56, 17)]
EXTREMES = [(0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255)]

# Geometries of the GPU tests: one level (every level needs width and height >= 67), 80 rows where the width allows it
H = 80


def rows_for(w):
    """The height the frames of width w get: 80 rows, or the smallest multiple of 8 above that at which the level has at
    most 16 initial octree nodes -- round((w - 32) / (h - 32)) of them (ORBextractor.cc:566), and build_geometry
    (vsg_geometry.h) refuses more than kMaxIniNodes = 16, so 80 rows stop at a width of about 820."""
    h = H
    while round((w - 32) / (h - 32)) > 16:
        h += 8
    return h


NLEVELS = 1
NFEATURES = 300
WIDTHS_PARTIAL_GROUP = [128, 129, 130, 131]          # cols % 4 = 0, 1, 2, 3
WIDTHS_BLOCK_EDGE = [1021, 1024, 1025, 1027, 1028]   # around blockIdx.x = 0 | 1
WIDTHS_THIRD_BLOCK = [2051]
WIDTHS = WIDTHS_PARTIAL_GROUP + WIDTHS_BLOCK_EDGE + WIDTHS_THIRD_BLOCK
MULTI_LEVEL = (322, 240, 600, 8)                     # w, h, nfeatures, nlevels: the one 8-level case
EXTRACTOR = (1.2, 20, 7)                             # scaleFactor, iniThFAST, minThFAST of every case
INTERLEAVE = [(163, 121, 400, 3), (262, 191, 400, 3)]  # the two geometries of the one-handle interleaving test
INGEST_WIDTHS = [128, 129, 143]                      # k_ingest moves 16 bytes per thread: cols % 16 = 0, 1, 15
SEED = 100                                           # frame f of a textured batch is textured(..., SEED + f), f < 8


def gray_reference(col, rgb_order, coeffs=DEFAULT_COEFFS, shift=DEFAULT_SHIFT):
    """[..., 3 | 4] uint8 -> [...] uint8: ((R*cr + G*cg + B*cb + (1 << (shift-1))) >> shift) in int64; R is byte 0 of a
    pixel when rgb_order, byte 2 otherwise; a fourth byte is ignored."""
    col = np.asarray(col)
    assert col.dtype == np.uint8 and col.shape[-1] in (3, 4)
    c = col.astype(np.int64)
    r, g, b = (c[..., 0], c[..., 1], c[..., 2]) if rgb_order else (c[..., 2], c[..., 1], c[..., 0])
    cr, cg, cb = (int(v) for v in coeffs)
    return ((r * cr + g * cg + b * cb + (1 << (int(shift) - 1))) >> int(shift)).astype(np.uint8)


def directed_pixels():
    """The directed (byte0, byte1, byte2) triples of `palette`: the extremes and the rounding-boundary colours, the latter
    in both byte orders so that RGB and BGR readers both meet them as (R, G, B)."""
    both = BOUNDARY_UP + BOUNDARY_DOWN
    return np.array(EXTREMES + both + [t[::-1] for t in both], np.uint8)


def palette(w, h, channels, seed):
    """Directed frame: rows 0 .. n-1 (n = the number of directed pixels, at most h / 2) hold directed pixel (x + y) % n at
    column x, so every column -- column 0, the last one, the partial last group, both sides of every block edge -- meets
    every directed pixel; the rows below are a band of independent uniform channels.  Alpha is independent and uniform."""
    assert channels in (3, 4)
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, channels), dtype=np.uint8)
    d = directed_pixels()
    n = min(len(d), h // 2)
    yy, xx = np.mgrid[0:n, 0:w]
    img[:n, :, :3] = d[(xx + yy + seed) % len(d)]
    return img


def textured(w, h, channels, seed):
    """synth.frame with a gain and an offset of its own per channel: R = base, G = 40 + 3 * base / 4, B = base / 2 + noise.
    R and B differ by half the base level, so a reader that swaps them, or drops a channel, moves the gray level by tens of
    levels; the seed selects the scene, so the frames of a batch differ.  The colour bytes do not depend on `channels`;
    alpha is independent and uniform.  The base is every second pixel of a frame of twice the size: rectangles of half
    the size, so that the 96 x 48 pixels an 128 x 80 frame leaves to FAST still hold a few dozen corners."""
    assert channels in (3, 4)
    rng = np.random.default_rng(seed)
    base = synth.frame(2 * w, 2 * h, seed)[::2, ::2].astype(np.int32)
    img = np.empty((h, w, channels), np.uint8)
    img[..., 0] = base
    img[..., 1] = 40 + 3 * base // 4
    img[..., 2] = base // 2 + rng.integers(0, 16, base.shape)
    if channels == 4:
        img[..., 3] = rng.integers(0, 256, base.shape)
    return img
