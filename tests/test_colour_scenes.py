"""The reference side of tests/test_gpu_colour.py, checked where the oracle runs and no GPU is needed: the definition of
the gray conversion (colour_scenes.gray_reference) against the oracle's conversion and the OpenCV 4.2 fixture, and the
conditions on the directed scenes that keep the GPU comparison from being vacuous."""
from pathlib import Path

import numpy as np
import pytest

import colour_scenes as cs
import oracle_lib as ol

PIN = Path(__file__).parent / "golden" / "opencv42_v1.npz"
TABLES = [(cs.DEFAULT_COEFFS, cs.DEFAULT_SHIFT)] + cs.ALT_TABLES
GEOMETRIES = [(w, cs.rows_for(w), cs.NFEATURES, cs.NLEVELS) for w in cs.WIDTHS + cs.INGEST_WIDTHS[2:]] + [cs.MULTI_LEVEL] + cs.INTERLEAVE


def _scenes():
    """every kind of scene at widths of every position class, both channel counts"""
    for w, h in ((131, cs.H), (1027, cs.rows_for(1027)), (2051, cs.rows_for(2051)), cs.MULTI_LEVEL[:2]):
        for ch in (3, 4):
            yield f"palette {w}x{h}x{ch}", cs.palette(w, h, ch, w + ch)
            yield f"textured {w}x{h}x{ch}", cs.textured(w, h, ch, w + ch)


@pytest.mark.parametrize("coeffs,shift", TABLES, ids=[f"{c[0]}_{c[1]}_{c[2]}_s{s}" for c, s in TABLES])
def test_definition_equals_the_oracle_conversion(coeffs, shift):
    assert sum(coeffs) == 1 << shift and min(coeffs) >= 0 and 255 * sum(coeffs) + (1 << (shift - 1)) < 2 ** 31
    for name, col in _scenes():
        for rgb in (True, False):
            want = ol.cvt_gray(col, rgb, coeffs, shift)
            assert np.array_equal(cs.gray_reference(col, rgb, coeffs, shift), want), (name, rgb)


@pytest.mark.skipif(not PIN.exists(), reason="tests/golden/opencv42_v1.npz absent: run tools/pin_with_opencv (needs "
                    "OpenCV 4.2 + the reference checkout), as for tests/test_pin_opencv42.py")
def test_definition_equals_opencv_42():
    """the 4096 seeded colours tools/pin_with_opencv converts with a real cv::cvtColor (the fixture of
    tests/test_pin_opencv42.py; like every test there it can only run once that fixture has been produced)"""
    P = np.load(PIN)
    rgb = P["gray/rgb"]
    assert np.array_equal(cs.gray_reference(rgb, True), P["gray/rgb2gray"].ravel())
    assert np.array_equal(cs.gray_reference(rgb, False), P["gray/bgr2gray"].ravel())


def test_single_channel_tables_select_that_channel():
    col = cs.palette(131, cs.H, 4, 5)
    for rgb in (True, False):
        assert np.array_equal(cs.gray_reference(col, rgb, (16384, 0, 0), 14), col[..., 0 if rgb else 2])
        assert np.array_equal(cs.gray_reference(col, rgb, (0, 0, 16384), 14), col[..., 2 if rgb else 0])


@pytest.mark.parametrize("w", cs.WIDTHS + [cs.MULTI_LEVEL[0]])
@pytest.mark.parametrize("channels", [3, 4])
def test_palette_puts_every_directed_pixel_on_every_column(w, channels):
    h = cs.MULTI_LEVEL[1] if w == cs.MULTI_LEVEL[0] else cs.rows_for(w)
    img = cs.palette(w, h, channels, 3)
    assert img.shape == (h, w, channels) and img.dtype == np.uint8
    cr, cg, cb = cs.DEFAULT_COEFFS
    columns = sorted({0, w - 1, *range(w - max(w % 4, 1), w), *(x for x in (1023, 1024, 2047, 2048) if x < w)})
    for rgb in (True, False):
        px = img[..., :3].astype(np.int64) if rgb else img[..., 2::-1].astype(np.int64)
        frac = (px[..., 0] * cr + px[..., 1] * cg + px[..., 2] * cb) % (1 << cs.DEFAULT_SHIFT)
        for x in columns:
            col = [tuple(p) for p in px[:, x].tolist()]
            assert (frac[:, x] == 8192).any() and (frac[:, x] == 8191).any(), (x, rgb)  # both sides of the boundary
            for e in cs.EXTREMES:
                assert e in col, (x, rgb, e)
        # the two sides really round differently
        up, down = frac == 8192, frac == 8191
        g = cs.gray_reference(img, rgb).astype(np.int64)
        s = px[..., 0] * cr + px[..., 1] * cg + px[..., 2] * cb
        assert np.array_equal(g[up], (s[up] >> 14) + 1) and np.array_equal(g[down], s[down] >> 14)
    band = img[len(cs.directed_pixels()):]
    assert len(band) >= 20
    for c in range(channels):  # independent uniform channels: every byte value occurs, no channel copies another
        assert len(np.unique(band[..., c])) == 256
        for c2 in range(c):
            assert np.mean(band[..., c] == band[..., c2]) < 0.02
    if channels == 4:
        assert len(np.unique(img[..., 3])) == 256


@pytest.mark.parametrize("w,h,nf,nl", GEOMETRIES, ids=[f"{g[0]}x{g[1]}" for g in GEOMETRIES])
def test_textured_frames_tell_the_channels_apart_and_hold_keypoints(w, h, nf, nl):
    """Every textured frame the GPU tests extract from (seeds SEED .. SEED + 7 at every geometry of the lists): swapped or
    dropped channels move the gray level, the frames differ pairwise, and the oracle finds at least 20 keypoints."""
    frames = [cs.textured(w, h, 4, cs.SEED + f) for f in range(8)]
    ref = ol.OracleExtractor(nf, cs.EXTRACTOR[0], nl, *cs.EXTRACTOR[1:])
    for col in frames:
        for rgb in (True, False):
            g = cs.gray_reference(col, rgb)
            swapped = cs.gray_reference(col, not rgb)  # reading R as B
            moved = np.abs(g.astype(np.int32) - swapped.astype(np.int32)) >= 8
            assert moved.mean() >= 0.25, (rgb, moved.mean())
            # a dropped channel shows as well
            for drop in range(3):
                d = col.copy()
                d[..., drop] = 0
                assert (np.abs(g.astype(np.int32) - cs.gray_reference(d, rgb).astype(np.int32)) >= 8).mean() >= 0.25
            assert len(ref(g)[1]) >= 20, (rgb, len(ref(g)[1]))
    for rgb in (True, False):  # the frames of one batch differ pairwise
        grays = [cs.gray_reference(c, rgb) for c in frames]
        for i in range(8):
            for j in range(i):
                assert (grays[i] != grays[j]).mean() > 0.25, (i, j)


def test_textured_colour_bytes_do_not_depend_on_the_channel_count():
    a, b = cs.textured(131, cs.H, 3, 9), cs.textured(131, cs.H, 4, 9)
    assert np.array_equal(a, b[..., :3])
    assert len(np.unique(b[..., 3])) > 200
