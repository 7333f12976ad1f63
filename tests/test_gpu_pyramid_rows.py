"""k_pyramid's row loop (horizontal sums read as high halves, the vertical pass as two 16-bit multiply-adds, stores through
the owned rows' buffer descriptor, running LDS / HBM offsets) at the smallest shapes where it can go wrong, on contents
chosen for its arithmetic: every level of every frame byte for byte against the oracle's ComputePyramid
(ORBextractor.cc:1171-1195), for the three fused tilings and the automatic choice, in batches of 1 and 3.

 * 320x240, 4 levels: the plain case.
 * 322x241, 5 levels: level widths that are no multiple of 4 and odd heights -- partial seam dwords, chunks that end on
   the first row of a pair.
 * 376x240, 8 levels: a top level just over 64 rows (67).
 * 400x300, 3 levels, scale factor 2.0: the widest source window (6 bytes over 3 columns) and every weight 1024.
Contents: all 0, all 255 (the largest products and sums), a 1-pixel 0 / 255 checkerboard (every truncation carries), uniform
noise, a vertical ramp (every row pair differs, every column equal)."""
import functools

import numpy as np
import pytest

import oracle_lib as ol
from visual_sgraphs_amd import orb

GEOMS = [(320, 240, 4, 1.2), (322, 241, 5, 1.2), (376, 240, 8, 1.2), (400, 300, 3, 2.0)]
CONTENTS = ("zeros", "full", "checker", "noise", "ramp")


def content(kind, w, h):
    if kind == "zeros":
        return np.zeros((h, w), np.uint8)
    if kind == "full":
        return np.full((h, w), 255, np.uint8)
    if kind == "checker":
        y, x = np.mgrid[0:h, 0:w]
        return (((x + y) & 1) * 255).astype(np.uint8)
    if kind == "noise":
        return np.random.default_rng(w * 1000 + h).integers(0, 256, (h, w), dtype=np.uint8)
    if kind == "ramp":
        return np.repeat(((np.arange(h) * 255) // (h - 1)).astype(np.uint8)[:, None], w, axis=1)
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def oracle_levels(kind, w, h, nl, sf):
    """The oracle's pyramid of one content at one geometry: computed once, shared by every tiling, read only."""
    ref = ol.OracleExtractor(500, sf, nl, 20, 7)
    ref(content(kind, w, h))
    levels = tuple(ref.pyramid_level(l) for l in range(nl))
    for a in levels:
        a.setflags(write=False)
    return levels


@pytest.mark.gpu
@pytest.mark.parametrize("which", [0, 1, 2, -1])
@pytest.mark.parametrize("w,h,nl,sf", GEOMS)
def test_every_level_byte_for_byte(w, h, nl, sf, which):
    ex = orb.ORBextractor(500, sf, nl, 20, 7, max_batch=3)
    ex.set_pyramid_tiling(which)
    batches = [("zeros", "full", "checker"), ("noise", "ramp", "checker"), ("noise",), ("checker",), ("full",)]
    for kinds in batches:
        ex.extract_batch(np.stack([content(k, w, h) for k in kinds]))
        for f, kind in enumerate(kinds):
            want = oracle_levels(kind, w, h, nl, sf)
            for l in range(nl):
                got = ex.image_pyramid(l, frame=f)
                assert got.shape == want[l].shape
                bad = np.argwhere(got != want[l])
                assert len(bad) == 0, (f"tiling {which} batch {kinds} frame {f} ({kind}) level {l}: {len(bad)} bytes differ, "
                                       f"first at (y, x) = {tuple(bad[0])}: {got[tuple(bad[0])]} != {want[l][tuple(bad[0])]}")
