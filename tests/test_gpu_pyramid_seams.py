"""k_pyramid's stores at the seams between tiles: the row loop stores only column groups a tile owns whole, the seam pass
after each level's barrier stores the owned columns left over (csrc/vsg_geometry.h: pyr_seam), byte by byte out of the
level's LDS image.  Every level of every frame byte for byte against the oracle's ComputePyramid
(ORBextractor.cc:1171-1195), for the three fused tilings and the per-level kernel (-1), in batches of 1 and 3.

Geometries: the smallest ones (found by enumeration on the host, widths 100..400, height 3/4 of the width made odd, 4 and
5 levels) in which, for every fused tiling, every residue of ox0 % 4 and of ox1 % 4 occurs on an interior tile boundary of
some level, and in which no level's width is a multiple of 4 (the level's right edge is then a seam too).
test_geometries_show_every_residue keeps that set honest.  Plus 322x241 / 5 levels, the odd-sized geometry of
test_gpu_pyramid_rows.py: it shows every residue too, but its levels 1 and 2 are 268 and 224 wide.

Contents: noise; all 255; and two different noise frames run back to back through the same extractor -- a seam byte that
is not stored keeps the previous frame's value."""
import functools

import numpy as np
import pytest

import oracle_lib as ol
import pyramid_seam_hostcore as ps
from visual_sgraphs_amd import orb

SMALLEST = {4: (157, 117), 5: (189, 141)}  # levels -> (w, h)
ENUMERATED = [(157, 117, 4, 1.2), (189, 141, 5, 1.2)]
GEOMS = ENUMERATED + [(322, 241, 5, 1.2)]
EVERY_RESIDUE = {(ti, side, r) for ti in ps.TILINGS for side in (0, 1) for r in range(4)}


def candidate_height(w):
    return ((3 * w) // 4) | 1


def boundary_residues(G):
    """{(tiling, side, residue)} over the interior boundaries of every level >= 1: side 0 = ox0 % 4 of a tile that does
    not start the level, side 1 = ox1 % 4 of a tile that does not end it."""
    found = set()
    for ti in ps.TILINGS:
        for recs in G.tilings[ti]["records"]:
            for l in range(1, G.nl):
                ox0, _, ox1, _ = recs[l]["own"]
                if ox0 > 0:
                    found.add((ti, 0, ox0 % 4))
                if ox1 < G.levels[l][0]:
                    found.add((ti, 1, ox1 % 4))
    return found


def usable(G):
    return G.rc == 0 and all(P["ok"] for P in G.tilings.values()) and all(lv[0] % 4 != 0 for lv in G.levels)


def test_geometries_show_every_residue():
    for w, h, nl, sf in GEOMS:
        G = ps.geometry(w, h, nl, sf)
        if (w, h, nl, sf) in ENUMERATED:
            assert usable(G), f"{w}x{h}/{nl}: a level width is a multiple of 4, or a tiling is not usable"
        assert boundary_residues(G) == EVERY_RESIDUE, f"{w}x{h}/{nl}: residues missing {EVERY_RESIDUE - boundary_residues(G)}"
        assert w <= 400
    # the first two are the smallest of their family: no narrower candidate shows every residue
    for nl, (w_min, h_min) in SMALLEST.items():
        assert h_min == candidate_height(w_min) and (w_min, h_min, nl, 1.2) in ENUMERATED
        for w in range(100, w_min):
            G = ps.Geometry(w, candidate_height(w), nl, 1.2)
            assert not (usable(G) and boundary_residues(G) == EVERY_RESIDUE), f"{w} wide / {nl} levels is smaller"


def content(kind, w, h):
    if kind == "full":
        return np.full((h, w), 255, np.uint8)
    seed = {"noise": 1, "noise_b": 2}[kind]
    return np.random.default_rng(seed * 100000 + w * 1000 + h).integers(0, 256, (h, w), dtype=np.uint8)


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
    # the same extractor (the same pyramid buffer) throughout: noise, then other noise in the same place, then 255
    batches = [("noise",), ("noise_b",), ("full",), ("noise", "noise_b", "full"), ("noise_b", "full", "noise")]
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
