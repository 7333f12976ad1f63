"""What k_pyramid stores to a level, modelled on the host from the same tile records and the same seam helper
(csrc/vsg_geometry.h: PyrTileLevel, pyr_seam, pyr_seam_column): a lane of the row loop stores the whole dword of a column
group that is fully owned (rows limited to the owned ones by the buffer descriptor), and the seam pass stores the owned
columns that lie in no such group, byte by byte, out of the level's LDS image.  Over all tiles of a tiling these writes must
cover every byte of every level >= 1 exactly once and nothing else.

Also here: the LDS footprint of every tiling is the one the kernel had before the seam pass existed (the reference
configuration sits 660 bytes under the four-workgroups-per-CU edge), and the per-(tile, level) thread split carried in the
records equals the formulas the kernel used to evaluate per level."""
import numpy as np
import pytest

import pyramid_seam_hostcore as ps

GEOMS = [(640, 480, 8, 1.2), (752, 480, 8, 1.2), (1280, 720, 8, 1.2), (322, 241, 5, 1.2), (376, 240, 8, 1.2),
         (400, 300, 3, 2.0)]
# PyrTiling::lds_bytes() per tiling 0 / 1 / 2, read from a build of the commit before the seam pass
LDS_BEFORE = {
    (640, 480, 8, 1.2): (29528, 40336, 11688),
    (752, 480, 8, 1.2): (28624, 38616, 11368),
    (1280, 720, 8, 1.2): (30920, 41776, 12368),
    (322, 241, 5, 1.2): (10856, 10856, 4024),
    (376, 240, 8, 1.2): (21592, 36616, 9664),
    (400, 300, 3, 2.0): (13816, 18432, 5288),
}


@pytest.mark.parametrize("ti", ps.TILINGS)
@pytest.mark.parametrize("w,h,nl,sf", GEOMS)
def test_every_level_byte_written_exactly_once(w, h, nl, sf, ti):
    G = ps.geometry(w, h, nl, sf)
    assert G.rc == 0
    P = G.tilings[ti]
    assert P["ntiles"] > 0
    for l in range(1, nl):
        lw, lh, _, _ = G.levels[l]
        count = np.zeros((lh, lw), np.int32)

        def mark(x0, x1, y0, y1, what):
            assert 0 <= x0 <= x1 <= lw and 0 <= y0 <= y1 <= lh, f"level {l} {what}: [{x0},{x1}) x [{y0},{y1}) leaves {lw} x {lh}"
            count[y0:y1, x0:x1] += 1

        for t, recs in enumerate(P["records"]):
            R = recs[l]
            dx0, dy0, dx1, dy1 = R["need"]
            ox0, oy0, ox1, oy1 = R["own"]
            dx0a = dx0 & ~3
            (a0, a1, nl_, n), cols = ps.seam(ox0, ox1)
            assert n <= 6 and len(cols) == n == len(set(cols)), f"tile {t} level {l}: seam columns {cols}"
            # rows: the row loop produces the needed rows, the descriptor lets the owned ones through; the seam pass reads
            # the owned rows out of the LDS image, which holds the needed ones
            assert dy0 <= oy0 and oy1 <= dy1 and dx0 <= ox0 and ox1 <= dx1, f"tile {t} level {l}: owned part outside the LDS image"
            ry0, ry1 = max(dy0, oy0), min(dy1, oy1)
            for cg in range(R["ncg"]):
                gx = dx0a + 4 * cg
                if a0 <= gx < a1:
                    assert ox0 <= gx and gx + 4 <= ox1
                    mark(gx, gx + 4, ry0, ry1, f"tile {t} group {cg}")
            for x in cols:
                assert ox0 <= x < ox1 and dx0a <= x < dx0a + 4 * R["ncg"], f"tile {t} level {l}: seam column {x}"
                mark(x, x + 1, oy0, oy1, f"tile {t} seam column {x}")
        bad = np.argwhere(count != 1)
        assert len(bad) == 0, (f"tiling {ti} level {l}: {len(bad)} bytes not written exactly once, first (y, x) = "
                               f"{tuple(bad[0])} written {count[tuple(bad[0])]} times")


def test_seam_helper_on_every_small_range():
    """pyr_seam on every owned range up to 40 columns: the groups [a0, a1) are the aligned groups inside the range, the
    seam columns are the rest, at most 3 on each side."""
    for ox0 in range(0, 12):
        for ox1 in range(ox0, ox0 + 41):
            (a0, a1, nl_, n), cols = ps.seam(ox0, ox1)
            full = [g for g in range(0, ox1 + 4, 4) if ox0 <= g and g + 4 <= ox1]
            assert [g for g in range(0, ox1 + 4, 4) if a0 <= g < a1] == full
            covered = {x for g in full for x in range(g, g + 4)}
            assert sorted(cols) == [x for x in range(ox0, ox1) if x not in covered]
            assert nl_ <= 3 and n - nl_ <= 3 and n <= 6


@pytest.mark.parametrize("w,h,nl,sf", GEOMS)
def test_lds_footprint_is_unchanged(w, h, nl, sf):
    G = ps.geometry(w, h, nl, sf)
    assert tuple(G.tilings[ti]["lds"] for ti in ps.TILINGS) == LDS_BEFORE[(w, h, nl, sf)]


@pytest.mark.parametrize("w,h,nl,sf", GEOMS)
def test_thread_split_in_the_records_is_the_kernels_formula(w, h, nl, sf):
    G = ps.geometry(w, h, nl, sf)
    for ti in ps.TILINGS:
        P = G.tilings[ti]
        assert P["ok"] and P["rec_bytes"] == 32  # one 8-dword scalar load
        threads = P["threads"]
        for recs in P["records"]:
            tab = 0
            for l in range(1, nl):
                R = recs[l]
                dx0, dy0, dx1, dy1 = R["need"]
                dpitch = ((dx1 - (dx0 & ~3)) + 3) & ~3
                ncg = dpitch >> 2
                assert R["ncg"] == ncg
                nrg = threads // ncg
                assert R["nrg"] == nrg and R["chunk"] == (dy1 - dy0 + nrg - 1) // nrg
                assert R["tab"] == tab
                tab += (dx1 - dx0) + (dy1 - dy0)
                assert (R["pitch"], R["img_off"]) == G.levels[l][2:4]
