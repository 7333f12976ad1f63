"""k_fast_cells' two launch forms: the one compiled without the paths a geometry rules out (template switches kSeg and
kPlain of visual_sgraphs_amd/csrc/vsg_kernels.hip) and the general one, each against the CPU oracle bit for bit and each
proven taken through the launch-forms record (vsg_launch_forms.fast_specialised, include/vsg_orb_debug.h).

launch_fast takes the specialised form when the geometry has segmented candidate lists (no level of more than 4096 cells)
and is `plain` (Geometry::fastPlain, vsg_geometry.h fast_cells_plain): no live cell is a sliver (a tile row of fewer than 4
dwords) and every live cell's tile fits the prefetch registers of its tile class.  vsg_orb_set_fast_form(h, 0) forces the
general form on any handle.

The host part (tests/_fast_forms/fast_forms_host.cpp: the product's geometry code compiled for the CPU) needs no GPU: the
predicate against a restatement from the cell rectangles, and the search for the geometries the GPU cases run on.

Where slivers and oversized tiles can exist, with the reference's 35 px cell grid (ORBextractor.cc:795-809):
  * the last cell of a row has vw = width - (nCols - 1) * wCell - 6 > wCell - nCols - 6 columns (width = level width - 32,
    nCols = floor(width / 35), wCell = ceil(width / nCols) >= 35); a sliver needs ox + vw <= 6, so nCols >= 24 and a level
    more than 870 px wide.  No image of 200 x 160 or below has one; the smallest width with one is found below by
    evaluating the host geometry over widths (908 px), with the smallest height the geometry accepts for it.
  * a tile has nq4 * (vh + 6) chunks with vh <= 69 (one row of cells on a level 35..69 px high) and nq4 = chunks per tile row
    <= 4 / 4 / 5 in the 52 / 68 / 84-byte classes (a cell as wide as the class allows starts at a multiple of its width from
    column 16, so its tile has no alignment bytes): at most 300 / 300 / 375 chunks against 256 / 384 / 512 registers' worth --
    and 4 chunks per row in the 52-byte class would need a 40 px cell three bytes off alignment, which a 40 px grid never
    gives.  test_no_small_geometry_has_a_tile_beyond_the_prefetch_registers sweeps every level size up to 320 x 240 at the
    heights with the tallest cells: none exists, so that half of kPlain = false is covered by the forced general form."""
import ctypes as C
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

import oracle_lib as ol
from visual_sgraphs_amd import orb, synth

HERE = Path(__file__).resolve().parent
_i32p = C.POINTER(C.c_int32)
PREFETCH_CHUNKS = {52: 128 * 2, 68: 128 * 3, 84: 128 * 4}  # 128 threads x kPre 16-byte chunks (launch_fast)


@pytest.fixture(scope="module")
def ff(tmp_path_factory):
    so = tmp_path_factory.mktemp("fast_forms") / "libfast_forms_host.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-mfma",
                           "-I", str(HERE.parent / "visual_sgraphs_amd" / "csrc"), "-shared", "-o", str(so),
                           str(HERE / "_fast_forms" / "fast_forms_host.cpp")])
    L = C.CDLL(str(so))
    L.ff_build.argtypes = [C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.ff_info.argtypes = [_i32p]
    L.ff_cells.argtypes = [_i32p, C.c_int]
    L.ff_w3.argtypes = [C.POINTER(C.c_uint32), C.c_int]
    return L


def _geometry(ff, w, h, nf, sf, nl, ini=20, mn=7):
    """None if the geometry is refused, else (info dict, cells [n, 4], w3 [n + 1]) of the host geometry."""
    if ff.ff_build(nf, sf, nl, ini, mn, h, w) != 0:
        return None
    o = np.zeros(6, np.int32)
    ff.ff_info(o.ctypes.data_as(_i32p))
    info = dict(zip(("cells", "max_vw", "cand_segmented", "plain", "tile_pitch", "prefetch_chunks"), o.tolist()))
    cells = np.zeros((info["cells"], 4), np.int32)
    assert ff.ff_cells(cells.ctypes.data_as(_i32p), len(cells)) == len(cells)
    w3 = np.zeros(info["cells"] + 1, np.uint32)
    assert ff.ff_w3(w3.ctypes.data_as(C.POINTER(C.c_uint32)), len(w3)) == len(w3)
    return info, cells, w3


def _restate(cells):
    """(tile pitch of the class, slivers, tiles beyond the prefetch registers) from the cell rectangles alone: the tile of
    a cell starts at the 4-byte aligned column at or below x0 - 3 and spans ox + vw + 6 bytes by vh + 6 rows."""
    x0, y0, x1, y1 = (cells[:, k].astype(np.int64) for k in range(4))
    vw, vh = x1 - x0, y1 - y0
    live = (vw > 0) & (vh > 0)
    ox = (x0 - 3) % 4
    tdw = -(-(ox + vw + 6) // 4)      # dwords per tile row
    nq4 = -(-tdw // 4)                # 16-byte chunks per tile row
    max_vw = int(vw.max())
    pitch = 52 if max_vw <= 40 else 68 if max_vw <= 56 else 84
    sliver = live & (tdw < 4)
    over = live & (nq4 * (vh + 6) > PREFETCH_CHUNKS[pitch])
    return pitch, int(sliver.sum()), int(over.sum())


def _reference_configs():
    cases = json.loads((HERE / "golden" / "reference_configs.json").read_text())["cases"]
    return [tuple(c["params"][k] for k in ("w", "h", "nFeatures", "scaleFactor", "nLevels", "iniThFAST", "minThFAST"))
            for c in cases]


def test_plain_predicate_restated_over_the_reference_configurations(ff):
    """Geometry::fastPlain == "no sliver and no oversized tile" restated from the cell rectangles, for every reference
    configuration; all of them are plain with segmented lists, in the 52- and 68-byte classes only (the reason the 84-byte
    class has no specialised instantiation), and the records' own fields give the same answer."""
    pitches = set()
    for (w, h, nf, sf, nl, ini, mn) in _reference_configs():
        info, cells, w3 = _geometry(ff, w, h, nf, sf, nl, ini, mn)
        pitch, slivers, over = _restate(cells)
        assert info["tile_pitch"] == pitch and info["prefetch_chunks"] == PREFETCH_CHUNKS[pitch], (w, h, info)
        assert info["plain"] == int(slivers == 0 and over == 0), (w, h, info, slivers, over)
        lv = w3[w3 != 0].astype(np.int64)
        tdw, nq4, th = (lv >> 16) & 31, (lv >> 21) & 7, ((lv >> 7) & 127) + 6
        assert info["plain"] == int(not ((tdw < 4) | (nq4 * th > PREFETCH_CHUNKS[pitch])).any())
        assert w3[-1] == 0  # the empty record past the end
        assert info["plain"] == 1 and info["cand_segmented"] == 1, (w, h, info)
        pitches.add(pitch)
    assert pitches == {52, 68}


def test_plain_predicate_restated_over_geometries_that_are_not_plain(ff):
    """The same restatement where the answer is `not plain`: widths around the first sliver, and a few plain neighbours."""
    seen = set()
    for w in range(896, 921):
        g = _geometry(ff, w, 120, 500, 1.2, 2)
        assert g is not None
        info, cells, _ = g
        pitch, slivers, over = _restate(cells)
        assert info["tile_pitch"] == pitch and info["plain"] == int(slivers == 0 and over == 0), (w, info, slivers, over)
        seen.add(info["plain"])
    assert seen == {0, 1}


def _sliver_geometry(ff):
    """The narrowest single-level image whose record array holds a live sliver cell, at the smallest height the geometry
    accepts for that width."""
    for w in range(100, 1000):
        for h in range(67, 161):  # 67 = one 35 px cell between the 16 px borders
            g = _geometry(ff, w, h, 300, 1.2, 1)
            if g is None:
                continue
            if _restate(g[1])[1] == 0:
                break  # slivers depend on the width alone
            return w, h, g
    raise AssertionError("no sliver geometry below 1000 px")


def test_no_small_geometry_has_a_tile_beyond_the_prefetch_registers(ff):
    """Every level size up to 320 x 240 at the heights that give the tallest cells (60..69 rows: one row of cells) and, as a
    sample of the rest, every eighth height: no live cell's tile exceeds its class's prefetch registers (module docstring)."""
    heights = list(range(32 + 60, 32 + 70)) + list(range(67, 241, 8))
    built = 0
    for h in heights:
        for w in range(67, 321):
            g = _geometry(ff, w, h, 300, 1.2, 1)
            if g is None:
                continue
            built += 1
            assert _restate(g[1])[2] == 0, (w, h)
    assert built > 5000


# ---------------------------------------------------------------------------------------------------------------------------
def _host(ex, frames):
    """The blocking host entry as [B, 2] counts, [B, cap] records, [B, cap, 32] descriptors (zero beyond each count)."""
    B, H, W = frames.shape
    cap = ex.capacity(H, W)
    counts = np.zeros((B, 2), np.int32)
    kps = np.zeros((B, cap), orb.KP_DTYPE)
    desc = np.zeros((B, cap, 32), np.uint8)
    for f, (mono, k, d) in enumerate(ex.extract_batch(frames)):
        counts[f] = len(k), mono
        kps[f, :len(k)], desc[f, :len(k)] = k, d
    return counts, kps, desc


def _check_oracle(got, frames, cfg, cap, what):
    nf, sf, nl, ini, mn = cfg
    want = ol.extract_batch(frames, nf, cap, sf, nl, ini, mn, (0, 0))
    bad = ol.compare_batch(*got, *want)
    assert bad == [], f"{what}: frames {bad} differ from the oracle"


C2 = (1000, 1.2, 8, 20, 7)
# the default content; a dense class (every pixel passes the N / S / W / E test: phase 1b and the one-entry-per-pixel
# re-unpack); a smooth class whose cells take the minThFAST pass
CONTENTS = ["rectangles", "checker1", "value_noise"]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", CONTENTS)
def test_c2_takes_the_specialised_form_and_the_general_form_gives_the_same_bytes(kind):
    frames = np.stack([synth.content_frame(kind, 640, 480, 1000, t) for t in range(4)])
    ex = orb.ORBextractor(*C2, max_batch=4)
    auto = _host(ex, frames)
    fa = ex.debug_launch_forms()
    assert fa["fast_specialised"] == 1 and fa["cand_segmented"] == 1 and fa["fast_tile_pitch"] == 52, fa
    ex.set_fast_form(0)
    general = _host(ex, frames)
    fg = ex.debug_launch_forms()
    assert fg["fast_specialised"] == 0 and fg["fast_tile_pitch"] == 52 and fg["nframes"] == 4, fg
    for a, g, name in zip(auto, general, ("counts", "keypoints", "descriptors")):
        assert a.tobytes() == g.tobytes(), (kind, name)
    ex.set_fast_form(-1)
    again = _host(ex, frames[:2])
    assert ex.debug_launch_forms()["fast_specialised"] == 1
    assert all(a[:2].tobytes() == b.tobytes() for a, b in zip(auto, again))
    _check_oracle(auto, frames, C2, ex.capacity(480, 640), f"C2 {kind}")
    assert auto[0][:, 0].min() > 0, "a frame without keypoints checks nothing"


@pytest.mark.gpu
def test_68_byte_class_specialised_and_general():
    """512 x 512 (TUM-VI): the other tile class with a specialised instantiation."""
    cfg = (1000, 1.2, 8, 20, 7)
    frames = np.stack([synth.content_frame(k, 512, 512, 7, t) for t, k in enumerate(("rectangles", "photo_china"))])
    ex = orb.ORBextractor(*cfg, max_batch=2)
    auto = _host(ex, frames)
    fa = ex.debug_launch_forms()
    assert fa["fast_specialised"] == 1 and fa["fast_tile_pitch"] == 68, fa
    ex.set_fast_form(0)
    general = _host(ex, frames)
    assert ex.debug_launch_forms()["fast_specialised"] == 0
    assert all(a.tobytes() == g.tobytes() for a, g in zip(auto, general))
    _check_oracle(auto, frames, cfg, ex.capacity(512, 512), "512x512")


@pytest.mark.gpu
def test_sliver_geometry_takes_the_general_form(ff):
    """908 x 86, one level: 876 columns between the borders make 25 columns of 36 px cells, and the last cell keeps
    876 - 24 * 36 - 6 = 6 columns (x 883..888): a tile row of 6 + 6 bytes = 3 dwords, fewer than one 16-byte chunk.  No
    narrower image has a sliver (module docstring) -- the issue's "about 200 x 160" cannot hold one -- so this is the
    smallest: the first width of the search, at the smallest height the geometry accepts for it (one row of cells)."""
    w, h, (info, cells, _) = _sliver_geometry(ff)
    assert (w, h) == (908, 86), (w, h)
    assert info["plain"] == 0 and info["cand_segmented"] == 1 and _restate(cells)[1] >= 1
    cfg = (300, 1.2, 1, 20, 7)
    frames = np.stack([synth.sequence_frame(w, h, 11, 0), synth.content_frame("photo_china", w, h, 12, 1),
                       synth.content_frame("checker2", w, h, 13, 2)])
    ex = orb.ORBextractor(*cfg, max_batch=3)
    got = _host(ex, frames)
    forms = ex.debug_launch_forms()
    assert forms["fast_specialised"] == 0 and forms["cand_segmented"] == 1, forms
    _check_oracle(got, frames, cfg, ex.capacity(h, w), f"sliver {w}x{h}")
    # the sliver's own pixels: level-0 candidates of the last cell column, as the oracle's
    ref = ol.OracleExtractor(*cfg)
    ref(frames[1])
    gx, gy, gr = ex.candidates(0, frame=1)
    rx, ry, rr = ref.candidates(0)
    assert sorted(zip(gx.tolist(), gy.tolist(), gr.tolist())) == sorted(zip(rx.tolist(), ry.tolist(), rr.tolist()))


@pytest.mark.gpu
def test_a_level_of_more_than_4096_cells_takes_the_general_form():
    """2400 x 2336, one level: 67 x 65 = 4 355 cells -- one atomically appended candidate list per level, which only the
    general form (kSeg = false) carries."""
    w, h, cfg = 2400, 2336, (1500, 1.2, 1, 20, 7)
    frames = np.stack([synth.frame(w, h, 4321), synth.content_frame("photo_china", w, h, 5, 1)])
    ex = orb.ORBextractor(*cfg, max_batch=2)
    got = _host(ex, frames)
    forms = ex.debug_launch_forms()
    assert forms["cand_segmented"] == 0 and forms["fast_specialised"] == 0, forms
    _check_oracle(got, frames, cfg, ex.capacity(h, w), "2400x2336")
