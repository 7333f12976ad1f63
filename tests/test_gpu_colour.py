"""The colour entry points at the conversion kernel's edges, and the gray ingest kernel beside it.

vsg_orb_extract_batch_color / vsg_orb_extract_batch_device_color run k_cvt_gray (vsg_kernels.hip: thread = 4 pixels, block =
1024 pixels of one row, grid z = frame) in front of the stage chain; blocking gray calls of up to 8 frames run k_ingest
there.  Both C entries are called through orb.load_library() with explicit `stride` / `frame_stride` (the Python binding
copies to contiguous first, which hides every layout but one).  Every case checks, byte for byte,
  (a) level 0 of every frame against colour_scenes.gray_reference (the definition, tests/test_colour_scenes.py), and
  (b) counts, monoIndex, keypoint records and descriptors of every frame against OracleExtractor on that gray image.
The scenes are colour_scenes.palette (extremes and rounding-boundary colours on every column) and colour_scenes.textured
(channels with their own gain and offset, frames of a batch distinct).  No tolerance anywhere."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import colour_scenes as cs
import oracle_lib as ol
from test_gpu_extract import assert_same_output
from visual_sgraphs_amd import orb

pytestmark = pytest.mark.gpu

INVALID, EMPTY, CAPACITY = -6, -1, -2   # VSG_ERR_INVALID, VSG_ERR_EMPTY_IMAGE, VSG_ERR_CAPACITY (include/vsg_orb.h)
SENTINEL = 0xA5
DEFAULT = (cs.DEFAULT_COEFFS, cs.DEFAULT_SHIFT)
SF, INI, MIN = cs.EXTRACTOR
ENTRIES = ("host", "device")
_u8p = C.POINTER(C.c_uint8)
_i32p = C.POINTER(C.c_int32)


def _extractor(nf=cs.NFEATURES, nl=cs.NLEVELS, max_batch=1):
    return orb.ORBextractor(nf, SF, nl, INI, MIN, max_batch=max_batch)


def _layout(frames, stride, frame_stride, offset, poison, out=None):
    """The frames ([B, H, W, ch] or [B, H, W]) as a flat byte buffer: frame f at offset + f * frame_stride, its rows
    `stride` bytes apart, every other byte `poison`."""
    B, H = frames.shape[:2]
    row = int(np.prod(frames.shape[2:]))
    assert stride >= row and (B == 1 or frame_stride >= (H - 1) * stride + row)
    n = offset + (B - 1) * frame_stride + (H - 1) * stride + row + 9
    raw = np.empty(n, np.uint8) if out is None else out[:n]
    raw[:] = poison
    view = np.lib.stride_tricks.as_strided(raw[offset:], (B, H, row), (frame_stride, stride, 1))
    view[:] = frames.reshape(B, H, row)
    return raw


class _Result:
    """What one call of a C entry returned: rc and the [B, capacity] output arrays as the entry left them."""

    def __init__(self, rc, n, mono, kps, desc, src_after):
        self.rc, self.n, self.mono, self.kps, self.desc, self.src_after = rc, n, mono, kps, desc, src_after

    def frame(self, f):
        k = int(self.n[f])
        return int(self.mono[f]), self.kps[f, :k].copy(), self.desc[f, :k].copy()

    def untouched(self):
        return all((np.ascontiguousarray(a).view(np.uint8) == SENTINEL).all() for a in (self.n, self.mono, self.kps, self.desc))

    def same_as(self, other):
        return all(np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes() for a, b in
                   ((self.n, other.n), (self.mono, other.mono), (self.kps, other.kps), (self.desc, other.desc)))


def _call(ex, entry, raw, offset, channels, rgb, B, frame_stride, H, W, stride, lap=(0, 0), stream="torch", out_frames=None,
          override=None):
    """One call of vsg_orb_extract_batch_color ("host"), vsg_orb_extract_batch_device_color ("device") or, with channels ==
    0, vsg_orb_extract_batch ("gray") on the image at raw[offset:].  `override` replaces C arguments by name (img=None is a
    NULL image) after the sentinel-filled outputs have been sized for the true geometry."""
    L = orb.load_library()
    cap = ex.capacity(H, W)
    nb = out_frames or B
    a = dict(img=0, channels=channels, rgb=int(bool(rgb)), nframes=B, frame_stride=frame_stride, rows=H, cols=W, stride=stride,
             capacity=cap)
    a.update(override or {})
    h = ex.handle
    if entry in ("host", "gray"):
        kps = np.full((nb, cap, 28), SENTINEL, np.uint8)
        desc = np.full((nb, cap, 32), SENTINEL, np.uint8)
        n, mono = (np.full(4 * nb, SENTINEL, np.uint8).view(np.int32) for _ in range(2))
        img = None if a["img"] is None else C.cast(raw.ctypes.data + offset, _u8p)
        tail = (int(lap[0]), int(lap[1]), kps.ctypes.data_as(C.c_void_p), desc.ctypes.data_as(_u8p), a["capacity"],
                n.ctypes.data_as(_i32p), mono.ctypes.data_as(_i32p))
        if entry == "host":
            rc = L.vsg_orb_extract_batch_color(h, img, a["channels"], a["rgb"], a["nframes"], a["frame_stride"], a["rows"],
                                               a["cols"], a["stride"], *tail)
        else:
            rc = L.vsg_orb_extract_batch(h, img, a["nframes"], a["frame_stride"], a["rows"], a["cols"], a["stride"], *tail)
        return _Result(rc, n, mono, kps.view(orb.KP_DTYPE).reshape(nb, cap), desc, raw.copy())
    import torch
    dev = torch.device("cuda", 0)
    d_raw = torch.from_numpy(raw).to(dev)
    d_kps = torch.full((nb, cap, 28), SENTINEL, dtype=torch.uint8, device=dev)
    d_desc = torch.full((nb, cap, 32), SENTINEL, dtype=torch.uint8, device=dev)
    d_counts = torch.full((nb, 8), SENTINEL, dtype=torch.uint8, device=dev)
    img = None if a["img"] is None else C.c_void_p(d_raw.data_ptr() + offset)

    def run(st):
        return L.vsg_orb_extract_batch_device_color(h, img, a["channels"], a["rgb"], a["nframes"], a["frame_stride"],
                                                    a["rows"], a["cols"], a["stride"], int(lap[0]), int(lap[1]),
                                                    C.c_void_p(d_kps.data_ptr()), C.c_void_p(d_desc.data_ptr()),
                                                    C.c_void_p(d_counts.data_ptr()), a["capacity"], st)
    if stream == "torch":  # a stream of the caller's own, as tests/test_gpu_extract.py's device-entry test has it
        st = torch.cuda.Stream(device=dev)
        st.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(st):
            rc = run(C.c_void_p(st.cuda_stream))
        st.synchronize()
    else:  # stream = NULL: the chain is ordered between the fills above and the read-back below on the NULL stream
        assert stream == "null" and torch.cuda.current_stream(dev).cuda_stream == 0
        rc = run(None)
    counts = d_counts.cpu().numpy().view(np.int32).reshape(nb, 2)
    return _Result(rc, counts[:, 0].copy(), counts[:, 1].copy(), d_kps.cpu().numpy().view(orb.KP_DTYPE).reshape(nb, cap),
                   d_desc.cpu().numpy(), d_raw.cpu().numpy())


_ORACLE = {}


def _oracle(gray, nf, nl, lap=(0, 0)):
    """OracleExtractor on one gray image, computed once per image and parameter set and shared between the tests"""
    key = (hashlib.sha1(gray.tobytes()).digest(), gray.shape, nf, nl, tuple(lap))
    if key not in _ORACLE:
        _ORACLE[key] = ol.OracleExtractor(nf, SF, nl, INI, MIN)(gray, tuple(lap))
    return _ORACLE[key]


def _check(ex, res, frames, rgb, what, table=DEFAULT, nf=cs.NFEATURES, nl=cs.NLEVELS, lap=(0, 0), outputs=True):
    """(a) and (b) of the module docstring for every frame of one good call"""
    assert res.rc == 0, f"{what}: rc {res.rc} {orb.load_library().vsg_last_error()}"
    for f, col in enumerate(frames):
        gray = cs.gray_reference(col, rgb, *table) if col.ndim == 3 else col
        got = ex.image_pyramid(0, frame=f)
        bad = np.argwhere(got != gray)
        assert len(bad) == 0, (f"{what}: level 0 of frame {f} differs at {len(bad)} pixels, first (y, x) {bad[:6].tolist()}: "
                               f"{[int(got[y, x]) for y, x in bad[:6]]} != {[int(gray[y, x]) for y, x in bad[:6]]}")
        if outputs:
            assert_same_output(res.frame(f), _oracle(gray, nf, nl, lap), f"{what} frame {f}")


def _contiguous(ex, entry, frames, rgb, **kw):
    B, H, W, ch = frames.shape
    return _call(ex, entry, _layout(frames, W * ch, H * W * ch, 0, 0), 0, ch, rgb, B, H * W * ch, H, W, W * ch, **kw)


def _textured(w, h, ch, B, first=0):
    return np.stack([cs.textured(w, h, ch, cs.SEED + first + f) for f in range(B)])


# ---------------------------------------------------------------------------------------------------------------------------
# widths: the partial last 4-pixel group, the 1024-pixel block edge, a third block, and the one 8-level geometry
GEOMETRIES = [(w, cs.rows_for(w), cs.NFEATURES, cs.NLEVELS) for w in cs.WIDTHS] + [cs.MULTI_LEVEL]


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("rgb", [True, False], ids=["rgb", "bgr"])
@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("w,h,nf,nl", GEOMETRIES, ids=[f"{g[0]}x{g[1]}" for g in GEOMETRIES])
def test_every_width_class(w, h, nf, nl, channels, rgb, entry):
    ex = _extractor(nf, nl)
    pal = cs.palette(w, h, channels, w + channels)[None]
    _check(ex, _contiguous(ex, entry, pal, rgb), pal, rgb, f"palette {w}x{h}x{channels} {entry}", nf=nf, nl=nl, outputs=False)
    tex = _textured(w, h, channels, 1)
    _check(ex, _contiguous(ex, entry, tex, rgb), tex, rgb, f"textured {w}x{h}x{channels} {entry}", nf=nf, nl=nl)


# ---------------------------------------------------------------------------------------------------------------------------
# batches of distinct frames in unaligned layouts
def _padded(frames, offset, poison):
    B, H, W, ch = frames.shape
    stride = W * ch + 5                 # rows start at odd addresses
    frame_stride = H * stride + 7
    return _layout(frames, stride, frame_stride, offset, poison), stride, frame_stride


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("offset", [1, 3])
@pytest.mark.parametrize("B", [3, 4])
@pytest.mark.parametrize("channels", [3, 4])
def test_batches_with_padded_rows_frames_and_odd_base(channels, B, offset, entry):
    w, h, rgb = 1027, cs.rows_for(1027), offset == 1
    ex = _extractor(max_batch=4)
    frames = _textured(w, h, channels, B)
    raw, stride, fs = _padded(frames, offset, 0xEE)
    first = _call(ex, entry, raw, offset, channels, rgb, B, fs, h, w, stride)
    _check(ex, first, frames, rgb, f"{entry} B={B} ch={channels} offset={offset}")
    assert np.array_equal(first.src_after, raw), "the call changed its source image"
    level0 = [ex.image_pyramid(0, frame=f) for f in range(B)]
    # other pad bytes, other alpha: nothing but the colour bytes may reach the output
    again = frames.copy()
    if channels == 4:
        again[..., 3] = np.random.default_rng(offset).integers(0, 256, again.shape[:3])
        assert (again[..., 3] != frames[..., 3]).mean() > 0.9
    raw2, _, _ = _padded(again, offset, 0x11)
    second = _call(ex, entry, raw2, offset, channels, rgb, B, fs, h, w, stride)
    assert second.rc == 0 and second.same_as(first)
    for f in range(B):
        assert np.array_equal(ex.image_pyramid(0, frame=f), level0[f])
    assert np.array_equal(second.src_after, raw2)


@pytest.mark.parametrize("stream", ["torch", "null"])
def test_device_entry_on_a_caller_stream_and_on_the_null_stream(stream):
    w, h, B = 1025, cs.rows_for(1025), 2
    ex = _extractor(max_batch=B)
    frames = _textured(w, h, 4, B)
    raw, stride, fs = _padded(frames, 3, 0xEE)
    _check(ex, _call(ex, "device", raw, 3, 4, False, B, fs, h, w, stride, stream=stream), frames, False, f"stream {stream}")
    pal = np.stack([cs.palette(w, h, 3, s) for s in (1, 2)])
    raw, stride, fs = _padded(pal, 1, 0xEE)
    _check(ex, _call(ex, "device", raw, 1, 3, True, B, fs, h, w, stride, stream=stream), pal, True, f"palette, stream {stream}",
           outputs=False)


# ---------------------------------------------------------------------------------------------------------------------------
# coefficients are data of the handle
@pytest.mark.parametrize("table", cs.ALT_TABLES, ids=[f"{c[0]}_{c[1]}_{c[2]}_s{s}" for c, s in cs.ALT_TABLES])
def test_coefficient_tables_reach_both_entries_and_survive_a_size_change(table):
    ex = _extractor()
    ex.set_gray_coeffs(*table)
    for w in (131, 1025):  # the second width re-builds the handle's geometry
        for entry in ENTRIES:
            for rgb in (True, False):
                pal = cs.palette(w, cs.rows_for(w), 4, w)[None]
                assert (cs.gray_reference(pal, rgb, *table) != cs.gray_reference(pal, rgb)).any()  # the table matters
                _check(ex, _contiguous(ex, entry, pal, rgb), pal, rgb, f"palette {table} {w} {entry}", table, outputs=False)
                if table[0] == (16384, 0, 0):
                    assert np.array_equal(ex.image_pyramid(0), pal[0, ..., 0 if rgb else 2])   # R alone
                if table[0] == (0, 0, 16384):
                    assert np.array_equal(ex.image_pyramid(0), pal[0, ..., 2 if rgb else 0])   # B alone
                tex = _textured(w, cs.rows_for(w), 3, 1)
                _check(ex, _contiguous(ex, entry, tex, rgb), tex, rgb, f"textured {table} {w} {entry}", table)


@pytest.mark.parametrize("entry", ENTRIES)
def test_refused_tables_leave_the_previous_one_and_the_default_comes_back(entry):
    L = orb.load_library()
    ex = _extractor()
    pal = cs.palette(131, cs.H, 3, 8)[None]
    alt = cs.ALT_TABLES[2]
    assert (cs.gray_reference(pal, True, *alt) != cs.gray_reference(pal, True)).any()

    def holds(table, what):
        _check(ex, _contiguous(ex, entry, pal, True), pal, True, what, table, outputs=False)

    holds(DEFAULT, "before any table was set")
    ex.set_gray_coeffs(*alt)
    holds(alt, "after the set")

    def coeffs(*c):
        return (C.c_int32 * 3)(*c)
    refused = [("NULL handle", None, coeffs(*cs.DEFAULT_COEFFS), 14), ("NULL table", ex.handle, None, 14),
               ("shift 0", ex.handle, coeffs(1, 0, 0), 0), ("shift 21", ex.handle, coeffs(1 << 21, 0, 0), 21),
               ("sum below 1 << shift", ex.handle, coeffs(4899, 9617, 1867), 14),
               ("sum above 1 << shift", ex.handle, coeffs(4899, 9617, 1869), 14),
               ("the default table at another shift", ex.handle, coeffs(*cs.DEFAULT_COEFFS), 15)]
    for what, h, c, shift in refused:
        assert L.vsg_orb_set_gray_coeffs(h, c, shift) == INVALID, what
        holds(alt, f"after the refused {what}")
    ex.set_gray_coeffs(*DEFAULT)
    holds(DEFAULT, "after the default was set again")


# ---------------------------------------------------------------------------------------------------------------------------
# colour calls between gray calls, a larger batch, a pyramid read-back and other image sizes on ONE handle: the host entry's
# upload buffer is shared with the bordered read-back and grows with the batch and the geometry
@pytest.mark.parametrize("entry", ENTRIES)
def test_colour_calls_interleaved_with_other_work_on_one_handle(entry):
    nf, nl = 400, 3
    g1, g2 = (163, 121), (262, 191)
    ex = _extractor(nf, nl, max_batch=4)

    def colour(handle, frames, rgb, padded, what):
        B, H, W, ch = frames.shape
        if padded:
            raw, stride, fs = _padded(frames, 1, 0xEE)
            res = _call(handle, entry, raw, 1, ch, rgb, B, fs, H, W, stride)
        else:
            res = _contiguous(handle, entry, frames, rgb)
        _check(handle, res, frames, rgb, what, nf=nf, nl=nl)
        return res

    def step(frames, rgb, padded, what):
        res = colour(ex, frames, rgb, padded, what)
        fresh = colour(_extractor(nf, nl, max_batch=4), frames, rgb, padded, what + " (fresh handle)")
        assert res.same_as(fresh), what
        return res

    one = _textured(*g1, 3, 1)
    first = step(one, True, False, "1. colour B=1")
    grays = np.stack([cs.gray_reference(c, True) for c in _textured(*g1, 3, 2, first=4)])
    for f, got in enumerate(ex.extract_batch(grays)):
        assert_same_output(got, _oracle(grays[f], nf, nl), f"2. gray batch frame {f}")
        assert np.array_equal(ex.image_pyramid(0, frame=f), grays[f])
    four = _textured(*g1, 4, 4)
    step(four, False, True, "3. colour B=4")
    ref = ol.OracleExtractor(nf, SF, nl, INI, MIN)
    ref(cs.gray_reference(four[2], False))
    assert np.array_equal(ex.image_pyramid(1, frame=2, with_border=True), ref.pyramid_level(1, with_border=True)), "4."
    assert np.array_equal(ex.image_pyramid(0, frame=3), cs.gray_reference(four[3], False)), "4. level 0 after the read-back"
    step(_textured(*g2, 4, 4), True, True, "5. colour B=4 at a larger geometry")
    again = step(one, True, False, "6. the first geometry again")
    assert again.same_as(first)


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
def test_lapping_area_inside_the_image(entry):
    """vLappingArea of the stereo-fisheye rigs: monoIndex and the order of the records (mono features first) equal the
    oracle's, as tests/test_gpu_launch_forms.py test_lapping_area_batches has it for the gray entries."""
    w, h, nf, nl = cs.MULTI_LEVEL
    lap = (100, 200)
    ex = _extractor(nf, nl, max_batch=2)
    frames = _textured(w, h, 3, 2)
    raw, stride, fs = _padded(frames, 1, 0xEE)
    res = _call(ex, entry, raw, 1, 3, False, 2, fs, h, w, stride, lap=lap)
    _check(ex, res, frames, False, f"lapping {lap} {entry}", nf=nf, nl=nl, lap=lap)
    for f in range(2):
        assert 0 < res.mono[f] < res.n[f]   # features on both sides of the split
        assert res.frame(f)[1].tobytes() != _oracle(cs.gray_reference(frames[f], False), nf, nl)[1].tobytes()  # order changed


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
def test_refusals_touch_nothing(entry):
    w, h, ch, mb = 131, cs.H, 3, 2
    ex = _extractor(max_batch=mb)
    frames = _textured(w, h, ch, mb + 1)       # one frame more than max_batch, so that no refused count has too little behind it
    stride, fs = w * ch, h * w * ch
    raw = _layout(frames, stride, fs, 0, 0)

    def call(B=mb, **override):
        return _call(ex, entry, raw, 0, ch, True, B, fs, h, w, stride, out_frames=mb + 1, override=override)

    def good(what):
        res = call()
        _check(ex, res, frames[:mb], True, what)
        return res

    good("before the refusals")
    forms = ex.debug_launch_forms()
    cap = ex.capacity(h, w)
    refused = [(dict(channels=c), INVALID) for c in (1, 2, 5)] + \
              [(dict(img=None), EMPTY), (dict(rows=0), EMPTY), (dict(cols=0), EMPTY),
               (dict(nframes=0), INVALID), (dict(nframes=mb + 1), INVALID),
               (dict(stride=w * ch - 1), INVALID), (dict(stride=w), INVALID), (dict(stride=0), INVALID), (dict(stride=-stride), INVALID)]
    if entry == "device":
        refused += [(dict(capacity=cap - 1), CAPACITY), (dict(capacity=0), CAPACITY)]
    for override, code in refused:
        res = call(**override)
        assert res.rc == code, (override, res.rc)
        assert res.untouched(), f"{override}: a refused call wrote to its outputs"
        assert ex.debug_launch_forms() == forms, f"{override}: a refused call enqueued work"
        assert np.array_equal(ex.image_pyramid(0, frame=1), cs.gray_reference(frames[1], True)), override
    if entry == "device":  # 4 channels with the stride of 3: the rows would overlap silently
        assert call(channels=4).rc == INVALID
    good("after the refusals")


# ---------------------------------------------------------------------------------------------------------------------------
# the gray level-0 staging beside it: blocking calls of up to 8 frames read the image with k_ingest (thread = 16 bytes of a
# row, narrower moves at the end of a row), in place from vsg_host_alloc memory or from the slot's staging for pageable memory
@pytest.mark.parametrize("source", ["pinned", "pageable"])
@pytest.mark.parametrize("B", [1, 2, 8])
@pytest.mark.parametrize("w", cs.INGEST_WIDTHS)
def test_gray_ingest_from_unaligned_sub_views(w, B, source):
    h = cs.H
    ex = _extractor(max_batch=8)
    grays = np.stack([cs.gray_reference(c, True) for c in _textured(w, h, 3, B)])
    offset = 3                                         # odd column offset into the parent rows
    stride = w + 5 if (w + 5) % 4 else w + 6           # no multiple of 4
    fs = h * stride + 7                                # a gap between the frames
    assert offset % 2 == 1 and stride % 4 != 0
    nbytes = offset + (B - 1) * fs + h * stride + 16
    if source == "pinned":
        parent = orb.PinnedArray((nbytes,))
        raw = _layout(grays, stride, fs, offset, 0xEE, out=parent.a)
        assert orb.host_kind(parent.a) == "vsg_host_alloc"
    else:
        raw = _layout(grays, stride, fs, offset, 0xEE)
        assert orb.host_kind(raw) == "pageable"
    res = _call(ex, "gray", raw, offset, 0, True, B, fs, h, w, stride)
    forms = ex.debug_launch_forms()
    assert forms["latency_chain"] == 1 and forms["nframes"] == B, forms   # the chain k_ingest belongs to
    _check(ex, res, list(grays), True, f"ingest {w} B={B} {source}")
    assert np.array_equal(res.src_after, raw)
