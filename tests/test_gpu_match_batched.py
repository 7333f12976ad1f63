"""vsg_hamming_block_best2_device -- the matcher call the benchmark times -- at its count, stride and tie edges.

The scenes of tests/match_scenes.py (proven on the CPU by tests/test_match_scenes.py) as batched launches on device buffers,
through ctypes like tests/test_gpu_every_frame.py.  Every comparison is with match_scenes.best2_reference, on EVERY row of
EVERY block: rows below the clamped count must equal it, every other output row must still hold the sentinel the outputs
were filled with.  Each test prints how many blocks and rows it compared."""
import ctypes as C
import functools

import numpy as np
import pytest

import match_scenes as ms
from visual_sgraphs_amd import orb

pytestmark = pytest.mark.gpu

M = ms.COUNT_MAX_ROWS
VSG_OK, VSG_ERR_UNSUPPORTED, VSG_ERR_INVALID = 0, -3, -6
POISON = 5  # what sits between the counts when count_stride > 1: no scene has a count of 5


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


def _dev(x):
    torch, dev = _torch()
    return torch.from_numpy(np.array(x, order="C")).to(dev)  # a copy: the scenes are read-only arrays


def _outputs(nblocks, max_rows):
    torch, dev = _torch()
    return [torch.full((nblocks, max_rows), ms.SENTINEL, dtype=torch.int32, device=dev) for _ in range(3)]


def _counts(values, stride=1):
    """[len(values), stride] int32 on the device: the count in column 0, POISON in the gaps."""
    c = np.full((len(values), stride), POISON, np.int32)
    c[:, 0] = values
    return _dev(c)


def _ptr(t):
    if t is None:
        return None
    return C.c_void_p(t if isinstance(t, int) else t.data_ptr())


def _call(d_a, d_b, block_stride, d_ca, d_cb, count_stride, nblocks, max_rows, outs, stream=None):
    """The raw call; tensors, raw addresses or None for the pointers.  Everything enqueued before it has finished when it
    is made, and the caller synchronises before reading."""
    torch, _ = _torch()
    torch.cuda.synchronize()
    return orb.load_library().vsg_hamming_block_best2_device(
        0, _ptr(d_a), _ptr(d_b), block_stride, _ptr(d_ca), _ptr(d_cb), count_stride, nblocks, max_rows, _ptr(outs[0]),
        _ptr(outs[1]), _ptr(outs[2]), _ptr(stream))


def _host(outs):
    torch, _ = _torch()
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs]


def _compare(outs, refs, max_rows, names, what):
    """outs: three host arrays [nblocks, max_rows]; refs[i] = (best, second, arg) of block i, each of the clamped na[i] rows.
    Rows below na[i] equal the reference, all others still hold the sentinel.  Returns the number of rows compared."""
    rows = 0
    for i, ref in enumerate(refs):
        n = len(ref[0])
        for got, want, field in zip(outs, ref, ("best", "second", "argbest")):
            if not np.array_equal(got[i, :n], want):
                q = int(np.flatnonzero(got[i, :n] != want)[0])
                got3, want3 = [int(o[i, q]) for o in outs], [int(r[q]) for r in ref]
                pytest.fail(f"{what}: block {i} ({names[i]}), A row {q}: {field} differs; (best, second, arg) = {got3}, "
                            f"reference {want3}")
            left = got[i, n:]
            if not (left == ms.SENTINEL).all():
                q = n + int(np.flatnonzero(left != ms.SENTINEL)[0])
                pytest.fail(f"{what}: block {i} ({names[i]}): {field} row {q} was written, at or past na = {n} "
                            f"(now {int(got[i, q])})")
        rows += n
    assert len(refs) == outs[0].shape[0]
    print(f"{what}: {len(refs)} blocks, {rows} rows compared, {len(refs) * max_rows - rows} rows still the sentinel")
    return rows


# ---- the count scene, its references (computed once per distinct (rows, counts)) and its device copies
@functools.lru_cache(maxsize=None)
def _ref(side_a, ia, n, side_b, ib, m):
    """Reference of rows [:n] of block ia of count_scene()[side_a] against rows [:m] of block ib of [side_b]."""
    scene = ms.count_scene()
    out = ms.best2_reference(scene[side_a][ia], n, scene[side_b][ib], m)
    for v in out:
        v.setflags(write=False)
    return out


def _count_refs(na, nb, max_rows=M):
    """Block i of the count scene under (na[i], nb[i]); None = no count pointer on that side = max_rows rows."""
    N = len(ms.COUNT_PAIRS)
    na = [max_rows] * N if na is None else na
    nb = [max_rows] * N if nb is None else nb
    return [_ref(0, i, ms.clamp(na[i], max_rows), 1, i, ms.clamp(nb[i], max_rows)) for i in range(N)]


COUNT_NAMES = [f"na={n} nb={m}" for n, m in ms.COUNT_PAIRS]


@functools.lru_cache(maxsize=None)
def _count_scene_on_device(stale):
    a, b, na, nb = ms.count_scene()
    if stale:
        a, b = ms.with_stale_rows(a, b, na, nb, M)
    return _dev(a), _dev(b)


# ---- seams
@pytest.mark.parametrize("which", list(ms.CASE_LISTS))
def test_seams_one_launch_per_case_list(which):
    """Ties and best / second-best orders across the seams of the C/D layout, the accumulator's extremes, the query in every
    wave and query set, and the second prefetch-group edge: every case one block of a single launch.  A failure names the
    case (positions, d) and the seam it lies across."""
    make, max_rows = ms.CASE_LISTS[which]
    cases = make()
    a, b, na, nb = ms.pack_cases(cases, max_rows)
    outs = _outputs(len(cases), max_rows)
    rc = _call(_dev(a), _dev(b), max_rows * 32, _counts(na), _counts(nb), 1, len(cases), max_rows, outs)
    assert rc == VSG_OK, rc
    best, second, arg = host = _host(outs)
    bad = []
    for i, c in enumerate(cases):
        for row, want in c["expect"].items():
            got = (int(best[i, row]), int(second[i, row]), int(arg[i, row]))
            if got != want:
                bad.append(f"{c['name']} [{' + '.join(c['seam']) or 'no pair'}]: got {got}, built to give {want}")
    assert not bad, f"{len(bad)} of {len(cases)} directed cases of '{which}' fail, first: " + "; ".join(bad[:6])
    refs = [ms.best2_reference(c["a"], c["na"], c["b"], c["nb"]) for c in cases]
    _compare(host, refs, max_rows, [c["name"] for c in cases], f"seams/{which}")


# ---- counts
@pytest.mark.parametrize("stale", [False, True], ids=["rows_past_the_count_are_data_of_their_own", "stale_copies_of_the_queries"])
def test_counts_side_by_side_in_one_launch(stale):
    """Empty, one-row, tile-edge, workgroup-edge, over-large and negative counts next to each other in ONE launch.  Rows
    past the counts hold other tie-heavy rows, or (stale) exact copies of the block's queries, the rows of the partial tail
    tile included: a stale row that took part would win at distance 0.  The answer is the same."""
    _, _, na, nb = ms.count_scene()
    d_a, d_b = _count_scene_on_device(stale)
    N = len(na)
    outs = _outputs(N, M)
    rc = _call(d_a, d_b, M * 32, _counts(na, 2), _counts(nb, 2), 2, N, M, outs)
    assert rc == VSG_OK, rc
    _compare(_host(outs), _count_refs(na.tolist(), nb.tolist()), M, COUNT_NAMES, f"counts, stale={stale}")


@pytest.mark.parametrize("count_stride", [1, 2, 5])
def test_count_stride(count_stride):
    _, _, na, nb = ms.count_scene()
    d_a, d_b = _count_scene_on_device(True)
    N = len(na)
    outs = _outputs(N, M)
    rc = _call(d_a, d_b, M * 32, _counts(na, count_stride), _counts(nb, count_stride), count_stride, N, M, outs)
    assert rc == VSG_OK, rc
    _compare(_host(outs), _count_refs(na.tolist(), nb.tolist()), M, COUNT_NAMES, f"count_stride {count_stride}")


@pytest.mark.parametrize("null", ["a", "b", "both"])
def test_null_count_pointer_means_max_rows(null):
    a, b, na, nb = ms.count_scene()
    d_a, d_b = _count_scene_on_device(False)  # every row is data: max_rows rows of it are compared
    N = len(na)
    outs = _outputs(N, M)
    ca = None if null in ("a", "both") else _counts(na, 2)
    cb = None if null in ("b", "both") else _counts(nb, 2)
    rc = _call(d_a, d_b, M * 32, ca, cb, 2, N, M, outs)
    assert rc == VSG_OK, rc
    refs = _count_refs(None if ca is None else na.tolist(), None if cb is None else nb.tolist())
    rows = _compare(_host(outs), refs, M, COUNT_NAMES, f"NULL counts: {null}")
    if ca is None:
        assert rows == N * M


def test_chained_form_block_i_against_block_i_minus_1():
    """What the benchmark does: one descriptor array and one count array with a slot in front, d_b = d_a - block_stride,
    d_counts_b = d_counts_a - count_stride: block i is matched against block i - 1 under ITS count."""
    a, _, na, _ = ms.count_scene()
    d_desc, _ = _count_scene_on_device(True)  # stale rows are copies of rows of the same slot
    N = len(na) - 1
    d_c = _counts(na, 2)
    outs = _outputs(N, M)
    stride, esz = M * 32, d_c.element_size()
    rc = _call(d_desc.data_ptr() + stride, d_desc.data_ptr(), stride, d_c.data_ptr() + 2 * esz, d_c.data_ptr(), 2, N, M, outs)
    assert rc == VSG_OK, rc
    refs = [_ref(0, i + 1, ms.clamp(na[i + 1], M), 0, i, ms.clamp(na[i], M)) for i in range(N)]
    names = [f"slot {i + 1} (n={na[i + 1]}) against slot {i} (n={na[i]})" for i in range(N)]
    _compare(_host(outs), refs, M, names, "chained form")


# ---- block strides
def test_block_stride_0_every_block_reads_the_same_rows():
    _, _, na, nb = ms.count_scene()
    d_a, d_b = _count_scene_on_device(False)
    N = len(na)
    outs = _outputs(N, M)
    rc = _call(d_a, d_b, 0, _counts(na), _counts(nb), 1, N, M, outs)
    assert rc == VSG_OK, rc
    refs = [_ref(0, 0, ms.clamp(na[i], M), 1, 0, ms.clamp(nb[i], M)) for i in range(N)]
    _compare(_host(outs), refs, M, COUNT_NAMES, "block_stride 0")


def test_block_stride_with_padding_rows():
    """(max_rows + 3) * 32: three rows of padding behind every block, filled with copies of its queries like the stale rows."""
    a, b, na, nb = ms.count_scene()
    N = len(na)
    sa, sb = ms.with_stale_rows(*(np.concatenate([v, np.zeros((N, 3, 32), np.uint8)], axis=1) for v in (a, b)), na, nb, M)
    full = ms.COUNT_PAIRS.index((320, 320))
    assert sa.shape == (N, M + 3, 32) and np.array_equal(sb[full, M:], a[full, :3]) and np.array_equal(sa[full, M:], a[full, :3])
    outs = _outputs(N, M)
    rc = _call(_dev(sa), _dev(sb), (M + 3) * 32, _counts(na), _counts(nb), 1, N, M, outs)
    assert rc == VSG_OK, rc
    _compare(_host(outs), _count_refs(na.tolist(), nb.tolist()), M, COUNT_NAMES, "block_stride (max_rows + 3) * 32")


def test_self_match_d_a_equals_d_b():
    """A matched against itself: best == 0 and argbest is the first duplicate at or below the row's own index."""
    rng = np.random.default_rng(25)
    counts = [320, 1, 0, 33, 257, 289, 400, -1, 65, 256]
    N = len(counts)
    base = rng.integers(0, 256, (9, 32), dtype=np.uint8)
    rows = ms.near_duplicates(rng, base, N * M, 1).reshape(N, M, 32)
    d_rows, d_c = _dev(rows), _counts(counts, 2)
    outs = _outputs(N, M)
    rc = _call(d_rows, d_rows, M * 32, d_c, d_c, 2, N, M, outs)
    assert rc == VSG_OK, rc
    best, second, arg = host = _host(outs)
    refs = [ms.best2_reference(rows[i], ms.clamp(n, M), rows[i], ms.clamp(n, M)) for i, n in enumerate(counts)]
    _compare(host, refs, M, [f"n={n}" for n in counts], "self match")
    earlier = 0
    for i, n in enumerate(counts):
        n = ms.clamp(n, M)
        if n == 0:
            continue
        _, first, inverse = np.unique(rows[i, :n], axis=0, return_index=True, return_inverse=True)
        want = first[inverse.reshape(-1)]  # the first row with the same 32 bytes
        assert not best[i, :n].any() and np.array_equal(arg[i, :n], want), (i, n)
        assert (arg[i, :n] <= np.arange(n)).all()
        earlier += int((want < np.arange(n)).sum())
    # a property of the DATA, not of the kernel: about half the rows are an unflipped copy of one of 9 base rows, so that
    # a duplicate in front of the row itself is common (the answer is then not the row's own index)
    assert earlier > sum(ms.clamp(n, M) for n in counts) // 3


# ---- streams
def test_a_side_stream_and_the_null_stream():
    torch, dev = _torch()
    _, _, na, nb = ms.count_scene()
    d_a, d_b = _count_scene_on_device(True)
    N = len(na)
    d_ca, d_cb = _counts(na, 2), _counts(nb, 2)
    side = torch.cuda.Stream(device=dev)
    outs_side, outs_null = _outputs(N, M), _outputs(N, M)
    assert _call(d_a, d_b, M * 32, d_ca, d_cb, 2, N, M, outs_side, stream=side.cuda_stream) == VSG_OK
    assert _call(d_a, d_b, M * 32, d_ca, d_cb, 2, N, M, outs_null, stream=None) == VSG_OK
    refs = _count_refs(na.tolist(), nb.tolist())
    _compare(_host(outs_side), refs, M, COUNT_NAMES, "side stream")
    _compare(_host(outs_null), refs, M, COUNT_NAMES, "NULL stream")


# ---- refusals
def test_refusals_leave_the_outputs_alone():
    """Each bad argument is refused before anything is enqueued; the limits of the packed key (20 bits of row index) and of
    gridDim.y are refused, not launched.  Afterwards a correct call on the same buffers gives the reference."""
    _, _, na, nb = ms.count_scene()
    d_a, d_b = _count_scene_on_device(True)
    N = len(na)
    d_ca, d_cb = _counts(na, 2), _counts(nb, 2)
    outs = _outputs(N, M)
    good = dict(d_a=d_a, d_b=d_b, block_stride=M * 32, d_ca=d_ca, d_cb=d_cb, count_stride=2, nblocks=N, max_rows=M)
    refusals = [("d_a NULL", dict(d_a=None), VSG_ERR_INVALID), ("d_b NULL", dict(d_b=None), VSG_ERR_INVALID),
                ("d_best NULL", dict(null_out=0), VSG_ERR_INVALID), ("d_second NULL", dict(null_out=1), VSG_ERR_INVALID),
                ("d_argbest NULL", dict(null_out=2), VSG_ERR_INVALID),
                ("nblocks 0", dict(nblocks=0), VSG_ERR_INVALID), ("nblocks -1", dict(nblocks=-1), VSG_ERR_INVALID),
                ("max_rows 0", dict(max_rows=0), VSG_ERR_INVALID), ("max_rows -1", dict(max_rows=-1), VSG_ERR_INVALID),
                ("max_rows 2^20 + 1", dict(max_rows=(1 << 20) + 1), VSG_ERR_UNSUPPORTED),
                ("max_rows INT_MAX", dict(max_rows=ms.INT_MAX), VSG_ERR_UNSUPPORTED),
                ("nblocks 65536", dict(nblocks=65536), VSG_ERR_UNSUPPORTED),
                ("nblocks INT_MAX", dict(nblocks=ms.INT_MAX), VSG_ERR_UNSUPPORTED)]
    for what, change, want in refusals:
        kw = dict(good)
        o = list(outs)
        if "null_out" in change:
            o[change["null_out"]] = None
        else:
            kw.update(change)
        rc = _call(kw["d_a"], kw["d_b"], kw["block_stride"], kw["d_ca"], kw["d_cb"], kw["count_stride"], kw["nblocks"],
                   kw["max_rows"], o)
        assert rc == want, (what, rc)
        for h in _host(outs):
            assert (h == ms.SENTINEL).all(), f"{what}: refused, but an output was written"
    rc = _call(*(good[k] for k in ("d_a", "d_b", "block_stride", "d_ca", "d_cb", "count_stride", "nblocks", "max_rows")), outs)
    assert rc == VSG_OK, rc
    _compare(_host(outs), _count_refs(na.tolist(), nb.tolist()), M, COUNT_NAMES, f"after {len(refusals)} refusals")
