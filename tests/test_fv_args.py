"""CPU tests of the FeatureVector argument of the vocabulary-node searches (visual_sgraphs_amd/csrc/vsg_fv.h compiled for the
host by tests/_fvcore): fv_check on a valid CSR and on every single defect, join_nodes against numpy.intersect1d, and
pair_bits_check on the layouts of the triangulation search's predicate bits."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import fv_cases as fc

FC_DIR = Path(__file__).resolve().parent / "_fvcore"
_i32p = C.POINTER(C.c_int32)


def _p(a):
    return a.ctypes.data_as(_i32p)


@pytest.fixture(scope="module")
def core():
    subprocess.check_call(["make", "-C", str(FC_DIR)], stdout=subprocess.DEVNULL)
    L = C.CDLL(str(FC_DIR / "libvsg_fvcore.so"))
    L.fc_fv_check.restype, L.fc_fv_check.argtypes = C.c_int, [_i32p] * 3 + [C.c_int] * 2
    L.fc_join_nodes.restype, L.fc_join_nodes.argtypes = C.c_int, [_i32p, _i32p, C.c_int] * 2 + [_i32p, C.c_int]
    L.fc_pair_bits_check.restype, L.fc_pair_bits_check.argtypes = C.c_int, [_i32p, _i32p, C.c_int, _i32p]
    return L


@pytest.mark.parametrize("name", list(fc.fv_check_cases()))
def test_fv_check_accepts_a_valid_csr_and_refuses_each_defect(core, name):
    ids, off, idx, n, null, want = fc.fv_check_cases()[name]
    if null:
        got = core.fc_fv_check(None, None, None, len(ids), n)
    else:
        got = core.fc_fv_check(_p(ids), _p(off), _p(idx), len(ids), n)
    assert got == want


@pytest.mark.parametrize("name", list(fc.id_sets()))
def test_join_nodes_equals_intersect1d_in_ranges_and_order(core, name):
    idA, idB = fc.id_sets()[name]
    offA, offB = fc.offsets(idA, 1), fc.offsets(idB, 2)
    want = fc.expected_join(idA, offA, idB, offB)
    cap = min(len(idA), len(idB))
    pairs = np.full((cap + 1, 4), -7, np.int32)
    count = core.fc_join_nodes(_p(idA), _p(offA), len(idA), _p(idB), _p(offB), len(idB), _p(pairs), cap)
    assert count == len(want) and np.array_equal(pairs[:count], want) and (pairs[count:] == -7).all()
    if name in ("identical", "one_each_same"):
        assert count == len(idA) > 0
    if name in ("disjoint", "a_empty", "b_empty", "one_each_different"):
        assert count == 0


@pytest.mark.parametrize("name", list(fc.pair_bits_cases()))
def test_pair_bits_check_on_exact_slack_short_negative_and_oversized_layouts(core, name):
    na, nb, pair_off, want = fc.pair_bits_cases()[name]
    assert len(pair_off) == len(na) + 1
    assert core.fc_pair_bits_check(_p(na), _p(nb), len(na), _p(pair_off)) == want
