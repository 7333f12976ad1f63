"""The FeatureVector argument checks of the vocabulary-node searches (vsg::fv_check, join_nodes, pair_bits_check of
visual_sgraphs_amd/csrc/vsg_fv.h) under AddressSanitizer + UndefinedBehaviorSanitizer.  The core is built into a program of its
own with both runtimes linked in (tests/_fvcore/fv_sanitized.cpp: nothing is loaded into an interpreter and nothing is
preloaded), and that program runs every case of tests/test_fv_args.py, each array a heap block of exactly its size.  Any report
fails the run (-fno-sanitize-recover, halt_on_error), and so does any result that differs from the expected one."""
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import fv_cases as fc

I32 = np.int32
FC_DIR = Path(__file__).resolve().parent / "_fvcore"


@pytest.fixture(scope="module")
def program():
    for rt in ("libasan.a", "libubsan.a"):
        p = subprocess.run(["gcc", "-print-file-name=" + rt], capture_output=True, text=True).stdout.strip()
        if not (p and os.path.sep in p and os.path.exists(p)):
            pytest.skip("gcc's %s not found" % rt)
    subprocess.check_call(["make", "-C", str(FC_DIR), "sanitized"], stdout=subprocess.DEVNULL)
    return FC_DIR / "fv_sanitized"


def _record(kind, a, b, c, d, *arrays):
    return b"".join(np.ascontiguousarray(x, I32).tobytes() for x in (np.array([kind, a, b, c, d]),) + arrays)


def test_host_core_is_clean_and_right_under_asan_and_ubsan(program, tmp_path):
    records, want = [], []
    for ids, off, idx, n, null, ok in fc.fv_check_cases().values():
        records.append(_record(0, len(ids), n, len(idx), int(null), ids, off, idx))
        want.append([ok])
    for name, (idA, idB) in fc.id_sets().items():
        offA, offB = fc.offsets(idA, 1), fc.offsets(idB, 2)
        records.append(_record(1, len(idA), len(idB), 0, 0, idA, offA, idB, offB))
        pairs = fc.expected_join(idA, offA, idB, offB)
        want.append(np.concatenate([[len(pairs)], pairs.reshape(-1)]))
    for na, nb, pair_off, ok in fc.pair_bits_cases().values():
        records.append(_record(2, len(na), 0, 0, 0, na, nb, pair_off))
        want.append([ok])
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(b"".join(records))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(program), str(src), str(dst)], capture_output=True, text=True, env=env, timeout=120)
    out = r.stdout + r.stderr
    assert "Sanitizer" not in out and "runtime error:" not in out, out[-4000:]
    assert r.returncode == 0, (r.returncode, out[-4000:])
    want = np.concatenate(want).astype(I32)
    got = np.frombuffer(dst.read_bytes(), I32)
    assert len(want) > 300 and np.array_equal(got, want)   # the random_300 join alone has dozens of shared nodes
