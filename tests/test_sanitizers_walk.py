"""The round form of the ordered walks (csrc/vsg_walks_dev.h) and their definition (csrc/vsg_walks.h) under
AddressSanitizer + UndefinedBehaviorSanitizer.  Both are built into a program of its own with both runtimes linked in
(tests/_walkcore/walk_sanitized.cpp: nothing is loaded into an interpreter and nothing is preloaded), and that program
walks the cases of tests/walk_cases.py, each array a heap block of exactly its size.  Any report fails the run
(-fno-sanitize-recover, halt_on_error), and so does a result that differs from the definition's or from the unsanitised
build's."""
import os
import subprocess

import numpy as np
import pytest

import walk_cases as wc

I32 = np.int32


@pytest.fixture(scope="module")
def program():
    for rt in ("libasan.a", "libubsan.a"):
        p = subprocess.run(["gcc", "-print-file-name=" + rt], capture_output=True, text=True).stdout.strip()
        if not (p and os.path.sep in p and os.path.exists(p)):
            pytest.skip("gcc's %s not found" % rt)
    subprocess.check_call(["make", "-C", str(wc.DIR), "sanitized"], stdout=subprocess.DEVNULL)
    return wc.DIR / "walk_sanitized"


def test_walks_are_clean_and_right_under_asan_and_ubsan(program, tmp_path):
    cases = list(wc.random_cases()) + list(wc.directed().values())
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(b"".join(wc.record(c) for c in cases))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(program), str(src), str(dst)], capture_output=True, text=True, env=env, timeout=300)
    out = r.stdout + r.stderr
    assert "Sanitizer" not in out and "runtime error:" not in out, out[-4000:]
    assert r.returncode == 0, (r.returncode, out[-4000:])
    raw, at = dst.read_bytes(), 0
    for k, c in enumerate(cases):
        nf = c["nf"]
        differs, info = np.frombuffer(raw, I32, 1, at)[0], np.frombuffer(raw, I32, 34, at + 4)
        tm, tb = np.frombuffer(raw, I32, nf, at + 140), np.frombuffer(raw, I32, nf, at + 140 + 4 * nf)
        edges = np.frombuffer(raw, I32, 2 * nf, at + 140 + 8 * nf)
        at += 140 + 16 * nf
        assert differs == 0, (k, differs)
        if k % 50 == 0 or k >= wc.N_RANDOM:  # the unsanitised build's bits, on a sample and on every directed case
            _, d = wc.run(c)
            assert info.tobytes() == d["info"].tobytes() and tm.tobytes() == d["tm"].tobytes()
            assert tb.astype(np.uint8).tobytes() == d["tb"].tobytes()
            assert edges[:d["n_edges"]].tobytes() == d["edge_feat"].tobytes()
            assert edges[nf:nf + d["n_edges"]].tobytes() == d["edge_slot"].tobytes()
    assert at == len(raw)
