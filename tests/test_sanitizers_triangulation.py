"""The loop of CreateNewMapPoints (vsg::new_points_loop and the argument check of visual_sgraphs_amd/csrc/vsg_triangulate.h)
under AddressSanitizer + UndefinedBehaviorSanitizer.  The core is built into a program of its own with both runtimes linked in
(tests/_triangulatecore/triangulate_sanitized.cpp: nothing is loaded into an interpreter and nothing is preloaded); that program
runs the directed scenes, the parity scene with a store, two edge scenes and records the argument check must refuse, each array
a heap block of exactly its size.  Any report fails the run (-fno-sanitize-recover, halt_on_error), and so does any output that
differs from the ctypes build of the same core."""
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import triangulation_hostcore as hc
import triangulation_scenes as ts

F32, I32, U8 = np.float32, np.int32, np.uint8
DIR = Path(__file__).resolve().parent / "_triangulatecore"
FIELDS = ("world_pos", "normal", "min_dist", "max_dist", "desc", "observed")


@pytest.fixture(scope="module")
def program():
    for rt in ("libasan.a", "libubsan.a"):
        p = subprocess.run(["gcc", "-print-file-name=" + rt], capture_output=True, text=True).stdout.strip()
        if not (p and os.path.sep in p and os.path.exists(p)):
            pytest.skip("gcc's %s not found" % rt)
    subprocess.check_call(["make", "-C", str(DIR), "sanitized"], stdout=subprocess.DEVNULL)
    return DIR / "triangulate_sanitized"


def _record(s, matches, store=None, free_slots=()):
    n1, n2 = len(s["k1"]), len(s["k2"])
    cap = 0 if store is None else len(store["observed"])
    parts = [np.array([n1, n2, s["nlevels"], cap, len(free_slots)], I32).tobytes(), hc.params_blob(s["P"]).tobytes()]
    for t in ("1", "2"):
        k = s["k" + t]
        parts += [np.ascontiguousarray(k["x"], F32).tobytes(), np.ascontiguousarray(k["y"], F32).tobytes(),
                  np.ascontiguousarray(s["ur" + t], F32).tobytes(), np.ascontiguousarray(s["stereo" + t], F32).tobytes(),
                  np.ascontiguousarray(k["octave"], I32).tobytes(), np.ascontiguousarray(s["d" + t], U8).tobytes(),
                  np.ascontiguousarray(s["sf" + t], F32).tobytes(), np.ascontiguousarray(s["sigma2_" + t], F32).tobytes()]
    parts += [np.ascontiguousarray(matches, I32).tobytes(), np.ascontiguousarray(free_slots, I32).tobytes()]
    if store is not None:
        parts += [np.ascontiguousarray(store[k]).tobytes() for k in FIELDS]
    return b"".join(parts)


def _expected(s, matches, store=None, free_slots=()):
    h = hc.loop(s, matches, store, np.asarray(free_slots, I32))
    parts = [I32(1).tobytes(), I32(h["n_created"]).tobytes(), h["reason"].tobytes(), h["source"].tobytes(), h["x3d"].tobytes(),
             h["new_slot"].tobytes()]
    if store is not None:
        parts += [np.ascontiguousarray(h["store"][k]).tobytes() for k in FIELDS]
    return b"".join(parts)


def test_host_core_is_clean_and_equal_to_the_ctypes_build_under_asan_and_ubsan(program, tmp_path):
    rng = np.random.default_rng(2)
    cap = 400
    store = dict(world_pos=rng.normal(size=(cap, 3)).astype(F32), normal=rng.normal(size=(cap, 3)).astype(F32),
                 min_dist=rng.random(cap).astype(F32), max_dist=rng.random(cap).astype(F32),
                 desc=rng.integers(0, 256, (cap, 32)).astype(U8), observed=np.full(cap, 7, U8))
    cases = [(s, s["matches"], store, [5]) for s, _, _ in ts.directed().values()]
    p = ts.parity(kf2_first=True)
    cases += [(p, p["matches"], None, ()), (p, p["matches"], store, rng.permutation(cap)[:120]),
              (p, p["matches"], store, rng.permutation(cap)[:cap])]
    for n in (1, 65):
        e = ts.edge(n)
        cases += [(e, ts.with_matches(e, w), store, np.arange(max(len(w) - 1, 0))) for w in ts.edge_sets(n).values()]
    records, want = [], []
    for s, m, st, free in cases:
        records.append(_record(s, m, st, free)), want.append(_expected(s, m, st, free))
    # what the check refuses never reaches the loop: a match past kf2, a free slot outside the store and one listed twice, an
    # octave past the tables
    bad = p["matches"].copy()
    bad[np.flatnonzero(bad >= 0)[0]] = len(p["k2"])
    short = dict(p, nlevels=3, sf1=p["sf1"][:3], sigma2_1=p["sigma2_1"][:3], sf2=p["sf2"][:3], sigma2_2=p["sigma2_2"][:3])
    for s, m, st, free in ((p, bad, store, [1]), (p, p["matches"], store, [1, cap]), (p, p["matches"], store, [3, 4, 3]),
                           (short, p["matches"], None, ())):
        records.append(_record(s, m, st, free)), want.append(I32(0).tobytes())
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(b"".join(records))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(program), str(src), str(dst)], capture_output=True, text=True, env=env, timeout=120)
    out = r.stdout + r.stderr
    assert "Sanitizer" not in out and "runtime error:" not in out, out[-4000:]
    assert r.returncode == 0, (r.returncode, out[-4000:])
    got, want = dst.read_bytes(), b"".join(want)
    assert len(got) == len(want) > 100000 and got == want
