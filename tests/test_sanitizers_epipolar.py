"""The epipolar predicate of SearchForTriangulation (vsg::epipolar_reason_pair of visual_sgraphs_amd/csrc/vsg_epipolar.h) under
AddressSanitizer + UndefinedBehaviorSanitizer.  The core is built into a program of its own with both runtimes linked in
(tests/_epipolarcore/epipolar_sanitized.cpp: nothing is loaded into an interpreter and nothing is preloaded), and that program
computes the reason codes of the parity scene's legs and of every directed edge case, each array a heap block of exactly its
size.  Any report fails the run (-fno-sanitize-recover, halt_on_error), and so does any code that differs from the
restatement."""
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import epipolar_scenes as es

F32 = np.float32
EC_DIR = Path(__file__).resolve().parent / "_epipolarcore"


@pytest.fixture(scope="module")
def program():
    for rt in ("libasan.a", "libubsan.a"):
        p = subprocess.run(["gcc", "-print-file-name=" + rt], capture_output=True, text=True).stdout.strip()
        if not (p and os.path.sep in p and os.path.exists(p)):
            pytest.skip("gcc's %s not found" % rt)
    subprocess.check_call(["make", "-C", str(EC_DIR), "sanitized"], stdout=subprocess.DEVNULL)
    return EC_DIR / "epipolar_sanitized"


def _record(x1, y1, ur1, x2, y2, ur2, octave2, F12, ep, sf, sigma2, only_stereo, coarse):
    n = len(x2)
    parts = [np.array([n, len(sf), only_stereo, coarse], np.int32)]
    parts += [np.ascontiguousarray(v, F32).reshape(n) for v in (x1, y1, ur1, x2, y2, ur2)]
    parts += [np.ascontiguousarray(octave2, np.int32).reshape(n), np.ascontiguousarray(F12, F32).reshape(9),
              np.ascontiguousarray(ep, F32).reshape(2), np.ascontiguousarray(sf, F32), np.ascontiguousarray(sigma2, F32)]
    return b"".join(p.tobytes() for p in parts)


def test_host_core_is_clean_and_equal_to_the_restatement_under_asan_and_ubsan(program, tmp_path):
    s = es.frames()
    records, want = [], []
    for name, (key, only_stereo, coarse, u1, u2) in es.LEGS.items():
        ref = es.leg_scene(s, name)
        ur1 = s["ur1"] if u1 else np.full(len(s["k1"]), -1, F32)
        ur2 = s["ur2"] if u2 else np.full(len(s["k2"]), -1, F32)
        i1, i2 = ref["i1"], ref["i2"]
        records.append(_record(s["k1"]["x"][i1], s["k1"]["y"][i1], ur1[i1], s["k2"]["x"][i2], s["k2"]["y"][i2], ur2[i2],
                               s["k2"]["octave"][i2], s[key], s["ep"], s["sf"], s["sigma2"], only_stereo, coarse))
        want.append(ref["reason"])
    sf = (F32(1.2) ** np.arange(8, dtype=F32)).astype(F32)
    sigma2 = (sf * sf).astype(F32)
    for c in es.directed_cases(sf, sigma2).values():
        records.append(_record(c["x1"], c["y1"], c["ur1"], c["x2"], c["y2"], c["ur2"], c["octave2"], c["F12"], c["ep"], sf, sigma2,
                               c["only_stereo"], c["coarse"]))
        want.append(c["reason"])
    records.append(_record(*[np.zeros(0, F32)] * 6, np.zeros(0, np.int32), np.zeros(9), np.zeros(2), sf, sigma2, 0, 0))  # n = 0
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(b"".join(records))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(program), str(src), str(dst)], capture_output=True, text=True, env=env, timeout=120)
    out = r.stdout + r.stderr
    assert "Sanitizer" not in out and "runtime error:" not in out, out[-4000:]
    assert r.returncode == 0, (r.returncode, out[-4000:])
    want = np.concatenate(want)
    got = np.frombuffer(dst.read_bytes(), np.uint8)
    assert len(got) == len(want) > 100000 and np.array_equal(got, want)
    assert set(got.tolist()) == {0, 1, 2, 3, 4}
