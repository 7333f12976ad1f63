"""The host side of vsg_frame_optimize_sim3 (the argument check and the whole core of csrc/vsg_sim3_opt.h) under
AddressSanitizer + UndefinedBehaviorSanitizer.  The core is built into a program of its own with both runtimes linked in
(tests/_sim3optcore/sim3opt_sanitized.cpp: nothing is loaded into an interpreter and nothing is preloaded), and that
program runs every scene of tests/sim3opt_scenes.py plus the argument errors, each array a heap block of exactly its size.
Any report fails the run (-fno-sanitize-recover, halt_on_error), and so does a result that differs from the unsanitised
build's by a bit."""
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import sim3opt_hostcore as hc
import sim3opt_scenes as ss

I32, F32, U8, F64 = np.int32, np.float32, np.uint8, np.float64
DIR = Path(__file__).resolve().parent / "_sim3optcore"


@pytest.fixture(scope="module")
def program():
    for rt in ("libasan.a", "libubsan.a"):
        p = subprocess.run(["gcc", "-print-file-name=" + rt], capture_output=True, text=True).stdout.strip()
        if not (p and os.path.sep in p and os.path.exists(p)):
            pytest.skip("gcc's %s not found" % rt)
    subprocess.check_call(["make", "-C", str(DIR), "sanitized"], stdout=subprocess.DEVNULL)
    return DIR / "sim3opt_sanitized"


def record(s, null_slots=False):
    nl = min(max(int(s["nlevels"]), 0), 16)
    head = np.array([s["n1"], s["n2"], s["cap1"], s["cap2"], s["nlevels"], s["fix_scale"], s["all_points"],
                     1 if s["shared"] else 0, 1 if null_slots else 0, 0, 0, 0], I32)

    def pose(p):
        return np.concatenate([p["Rcw"], p["tcw"], [p["fx"], p["fy"], p["cx"], p["cy"]]]).astype(F32)
    parts = [head, s["slots1"].astype(I32), s["slots2"].astype(I32), s["idx2"].astype(I32), s["level2"].astype(I32),
             np.asarray(s["pos1"], F32)]
    if not s["shared"]:
        parts.append(np.asarray(s["pos2"], F32))
    parts += [s["kps1"]["x"].astype(F32), s["kps1"]["y"].astype(F32), s["kps1"]["octave"].astype(I32),
              s["kps2"]["x"].astype(F32), s["kps2"]["y"].astype(F32), s["kps2"]["octave"].astype(I32), pose(s["pose1"]),
              pose(s["pose2"]), np.resize(s["sig1"], nl).astype(F32), np.resize(s["sig2"], nl).astype(F32),
              np.array([s["th2"]], F32), np.concatenate([s["S12"][0], s["S12"][1], [s["S12"][2]]]).astype(F64)]
    return b"".join(np.ascontiguousarray(a).tobytes() for a in parts)


def test_host_core_is_clean_and_right_under_asan_and_ubsan(program, tmp_path):
    cases = list(ss.scenes().values())
    base = ss.scenes()["pairs_64"]
    cand = ss.candidates(base)
    bad1, bad2, badi = base["slots1"].copy(), base["slots2"].copy(), base["idx2"].copy()
    bad1[cand[2]], bad2[cand[2]], badi[cand[2]] = base["cap1"], base["cap2"], base["n2"]
    errors = [dict(base, slots1=bad1), dict(base, slots2=bad2), dict(base, idx2=badi), dict(base, nlevels=17),
              dict(base, nlevels=0), dict(base, nlevels=int(base["kps1"]["octave"][cand].max())),
              dict(base, th2=F32(0.0)), dict(base, th2=F32(np.nan))]
    recs = [record(s) for s in cases + errors] + [record(base, null_slots=True)]
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(b"".join(recs))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(program), str(src), str(dst)], capture_output=True, text=True, env=env, timeout=300)
    out = r.stdout + r.stderr
    assert "Sanitizer" not in out and "runtime error:" not in out, out[-4000:]
    assert r.returncode == 0, (r.returncode, out[-4000:])
    raw, at = dst.read_bytes(), 0
    for k, s in enumerate(cases + errors + [None]):
        n = base["n1"] if s is None else s["n1"]
        rc, cnt = np.frombuffer(raw, I32, 1, at)[0], np.frombuffer(raw, I32, 7, at + 4)
        state = np.frombuffer(raw, I32, n, at + 32)
        chi2 = np.frombuffer(raw, F64, 2 * n, at + 32 + 4 * n)
        S12 = raw[at + 32 + 20 * n:at + 32 + 20 * n + 64]
        at += 32 + 20 * n + 64
        if k >= len(cases):
            assert rc == -6 and (state == 9).all() and (chi2 == -1).all() and (cnt == 0).all()
            continue
        want = hc.run(s)
        assert rc == want["ret"] and cnt.tolist() == [want[c] for c in hc.COUNTERS]
        assert state.astype(U8).tobytes() == want["state"].tobytes() and chi2.tobytes() == want["chi2"].tobytes()
        assert S12 == want["S12_bytes"]
    assert at == len(raw)
