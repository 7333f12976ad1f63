"""The host side of vsg_frame_pose_optimization (the argument check and the whole core of csrc/vsg_pose_opt.h) under
AddressSanitizer + UndefinedBehaviorSanitizer.  The core is built into a program of its own with both runtimes linked in
(tests/_posecore/pose_sanitized.cpp: nothing is loaded into an interpreter and nothing is preloaded), and that program
runs every scene of tests/pose_scenes.py plus the argument errors, each array a heap block of exactly its size.  Any
report fails the run (-fno-sanitize-recover, halt_on_error), and so does a result that differs from the unsanitised
build's by a bit."""
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import pose_hostcore as hc
import pose_scenes as ps

I32, F32, U8 = np.int32, np.float32, np.uint8
PC_DIR = Path(__file__).resolve().parent / "_posecore"


@pytest.fixture(scope="module")
def program():
    for rt in ("libasan.a", "libubsan.a"):
        p = subprocess.run(["gcc", "-print-file-name=" + rt], capture_output=True, text=True).stdout.strip()
        if not (p and os.path.sep in p and os.path.exists(p)):
            pytest.skip("gcc's %s not found" % rt)
    subprocess.check_call(["make", "-C", str(PC_DIR), "sanitized"], stdout=subprocess.DEVNULL)
    return PC_DIR / "pose_sanitized"


def _pad(b):
    return b + b"\0" * (-len(b) % 4)


def record(s, null_slots=False):
    hold = s["removed"] is not None
    head = np.array([s["n"], s["capacity"], s["nlevels"], 2 if hold else -1, 0 if s["u_right"] is None else 1,
                     1 if hold else 0, 1 if null_slots else 0, 0], I32)
    parts = [head, s["feat_slots"].astype(I32), s["world_pos"].astype(F32), s["kx"].astype(F32), s["ky"].astype(F32),
             s["octave"].astype(I32)]
    if s["u_right"] is not None:
        parts.append(s["u_right"].astype(F32))
    parts += [np.concatenate([s["q"], s["t"]]).astype(F32), np.array(s["cam"], F32),
              np.resize(s["inv_sigma2"], min(max(s["nlevels"], 0), 16)).astype(F32)]
    out = b"".join(np.ascontiguousarray(a).tobytes() for a in parts)
    if hold:
        out += _pad(s["removed"].astype(U8).tobytes())
    return out


def test_host_core_is_clean_and_right_under_asan_and_ubsan(program, tmp_path):
    cases = list(ps.scenes().values())
    base = ps.scenes()["edges_64"]
    bad = base["feat_slots"].copy()
    bad[np.flatnonzero(bad >= 0)[2]] = base["capacity"]
    errors = [dict(base, feat_slots=bad), dict(base, nlevels=17), dict(base, nlevels=0),
              dict(base, nlevels=int(base["octave"][base["feat_slots"] >= 0].max()))]
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
        n = base["n"] if s is None else s["n"]
        rc, ri = np.frombuffer(raw, I32, 1, at)[0], np.frombuffer(raw, I32, 4, at + 4)
        outlier = np.frombuffer(raw, I32, n, at + 20)
        chi2 = np.frombuffer(raw, F32, n, at + 20 + 4 * n)
        qt = np.frombuffer(raw, np.float64, 7, at + 20 + 8 * n)
        at += 20 + 8 * n + 56
        if k >= len(cases):
            assert rc == -6 and (outlier == 7).all() and (chi2 == -1).all()
            continue
        want = hc.run(s)
        assert rc == want["ret"] and ri.tolist()[:3] == [want["n_initial"], want["n_bad"], want["rounds_run"]]
        assert outlier.astype(U8).tobytes() == want["outlier"].tobytes() and chi2.tobytes() == want["chi2"].tobytes()
        assert qt.tobytes() == np.concatenate([want["q"], want["t"]]).tobytes()
    assert at == len(raw)
