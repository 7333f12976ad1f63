"""MLPnPsolver's host core (vsg::mlpnp::ransac_host and the argument check of visual_sgraphs_amd/csrc/vsg_mlpnp.h) under
AddressSanitizer + UndefinedBehaviorSanitizer.  The core is built into a program of its own with both runtimes linked in
(tests/_mlpnpcore/mlpnp_sanitized.cpp: nothing is loaded into an interpreter and nothing is preloaded); that program runs the
seeded scenes (general and planar, first and resumed calls), the group scene whose records are refined, the smallest calls and
records the argument check must refuse, each array a heap block of exactly its size.  Any report fails the run
(-fno-sanitize-recover, halt_on_error), and so does any output that differs from the ctypes build of the same core."""
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import mlpnp_hostcore as hc
import mlpnp_scenes as ms

F32, I32, U8 = np.float32, np.int32, np.uint8
DIR = Path(__file__).resolve().parent / "_mlpnpcore"


@pytest.fixture(scope="module")
def program():
    for rt in ("libasan.a", "libubsan.a"):
        p = subprocess.run(["gcc", "-print-file-name=" + rt], capture_output=True, text=True).stdout.strip()
        if not (p and os.path.sep in p and os.path.exists(p)):
            pytest.skip("gcc's %s not found" % rt)
    subprocess.check_call(["make", "-C", str(DIR), "sanitized"], stdout=subprocess.DEVNULL)
    return DIR / "mlpnp_sanitized"


def _record(s, min_inliers, max_its, first, n_iterations, sets, want_hyp, slots=None, octave=None, nlevels=ms.NLEVELS, th2=ms.TH2,
            n_hyp=None, capacity=None):
    sm = np.ascontiguousarray(sets, I32).reshape(-1, 6)
    nh = len(sm) if n_hyp is None else n_hyp
    cap = s["capacity"] if capacity is None else capacity
    sl = np.asarray(s["slots"] if slots is None else slots, I32)
    oc = np.asarray(s["octave"] if octave is None else octave, I32)
    return b"".join([np.array([s["n_feat"], nh, cap, nlevels, min_inliers, max_its, first, n_iterations, int(want_hyp)], I32).tobytes(),
                     np.array([th2] + list(ms.CAM), F32).tobytes(), sl.tobytes(), oc.tobytes(),
                     np.ascontiguousarray(s["world_pos"], F32)[:cap].tobytes(), s["kx"].tobytes(), s["ky"].tobytes(),
                     ms.LEVEL_SIGMA2[:nlevels].tobytes() if nlevels <= ms.NLEVELS else np.resize(ms.LEVEL_SIGMA2, nlevels).tobytes(),
                     sm[:nh].tobytes() if nh <= len(sm) else np.resize(sm, (nh, 6)).tobytes()])


def _expected(s, min_inliers, max_its, first, n_iterations, sets, want_hyp):
    h = hc.ransac(s, ms.CAM, ms.LEVEL_SIGMA2, ms.TH2, min_inliers, max_its, first, n_iterations, sets, want_hyp)
    parts = [I32(1).tobytes(), h["inlier"].tobytes(), h["res"]["raw"]]
    if want_hyp and s["n"] >= min_inliers:
        parts += [h["hyp_inliers"].tobytes(), h["hyp_T"].tobytes()]
    elif want_hyp:
        parts += [np.zeros(len(np.reshape(sets, (-1, 6))), I32).tobytes(), np.zeros(12 * len(np.reshape(sets, (-1, 6)))).tobytes()]
    return b"".join(parts)


def test_host_core_is_clean_and_equal_to_the_ctypes_build_under_asan_and_ubsan(program, tmp_path):
    cases = []
    for kind in ("general", "plane0", "plane1"):
        for n in ms.SIZES:
            s = ms.make(ms.SEEDS[1] + n, n=n, kind=kind, n_hyp=45)
            mi, mx = hc.parameters(0.99, 10, 300, 6, 0.5, n)
            cases += [(s, mi, mx, 0, 5, s["sets"], True), (s, mi, mx, 3, 5, s["sets"], False), (s, n, 40, 40, 5, s["sets"], True)]
    g = ms.group_scene((8, 9, 10, 11, 12, 13, 14, 15, 63, 64, 65))
    cases += [(g, 8, 11, 0, 5, g["sets"], True), (g, 65, 11, 0, 5, g["sets"], True), (g, 66, 11, 0, 5, g["sets"], False)]
    small = ms.make(7, n=6, outliers=0.0, noise=0.0, n_hyp=1)
    cases += [(small, 6, 1, 0, 1, [[5, 3, 1, 0, 2, 4]], True), (small, 7, 1, 0, 1, [[0, 1, 2, 3, 4, 5]], True)]  # the second: N < min
    for n in (63, 65, 129):
        s = ms.make(200 + n, n=n, n_hyp=5)
        cases.append((s, 6, 5, 0, 5, s["sets"], True))
    records = [_record(*c) for c in cases]
    want = [_expected(*c) for c in cases]
    # what the check refuses never reaches the solver
    s = ms.make(ms.SEEDS[0], n=60, n_hyp=4)
    sm, used = s["sets"], np.flatnonzero(s["slots"] >= 0)

    def edit(a, i, v):
        a = np.array(a, copy=True)
        a.reshape(-1)[i] = v
        return a
    refused = [dict(slots=edit(s["slots"], used[9], s["capacity"])), dict(octave=edit(s["octave"], used[0], ms.NLEVELS)),
               dict(octave=edit(s["octave"], used[1], -1)), dict(sets=edit(sm, 5, 60)), dict(sets=edit(sm, 7, -2)),
               dict(sets=edit(sm, 2, sm[0, 0])), dict(n_hyp=0), dict(n_hyp=1025, max_its=1), dict(max_its=5), dict(first=2, n_iterations=3),
               dict(min_inliers=5), dict(nlevels=0), dict(nlevels=17), dict(th2=0.0), dict(th2=float("nan"))]
    for kw in refused:
        a = dict(s=s, min_inliers=10, max_its=4, first=0, n_iterations=4, sets=sm, want_hyp=True)
        a.update(kw)
        records.append(_record(**a)), want.append(I32(0).tobytes())
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(b"".join(records))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(program), str(src), str(dst)], capture_output=True, text=True, env=env, timeout=120)
    out = r.stdout + r.stderr
    assert "Sanitizer" not in out and "runtime error:" not in out, out[-4000:]
    assert r.returncode == 0, (r.returncode, out[-4000:])
    got, want = dst.read_bytes(), b"".join(want)
    assert len(got) == len(want) > 50000 and got == want
