"""The host side of vsg_mappoints_local_bundle_adjustment_sgraph (the argument check, the lists and the whole core of
csrc/vsg_sgraph_ba.h) under AddressSanitizer + UndefinedBehaviorSanitizer.  The core is built into a program of its own with
both runtimes linked in (tests/_sgbacore/sgba_sanitized.cpp: nothing is loaded into an interpreter and nothing is
preloaded), and that program runs every scene of tests/sgba_scenes.py (the cap and the scene past it among them) plus every
argument error, each array a heap block of exactly its size.  Any report fails the run (-fno-sanitize-recover,
halt_on_error), and so does a result that differs from the unsanitised build's by a bit."""
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import sgba_hostcore as sh
import sgba_scenes as ss
from test_sanitizers_lba import record as visual_record
from test_sgba_hostmath import error_cases

I32, F32, U8, F64 = np.int32, np.float32, np.uint8, np.float64
DIR = Path(__file__).resolve().parent / "_sgbacore"
SEM_NULL_BITS = {k: i for i, k in enumerate(sh.SEM_IN + sh.SEM_OUT[:3])}


@pytest.fixture(scope="module")
def program():
    for rt in ("libasan.a", "libubsan.a"):
        p = subprocess.run(["gcc", "-print-file-name=" + rt], capture_output=True, text=True).stdout.strip()
        if not (p and os.path.sep in p and os.path.exists(p)):
            pytest.skip("gcc's %s not found" % rt)
    subprocess.check_call(["make", "-C", str(DIR), "sanitized"], stdout=subprocess.DEVNULL)
    return DIR / "sgba_sanitized"


def record(s, stop_flag=None, null=(), sem=None):
    q = dict(s["sem"], **(sem or {}))
    head, dims = visual_record(s, stop_flag=stop_flag, null=[n for n in null if n not in SEM_NULL_BITS])
    t = lambda k, ty: np.ascontiguousarray(q[k], ty).reshape(-1)
    Pl, R, NO = len(t("plane_eq", F64)) // 4, len(t("room_center", F64)) // 3, len(t("pl_obs_kf", I32))
    mask = sum(1 << SEM_NULL_BITS[n] for n in null if n in SEM_NULL_BITS)
    parts = [np.array([Pl, NO, R, len(t("pl_obs_off", I32)), mask, 0], I32), t("plane_eq", F64), t("pl_obs_off", I32), t("pl_obs_kf", I32),
             t("pl_obs_local", F64), t("pl_obs_G", F64), t("w_plane_kf", F64), t("w_plane_point", F64), t("room_center", F64),
             t("room_n_walls", I32), t("room_wall", I32)]
    return head + b"".join(p.tobytes() for p in parts), dims + (Pl, R, NO)


def test_host_core_is_clean_and_right_under_asan_and_ubsan(program, tmp_path):
    base, cases = error_cases()
    runs = [(s, {}) for s in ss.scenes().values()] + [(s, {}) for s in ss.big_scenes().values()] + [(ss.rows_771(), {})]
    for kw, _ in cases.values():
        over = {k: v for k, v in kw.items() if k not in ("null", "sem")}
        runs.append((dict(base, **over), dict(null=kw.get("null", ()), sem=kw.get("sem"))))
    runs += [(base, dict(stop_flag=1)), (base, dict(stop_flag=0)), (dict(base, fixed=np.zeros(4, U8)), {}),
             (dict(base, obs_off=np.zeros_like(base["obs_off"])), {})]
    recs = [record(s, **kw) for s, kw in runs]
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(b"".join(r[0] for r in recs))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(program), str(src), str(dst)], capture_output=True, text=True, env=env, timeout=600)
    out = r.stdout + r.stderr
    assert "Sanitizer" not in out and "runtime error:" not in out, out[-4000:]
    assert r.returncode == 0 and "OK %d" % len(runs) in out, (r.returncode, out[-4000:])
    raw, at = dst.read_bytes(), 0
    nres = len(bytes(sh.SGraphLocalBaResult()))
    for (s, kw), (_, (K, P, E, cap, Pl, R, NO)) in zip(runs, recs):
        want = sh.run(s, **kw)
        assert np.frombuffer(raw[at:at + 4], I32)[0] == want["ret"]
        at += 4
        for blob, n in ((want["res_bytes"], nres), (want["kf_out"].tobytes(), 56 * K), (want["pos_out"].tobytes(), 12 * P),
                        (want["erase"].tobytes(), E), (want["chi2"].tobytes(), 8 * E), (want["store_pos"].tobytes(), 12 * cap),
                        (want["plane_out"].tobytes(), 32 * Pl), (want["room_out"].tobytes(), 24 * R), (want["erase_plane"].tobytes(), NO),
                        (want["chi2_pk"].tobytes(), 8 * NO), (want["chi2_pp"].tobytes(), 8 * NO)):
            assert raw[at:at + n] == blob[:n] and len(blob) >= n
            at += n
    assert at == len(raw)
