"""The host side of vsg_mappoints_local_bundle_adjustment (the argument check, the lists and the whole core of
csrc/vsg_local_ba.h) under AddressSanitizer + UndefinedBehaviorSanitizer.  The core is built into a program of its own with
both runtimes linked in (tests/_localbacore/lba_sanitized.cpp: nothing is loaded into an interpreter and nothing is
preloaded), and that program runs every scene of tests/lba_scenes.py plus every argument error, each array a heap block of
exactly its size.  Any report fails the run (-fno-sanitize-recover, halt_on_error), and so does a result that differs from
the unsanitised build's by a bit."""
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import lba_hostcore as hc
import lba_scenes as ls
from test_lba_hostmath import error_cases

I32, F32, U8, F64 = np.int32, np.float32, np.uint8, np.float64
DIR = Path(__file__).resolve().parent / "_localbacore"
NULL_BITS = dict(slots=0, obs_off=1, obs_kf=2, obs_idx=3, kf_Tcw=4, kf_fixed=5, kf_cam=6, inv_level_sigma2=7, kf_Tcw_out=8,
                 erase=9, res=10)


@pytest.fixture(scope="module")
def program():
    for rt in ("libasan.a", "libubsan.a"):
        p = subprocess.run(["gcc", "-print-file-name=" + rt], capture_output=True, text=True).stdout.strip()
        if not (p and os.path.sep in p and os.path.exists(p)):
            pytest.skip("gcc's %s not found" % rt)
    subprocess.check_call(["make", "-C", str(DIR), "sanitized"], stdout=subprocess.DEVNULL)
    return DIR / "lba_sanitized"


def record(s, stop_flag=None, nleft=None, null=()):
    a = hc.marshal(s)
    K = a["K"]
    kf_off = np.zeros(K + 1, I32)
    kf_off[1:] = np.cumsum([len(f["x"]) for f in s["kfs"]])
    cat = lambda k, t: np.concatenate([np.asarray(f[k], t) for f in s["kfs"]]).astype(t)
    ur = np.concatenate([np.full(len(f["x"]), -1, F32) if f["ur"] is None else np.asarray(f["ur"], F32) for f in s["kfs"]])
    nl = min(max(int(s["nlevels"]), 0), 16)
    mask = sum(1 << NULL_BITS[n] for n in null)
    head = np.array([s["capacity"], a["P"], len(a["kf"]), K, s["nlevels"], s["iterations"], -1 if stop_flag is None else stop_flag,
                     mask, int(kf_off[-1]), len(a["off"]), a["E"], 0], I32)
    parts = [head, np.asarray(s["store_pos"], F32), a["slots"][:a["P"]], a["off"], a["kf"], a["idx"], kf_off, cat("x", F32),
             cat("y", F32), cat("octave", I32), ur, np.full(K, -1, I32) if nleft is None else np.asarray(nleft, I32), a["Tcw"],
             a["fixed"], a["cam"], np.resize(a["sig"], nl).astype(F32)]
    return b"".join(np.ascontiguousarray(p).tobytes() for p in parts), (a["K"], a["P"], a["E"], s["capacity"])


def test_host_core_is_clean_and_right_under_asan_and_ubsan(program, tmp_path):
    base, cases, many = error_cases()
    runs = [(s, {}) for s in ls.scenes().values()]
    for kw, _ in cases.values():
        over = {k: v for k, v in kw.items() if k not in ("null", "nleft")}
        runs.append((dict(base, **over), dict(null=kw.get("null", ()), nleft=kw.get("nleft"))))
    runs += [(many, {}), (base, dict(stop_flag=1)), (base, dict(stop_flag=0)), (dict(base, fixed=np.zeros(3, U8)), {}),
             (dict(base, slots=base["slots"][:0], obs_off=np.zeros(1, I32), obs_kf=base["obs_kf"][:0], obs_idx=base["obs_idx"][:0]), {})]
    recs = [record(s, **kw) for s, kw in runs]
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(b"".join(r[0] for r in recs))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(program), str(src), str(dst)], capture_output=True, text=True, env=env, timeout=300)
    out = r.stdout + r.stderr
    assert "Sanitizer" not in out and "runtime error:" not in out, out[-4000:]
    assert r.returncode == 0 and "OK %d" % len(runs) in out, (r.returncode, out[-4000:])
    raw, at = dst.read_bytes(), 0
    nres = len(bytes(hc.LocalBaResult()))
    for (s, kw), (_, (K, P, E, cap)) in zip(runs, recs):
        want = hc.run(s, **kw)
        take = lambda n: raw[at:at + n]
        assert np.frombuffer(take(4), I32)[0] == want["ret"]
        at += 4
        for blob, n in ((want["res_bytes"], nres), (want["kf_out"].tobytes(), 56 * K), (want["pos_out"].tobytes(), 12 * P),
                        (want["erase"].tobytes(), E), (want["chi2"].tobytes(), 8 * E), (want["store_pos"].tobytes(), 12 * cap)):
            assert raw[at:at + n] == blob[:n] and len(blob) >= n
            at += n
    assert at == len(raw)
