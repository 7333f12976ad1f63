"""The host side of vsg_mappoints_global_bundle_adjustment (the argument check, the lists, the whole core of
csrc/vsg_global_ba.h with the blocked reduced solve) under AddressSanitizer + UndefinedBehaviorSanitizer.  The core is built
into a program of its own with both runtimes linked in (tests/_gbacore/gba_sanitized.cpp: nothing is loaded into an
interpreter and nothing is preloaded), and that program runs every scene of tests/gba_scenes.py plus every argument error,
each array a heap block of exactly its size.  Any report fails the run (-fno-sanitize-recover, halt_on_error), and so does
a result that differs from the unsanitised build's by a bit."""
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import gba_hostcore as hc
import gba_scenes as gs
from test_gba_hostmath import error_cases

I32, F32, U8, F64 = np.int32, np.float32, np.uint8, np.float64
DIR = Path(__file__).resolve().parent / "_gbacore"
NULL_BITS = dict(slots=0, obs_off=1, obs_kf=2, obs_idx=3, kf_Tcw=4, kf_fixed=5, kf_cam=6, inv_level_sigma2=7, kf_Tcw_out=8,
                 included=9, res=10, world_pos_out=11)


@pytest.fixture(scope="module")
def program():
    for rt in ("libasan.a", "libubsan.a"):
        p = subprocess.run(["gcc", "-print-file-name=" + rt], capture_output=True, text=True).stdout.strip()
        if not (p and os.path.sep in p and os.path.exists(p)):
            pytest.skip("gcc's %s not found" % rt)
    subprocess.check_call(["make", "-C", str(DIR), "sanitized"], stdout=subprocess.DEVNULL)
    return DIR / "gba_sanitized"


def record(s, stop_flag=None, nleft=None, null=()):
    a = hc.marshal(s)
    K = a["K"]
    kf_off, kx, ky, oc, ur = hc.flat_features(s)
    nl = min(max(int(s["nlevels"]), 0), 16)
    mask = sum(1 << NULL_BITS[n] for n in null)
    head = np.array([s["capacity"], a["P"], len(a["kf"]), K, s["nlevels"], s["iterations"], -1 if stop_flag is None else stop_flag,
                     mask, int(kf_off[-1]), len(a["off"]), a["E"], s["robust"], s["write_store"], 0], I32)
    parts = [head, np.asarray(s["store_pos"], F32), a["slots"][:a["P"]], a["off"], a["kf"], a["idx"], kf_off, kx, ky, oc, ur,
             np.full(K, -1, I32) if nleft is None else np.asarray(nleft, I32), a["Tcw"], a["fixed"], a["cam"],
             np.resize(a["sig"], nl).astype(F32)]
    return b"".join(np.ascontiguousarray(p).tobytes() for p in parts), (a["K"], a["P"], a["E"], s["capacity"])


def test_host_core_is_clean_and_right_under_asan_and_ubsan(program, tmp_path):
    base, cases = error_cases()
    runs = [(s, {}) for s in gs.scenes().values()]
    for kw, _ in cases.values():
        over = {k: v for k, v in kw.items() if k not in ("null", "nleft")}
        runs.append((dict(base, **over), dict(null=kw.get("null", ()), nleft=kw.get("nleft"))))
    K = len(base["kfs"])
    runs += [(base, dict(stop_flag=1)), (base, dict(stop_flag=0)), (dict(base, fixed=np.zeros(K, U8)), {}),
             (dict(base, obs_off=np.zeros_like(base["obs_off"])), {}),
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
    nres = len(bytes(hc.GlobalBaResult()))
    for (s, kw), (_, (K, P, E, cap)) in zip(runs, recs):
        want = hc.run(s, **kw)
        assert np.frombuffer(raw[at:at + 4], I32)[0] == want["ret"]
        at += 4
        for blob, n in ((want["res_bytes"], nres), (want["kf_out"].tobytes(), 56 * K), (want["pos_out"].tobytes(), 12 * P),
                        (want["included"].tobytes(), P), (want["chi2"].tobytes(), 8 * E), (want["store_pos"].tobytes(), 12 * cap)):
            assert raw[at:at + n] == blob[:n] and len(blob) >= n
            at += n
    assert at == len(raw)
