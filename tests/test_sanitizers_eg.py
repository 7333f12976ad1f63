"""The host side of vsg_mappoints_optimize_essential_graph (the argument check, the lists, the whole core of
csrc/vsg_essential_graph.h with the blocked dense solve) under AddressSanitizer + UndefinedBehaviorSanitizer.  The core is
built into a program of its own with both runtimes linked in (tests/_egcore/eg_sanitized.cpp: nothing is loaded into an
interpreter and nothing is preloaded), and that program runs every scene of tests/eg_scenes.py, sizes at the solver's panel
edge, and every argument error, each array a heap block of exactly its size.  Any report fails the run
(-fno-sanitize-recover, halt_on_error), and so does a result that differs from the unsanitised build's by a bit."""
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import eg_hostcore as hc
import eg_scenes as es
from test_eg_hostmath import error_cases

I32, F32, U8, F64 = np.int32, np.float32, np.uint8, np.float64
DIR = Path(__file__).resolve().parent / "_egcore"
NULL_BITS = dict(Scw=0, nonc=1, has=2, fixed=3, ei=4, ej=5, el=6, slots=7, ref=8, kf_out=9, res=10, store=11)


@pytest.fixture(scope="module")
def program():
    for rt in ("libasan.a", "libubsan.a"):
        p = subprocess.run(["gcc", "-print-file-name=" + rt], capture_output=True, text=True).stdout.strip()
        if not (p and os.path.sep in p and os.path.exists(p)):
            pytest.skip("gcc's %s not found" % rt)
    subprocess.check_call(["make", "-C", str(DIR), "sanitized"], stdout=subprocess.DEVNULL)
    return DIR / "eg_sanitized"


def record(s, null=(), n_kf=None, n_edges=None, n_points=None):
    a = hc.marshal(s)
    K, E, P = a["Scw"].shape[0], a["ei"].size, a["slots"].size
    store = s.get("store_pos")
    cap = -1 if store is None else len(store)
    mask = sum(1 << NULL_BITS[n] for n in null)
    head = np.array([cap, K, E, P, s["fix_scale"], s["iterations"], mask, K if n_kf is None else n_kf,
                     E if n_edges is None else n_edges, P if n_points is None else n_points], I32)
    parts = [head, np.zeros(0, F32) if store is None else np.asarray(store, F32), a["Scw"], a["nonc"], a["has"], a["fixed"], a["ei"],
             a["ej"], a["el"], a["slots"], a["ref"]]
    blob = b""
    for part in parts:
        raw = np.ascontiguousarray(part).tobytes()
        blob += raw + b"\0" * (-len(raw) % 4)
    return blob, (K, E, P, max(cap, 0))


def test_host_core_is_clean_and_right_under_asan_and_ubsan(program, tmp_path):
    base, cases = error_cases()
    runs = [(s, {}) for s in es.scenes().values()]
    runs += [(es.sized(400 + n, n, covis=2), {}) for n in (1, 6, 7, 10)]
    runs.append((es.sized(430, 20, hub=(5, 60)), {}))
    for kw, _ in cases.values():
        run_kw = {k: v for k, v in kw.items() if k in ("null", "n_kf", "n_edges", "n_points")}
        runs.append((dict(base, **{k: v for k, v in kw.items() if k not in run_kw}), run_kw))
    runs.append((dict(base, ei=np.zeros(0, I32), ej=np.zeros(0, I32), eloop=np.zeros(0, U8)), {}))
    runs.append((dict(base, slots=np.zeros(0, I32), point_ref=np.zeros(0, I32), store_pos=None), {}))
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
    for (s, kw), (_, (K, E, P, cap)) in zip(runs, recs):
        want = hc.run(s, **kw)
        assert np.frombuffer(raw[at:at + 4], I32)[0] == want["ret"]
        at += 4
        store = b"" if want["store_pos"] is None else want["store_pos"].tobytes()
        for blob, n in ((want["res_bytes"], 64), (want["kf_Scw"].tobytes(), 64 * K), (want["world_pos"].tobytes(), 12 * P),
                        (want["chi2"].tobytes(), 8 * E), (store, 12 * cap)):
            assert raw[at:at + n] == blob[:n] and len(blob) >= n
            at += n
    assert at == len(raw)
