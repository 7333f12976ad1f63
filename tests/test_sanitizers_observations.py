"""The host side of vsg_mappoints_refresh_from_observations (vsg::obs_check of csrc/vsg_obs_args.h and
vsg::update_normal_and_depth of csrc/vsg_observations.h) under AddressSanitizer + UndefinedBehaviorSanitizer.  The core is
built into a program of its own with both runtimes linked in (tests/_obscore/obs_sanitized.cpp: nothing is loaded into an
interpreter and nothing is preloaded), and that program runs every case of tests/obs_cases.py, each array a heap block of
exactly its size.  Any report fails the run (-fno-sanitize-recover, halt_on_error), and so does a result that differs."""
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import obs_cases as oc
import observations_reference as obr

I32 = np.int32
OC_DIR = Path(__file__).resolve().parent / "_obscore"


@pytest.fixture(scope="module")
def program():
    for rt in ("libasan.a", "libubsan.a"):
        p = subprocess.run(["gcc", "-print-file-name=" + rt], capture_output=True, text=True).stdout.strip()
        if not (p and os.path.sep in p and os.path.exists(p)):
            pytest.skip("gcc's %s not found" % rt)
    subprocess.check_call(["make", "-C", str(OC_DIR), "sanitized"], stdout=subprocess.DEVNULL)
    return OC_DIR / "obs_sanitized"


def _bytes(*arrays):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)


def test_host_core_is_clean_and_right_under_asan_and_ubsan(program, tmp_path):
    records, want = [], []
    for name, (c, rc) in sorted(oc.cases().items()):
        head = np.array([0, len(c["slots"]), len(c["kf"]), len(c["kf_n"]), c["capacity"], c["nlevels"],
                         0 if c["use_bad"] else 1, 0], I32)
        records.append(_bytes(head, c["slots"].astype(I32), c["off"].astype(I32), c["kf"].astype(I32), c["idx"].astype(I32),
                              c["bad"].astype(I32), c["ref_pos"].astype(I32), c["kf_n"].astype(I32),
                              np.concatenate(c["oct"]).astype(I32)))
        want.append(np.array([rc], I32))
        if rc != oc.INVALID:
            want.append(oc.expected_good(c))
    records.append(_bytes(np.array([0, 0, 0, 0, 10, 8, 2, 0], I32), np.zeros(1, I32)))  # n == 0, every array NULL; off[1]
    want.append(np.array([oc.OK], I32))
    # the arithmetic on the valid case's lists, with a point that coincides with a camera centre (0 / 0)
    c = oc.base()
    rng = np.random.default_rng(3)
    n, n_kf = len(c["slots"]), len(c["kf_n"])
    P, Ow = rng.normal(0, 3, (n, 3)).astype(np.float32), rng.normal(0, 3, (n_kf, 3)).astype(np.float32)
    P[4] = Ow[3]
    sf = (np.float32(1.2) ** np.arange(8, dtype=np.float32)).astype(np.float32)
    lvl = np.array([c["oct"][c["kf"][c["off"][i] + c["ref_pos"][i]]][c["idx"][c["off"][i] + c["ref_pos"][i]]]
                    if c["off"][i + 1] > c["off"][i] else 0 for i in range(n)], I32)
    records.append(_bytes(np.array([1, n, len(c["kf"]), n_kf, 0, 8, 0, 0], I32), c["off"], c["kf"], c["ref_pos"], lvl, P, Ow, sf))
    nrm, mn, mx = np.zeros((n, 3), np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
    for i in range(n):
        o, e = c["off"][i], c["off"][i + 1]
        if e > o:
            nrm[i], mn[i], mx[i] = obr.update_normal_and_depth(P[i], Ow[c["kf"][o:e]], c["ref_pos"][i], lvl[i], sf, 8)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(b"".join(records))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(program), str(src), str(dst)], capture_output=True, text=True, env=env, timeout=120)
    out = r.stdout + r.stderr
    assert "Sanitizer" not in out and "runtime error:" not in out, out[-4000:]
    assert r.returncode == 0, (r.returncode, out[-4000:])
    got = np.frombuffer(dst.read_bytes(), I32)
    want = np.concatenate(want).astype(I32)
    assert len(want) > 60 and np.array_equal(got[:len(want)], want)
    f = got[len(want):].view(np.float32)
    assert len(f) == 5 * n
    g_nrm, g_mn, g_mx = f[:3 * n].reshape(n, 3), f[3 * n:4 * n], f[4 * n:]
    assert np.isnan(nrm[4]).all() and np.isnan(g_nrm[4]).all()   # 0 / 0 on both sides, then summed and divided
    ok = np.arange(n) != 4
    assert g_nrm[ok].tobytes() == nrm[ok].tobytes()
    assert g_mn.tobytes() == mn.tobytes() and g_mx.tobytes() == mx.tobytes()
