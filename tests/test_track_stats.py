"""The statistics loop that ends Tracking::TrackLocalMap (Tracking.cc:3074-3095) as vsg_frame_track_local_map runs it
(csrc/vsg_track_stats.h, built for the host in tests/_trackstatscore) against a numpy restatement of those lines: the
returned mnMatchesInliers, the slots after the STEREO drop, and the outlier flags left alone.  The same cases run once more
through a program of its own built with AddressSanitizer + UBSan (both runtimes linked in; nothing is preloaded)."""
import ctypes as C
import functools
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

I32, U8 = np.int32, np.uint8
DIR = Path(__file__).resolve().parent / "_trackstatscore"


@functools.lru_cache(maxsize=None)
def lib():
    subprocess.check_call(["make", "-C", str(DIR)], stdout=subprocess.DEVNULL)
    L = C.CDLL(str(DIR / "libvsg_trackstatscore.so"))
    L.trackstats_case.restype = C.c_int
    L.trackstats_case.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    return L


def restated(fs, outlier, observed, only_tracking, drop_outliers):
    """:3074-3095 line by line; observed[i] = mvpMapPoints[i]->Observations() > 0."""
    fs = fs.copy()
    inliers = 0
    for i in range(len(fs)):
        if fs[i] >= 0:  # :3079
            if not outlier[i]:  # :3081
                if not only_tracking:  # :3084
                    if observed[i]:  # :3086
                        inliers += 1
                else:
                    inliers += 1  # :3090
            elif drop_outliers:  # :3092
                fs[i] = -1
    return inliers, fs


def run(fs, outlier, observed, only_tracking, drop_outliers):
    got = np.ascontiguousarray(fs, I32).copy()
    out, obs = np.ascontiguousarray(outlier, U8).copy(), np.ascontiguousarray(observed, U8).copy()
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
    ret = lib().trackstats_case(len(got), p(got), p(out), p(obs), int(only_tracking), int(drop_outliers))
    assert out.tobytes() == np.ascontiguousarray(outlier, U8).tobytes()  # :3093 drops the point, not the flag
    return ret, got


def random_arrays(seed):
    rng = np.random.default_rng(seed)
    nf = int(rng.integers(0, 1200))
    p_slot, p_out, p_obs = rng.choice([0.0, 0.3, 0.9, 1.0]), rng.choice([0.0, 0.2, 1.0]), rng.choice([0.0, 0.5, 1.0])
    fs = np.where(rng.random(nf) < p_slot, rng.integers(0, 6000, nf), rng.choice([-1, -7], nf)).astype(I32)
    # flags as the solve leaves them (0 / 1) and, for features without a slot, whatever the caller's storage held
    outlier = np.where(fs >= 0, rng.random(nf) < p_out, rng.integers(0, 256, nf)).astype(U8)
    observed = np.where(rng.random(nf) < p_obs, rng.choice([1, 3], nf), 0).astype(U8)
    return fs, outlier, observed


def directed():
    n = 64
    some = np.where(np.arange(n) % 3 == 0, np.arange(n) + 100, -1).astype(I32)
    return {
        "no_slot_at_all": (np.full(n, -1, I32), np.ones(n, U8), np.ones(n, U8)),
        "all_outliers": (some, np.ones(n, U8), np.ones(n, U8)),
        "no_outliers_none_observed": (some, np.zeros(n, U8), np.zeros(n, U8)),
        "slot_zero_counts": (np.zeros(n, I32), np.zeros(n, U8), np.ones(n, U8)),
        "no_features": (np.zeros(0, I32), np.zeros(0, U8), np.zeros(0, U8)),
    }


def all_cases():
    cases = [random_arrays(seed) for seed in range(300)] + list(directed().values())
    return [(a, ot, dr) for a in cases for ot in (0, 1) for dr in (0, 1)]


@pytest.mark.parametrize("only_tracking", [0, 1])
@pytest.mark.parametrize("drop_outliers", [0, 1])
def test_random_arrays_equal_the_restated_loop(only_tracking, drop_outliers):
    dropped = counted = 0
    for seed in range(300):
        fs, outlier, observed = random_arrays(seed)
        want_n, want_fs = restated(fs, outlier, observed, only_tracking, drop_outliers)
        got_n, got_fs = run(fs, outlier, observed, only_tracking, drop_outliers)
        assert got_n == want_n and got_fs.tobytes() == want_fs.tobytes(), seed
        dropped += int((want_fs != fs).sum())
        counted += want_n
    assert counted > 1000 and (dropped > 1000) == bool(drop_outliers)


@pytest.mark.parametrize("name", sorted(directed()))
def test_directed_arrays(name):
    fs, outlier, observed = directed()[name]
    for ot in (0, 1):
        for dr in (0, 1):
            want_n, want_fs = restated(fs, outlier, observed, ot, dr)
            got_n, got_fs = run(fs, outlier, observed, ot, dr)
            assert got_n == want_n and got_fs.tobytes() == want_fs.tobytes(), (ot, dr)
    n_slot = int((fs >= 0).sum())
    if name == "no_slot_at_all":
        assert run(fs, outlier, observed, 1, 1)[0] == 0 and (run(fs, outlier, observed, 1, 1)[1] == -1).all()
    if name == "all_outliers":
        assert run(fs, outlier, observed, 1, 0)[0] == 0 and (run(fs, outlier, observed, 1, 0)[1] == fs).all()
        assert run(fs, outlier, observed, 1, 1)[0] == 0 and (run(fs, outlier, observed, 1, 1)[1] == -1).all()
    if name == "no_outliers_none_observed":
        assert run(fs, outlier, observed, 0, 1)[0] == 0 and run(fs, outlier, observed, 1, 1)[0] == n_slot
    if name == "slot_zero_counts":
        assert run(fs, outlier, observed, 0, 0)[0] == len(fs)


@pytest.fixture(scope="module")
def program():
    for rt in ("libasan.a", "libubsan.a"):
        p = subprocess.run(["gcc", "-print-file-name=" + rt], capture_output=True, text=True).stdout.strip()
        if not (p and os.path.sep in p and os.path.exists(p)):
            pytest.skip("gcc's %s not found" % rt)
    subprocess.check_call(["make", "-C", str(DIR), "sanitized"], stdout=subprocess.DEVNULL)
    return DIR / "stats_sanitized"


def test_the_loop_is_clean_and_right_under_asan_and_ubsan(program, tmp_path):
    def pad(b):
        return b + b"\0" * (-len(b) % 4)
    cases = all_cases()
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(b"".join(np.array([len(fs), ot, dr, 0], I32).tobytes() + fs.tobytes() + pad(o.tobytes()) +
                             pad(ob.tobytes()) for (fs, o, ob), ot, dr in cases))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(program), str(src), str(dst)], capture_output=True, text=True, env=env, timeout=120)
    out = r.stdout + r.stderr
    assert "Sanitizer" not in out and "runtime error:" not in out, out[-4000:]
    assert r.returncode == 0, (r.returncode, out[-4000:])
    raw, at = dst.read_bytes(), 0
    for (fs, o, ob), ot, dr in cases:
        nf = len(fs)
        want_n, want_fs = restated(fs, o, ob, ot, dr)
        assert np.frombuffer(raw, I32, 1, at)[0] == want_n
        assert np.frombuffer(raw, I32, nf, at + 4).tobytes() == want_fs.tobytes()
        assert np.frombuffer(raw, I32, nf, at + 4 + 4 * nf).astype(U8).tobytes() == o.tobytes()
        at += 4 + 8 * nf
    assert at == len(raw)
