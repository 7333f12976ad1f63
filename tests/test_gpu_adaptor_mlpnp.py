"""vsg::MLPnPsolver of include/vsg_orb_adaptor.hpp driven as Tracking::Relocalization drives the solver (Tracking.cc:3735-3762:
SetRansacParameters(0.99, 10, 300, 6, 0.5, 5.991), then iterate(5, ...) until it returns true or bNoMore) from a C++ program
(tests/_adaptor_mlpnp), against the SEQUENTIAL restatement's sequence of returns (tests/mlpnp_reference.py) on one true and one
false candidate: every call's return value, bNoMore, nInliers and mnIterations exactly, vbInliers exactly, Tout within the
float32 rounding of two poses a few 1e-9 apart (tests/test_mlpnp_reference.py measures that)."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import mlpnp_reference as mr
import mlpnp_scenes as ms
from visual_sgraphs_amd import orb

ROOT = Path(__file__).resolve().parent.parent
ADAPTOR = ROOT / "tests" / "_adaptor_mlpnp"
F32, I32 = np.float32, np.int32
TOL_T32 = 1e-6  # one float32 ulp below 8 is 4.8e-7: the two sides round poses 4e-9 apart


def test_cpp_adaptor_compiles_and_fails_loudly_without_device():
    L = orb.load_library()
    subprocess.check_call(["make", "-C", str(ADAPTOR)], stdout=subprocess.DEVNULL)
    adaptor = (ROOT / "include" / "vsg_orb_adaptor.hpp").read_text()
    for name in ("class MLPnPsolver", "void SetRansacParameters(double probability = 0.99, int minInliers = 8",
                 "bool iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers, Matrix &Tout)"):
        assert name in adaptor, name
    if L.vsg_device_count() <= 0:
        r = subprocess.run([str(ADAPTOR / "mlpnp_check"), "/dev/null", "/dev/null"], capture_output=True, text=True)
        assert r.returncode == 3 and "no CPU fallback" in r.stdout


def run(s, tmp_path):
    subprocess.check_call(["make", "-C", str(ADAPTOR)], stdout=subprocess.DEVNULL)
    blob = lambda a, t: np.ascontiguousarray(a, t).tobytes()  # noqa: E731
    src, out = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(np.array([s["n_feat"], s["capacity"], len(s["sets"]), ms.NLEVELS], I32).tobytes() + blob(ms.CAM, F32) +
                    blob(ms.LEVEL_SIGMA2, F32) + blob(s["kx"], F32) + blob(s["ky"], F32) + blob(s["octave"], I32) +
                    blob(s["slots"], I32) + blob(s["world_pos"], F32) + blob(s["sets"], I32))
    r = subprocess.run([str(ADAPTOR / "mlpnp_check"), str(src), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
    raw = out.read_bytes()
    head = np.frombuffer(raw[:12], I32)
    calls, at = [], 12
    while True:
        rec = np.frombuffer(raw[at:at + 8], I32)
        if rec[0] == -1:
            nfl = int(rec[1])
            at += 8
            break
        calls.append(tuple(int(v) for v in np.frombuffer(raw[at:at + 16], I32)))
        at += 16
    flags = np.frombuffer(raw[at:at + nfl], np.uint8).astype(bool)
    T = np.frombuffer(raw[at + nfl:at + nfl + 64], F32).reshape(4, 4)
    return head, calls, flags, T


def reference(s):
    rp = mr.make_points(ms.CAM, s["kx"], s["ky"], s["octave"], s["world_pos"], s["slots"], ms.LEVEL_SIGMA2, ms.TH2)
    mi, mx = mr.ransac_parameters(0.99, 10, 300, 6, 0.5, s["n"])
    solver = mr.Solver(rp, s["sets"], mi, mx)
    calls = []
    while True:
        w = solver.iterate(5)
        calls.append((int(w["found"]), int(w["no_more"]), w["n_inliers"], solver.iterations))
        if w["found"] or w["no_more"]:
            return (s["n"], mi, mx), calls, w


@pytest.mark.gpu
@pytest.mark.parametrize("candidate", ("true", "false"))
def test_cpp_adaptor_equals_the_sequential_restatement(tmp_path, candidate):
    s = ms.make(ms.SEEDS[1] + 100, n=100, n_hyp=60, outliers=0.3 if candidate == "true" else 1.0)
    head, calls, flags, T = run(s, tmp_path)
    want_head, want_calls, w = reference(s)
    assert tuple(head) == want_head and calls == want_calls
    if candidate == "true":
        assert w["found"] and calls[-1][0] == 1
        fl = np.zeros(s["n_feat"], bool)
        fl[s["where"]] = w["inlier"]
        assert np.array_equal(flags, fl) and np.abs(T - w["T"]).max() <= TOL_T32
    else:
        assert len(calls) == 1 and calls[0] == (0, 1, 0, want_head[2])  # the first call walks all of mRansacMaxIts
        assert len(flags) == 0 and (T == np.eye(4)).all()
