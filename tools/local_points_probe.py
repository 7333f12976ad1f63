#!/usr/bin/env python3
"""Warm latency of Tracking::SearchLocalPoints with the local map resident on the device, next to what a caller does
without it.  Runs on the GPU box, one process, the variants alternating call by call.

C2-sized data: a 1000-feature frame (640x480, TUM1 intrinsics) and local maps of 1000 / 2000 / 4000 points
(tests/frustum_reference.py's scenario; the frame's features sit where the in-view points project, with slightly changed
descriptors, so the search matches a real share).  Host clock around the blocking calls, straight through ctypes with
preallocated arrays on both sides:

  A   the caller-side loop: Frame::isInFrustum per map point on the host (tools/local_points_cpu.cpp, the kernel's own
      arithmetic compiled -O2, one thread) + the gather of descriptors + vsg_frame_search_by_projection
  A2  A again: the run's own A-vs-A spread
  B   vsg_frame_search_local_points, store resident, only the pose changes (a small rotation per call, the same for
      every variant)
  B5  B with 5 % of the slots updated (position, normal, distances, descriptor) before each call: a keyframe's churn

usage: local_points_probe.py latency [calls]   -> one JSON object (medians, 10-90 % spread, microseconds)
       local_points_probe.py trace             -> a few B calls at 4000 points, for rocprofv3 --kernel-trace --stats"""
import ctypes as C
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
import frustum_reference as fr  # noqa: E402
from visual_sgraphs_amd import orb  # noqa: E402

_f32p, _u8p, _i32p = (C.POINTER(t) for t in (C.c_float, C.c_uint8, C.c_int32))
FIELDS = ("world_pos", "normal", "min_dist", "max_dist", "desc", "observed")
TH, NNRATIO = 3.0, 0.8


def host_side():
    out = ROOT / "tools" / "_bin"
    out.mkdir(exist_ok=True)
    so = out / "liblocal_points_cpu.so"
    src = [ROOT / "tools" / "local_points_cpu.cpp", ROOT / "visual_sgraphs_amd" / "csrc" / "vsg_frustum.h",
           ROOT / "visual_sgraphs_amd" / "csrc" / "vsg_math.h"]
    if not so.exists() or any(f.stat().st_mtime > so.stat().st_mtime for f in src):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                               "-I", str(ROOT / "visual_sgraphs_amd" / "csrc"), "-o", str(so),
                               str(ROOT / "tools" / "local_points_cpu.cpp")])
    L = C.CDLL(str(so))
    L.lp_host_side.restype = None
    L.lp_host_side.argtypes = [C.POINTER(orb.FramePose), _f32p, C.c_float, C.c_int, _i32p, _f32p, _f32p, _f32p, _f32p,
                               _u8p, _u8p, _u8p, _f32p, _f32p, _f32p, _i32p, _f32p, _u8p, _u8p]
    return L


def p(a, t):
    return a.ctypes.data_as(t)


class Case:
    def __init__(self, n, nfeat=1000):
        rng = np.random.default_rng(n)
        self.n = n
        self.pose, self.bounds, f = fr.scenario(3, "tum1", n=n)
        self.f = {k: np.ascontiguousarray(v) for k, v in f.items()}
        ref = fr.is_in_frustum(self.pose, self.bounds, f["world_pos"], f["normal"], f["min_dist"], f["max_dist"])
        iv = np.flatnonzero(ref["in_view"])
        src = iv[rng.integers(0, len(iv), nfeat)]
        keys = np.zeros(nfeat, orb.KP_DTYPE)
        keys["x"] = ref["proj_x"][src] + rng.normal(0, 2.0, nfeat).astype(np.float32)
        keys["y"] = ref["proj_y"][src] + rng.normal(0, 2.0, nfeat).astype(np.float32)
        keys["octave"] = np.maximum(ref["scale_level"][src] - rng.integers(0, 2, nfeat), 0)
        desc = f["desc"][src].copy()
        desc[:, :2] ^= rng.integers(0, 256, (nfeat, 2), dtype=np.uint8)
        self.F = orb.Frame(nfeat + 1)
        self.F.upload(keys, desc, self.bounds)
        self.nfeat = nfeat
        self.mp = orb.MapPoints(n)
        self.slots = np.arange(n, dtype=np.int32)
        self.mp.update(self.slots, **{k: self.f[k] for k in FIELDS})
        self.sf = (np.float32(1.2) ** np.arange(8, dtype=np.float32)).astype(np.float32)
        self.b = np.array(self.bounds, np.float32)
        # outputs / staging, allocated once
        z = np.zeros
        self.in_view, self.px, self.py, self.pxr = z(n, np.uint8), z(n, np.float32), z(n, np.float32), z(n, np.float32)
        self.lvl, self.vc, self.qd, self.qo = z(n, np.int32), z(n, np.float32), z((n, 32), np.uint8), z(n, np.uint8)
        self.tb, self.tm, self.ntm = z(nfeat, np.uint8), z(nfeat, np.int32), C.c_int(0)
        self.churn = rng.choice(n, max(n // 20, 1), replace=False).astype(np.int32)

    def pose_at(self, k):
        """The scenario's camera turned by a small angle about its y axis: the pose of call k."""
        a = 0.002 * (k % 50)
        Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        R = (Ry @ self.pose["Rcw"].astype(np.float64)).astype(np.float32)
        t = (Ry @ self.pose["tcw"].astype(np.float64)).astype(np.float32)
        q = fr.make_pose(R, t, self.pose["fx"], self.pose["fy"], self.pose["cx"], self.pose["cy"], self.pose["mbf"])
        return orb.FramePose.make(**q)

    def reset(self):
        self.tb[:] = 0
        self.tm[:] = -1

    def A(self, L, H, P):
        f = self.f
        H.lp_host_side(C.byref(P), p(self.b, _f32p), 0.5, self.n, p(self.slots, _i32p), p(f["world_pos"], _f32p),
                       p(f["normal"], _f32p), p(f["min_dist"], _f32p), p(f["max_dist"], _f32p), p(f["desc"], _u8p),
                       p(f["observed"], _u8p), p(self.in_view, _u8p), p(self.px, _f32p), p(self.py, _f32p),
                       p(self.pxr, _f32p), p(self.lvl, _i32p), p(self.vc, _f32p), p(self.qd, _u8p), p(self.qo, _u8p))
        return L.vsg_frame_search_by_projection(
            self.F.handle, self.n, p(self.qd, _u8p), p(self.qo, _u8p), p(self.in_view, _u8p), p(self.px, _f32p),
            p(self.py, _f32p), p(self.pxr, _f32p), p(self.lvl, _i32p), p(self.vc, _f32p), None, None, None, None, None, TH,
            NNRATIO, p(self.sf, _f32p), 8, None, None, p(self.tb, _u8p), p(self.tm, _i32p))

    def B(self, L, P):
        return L.vsg_frame_search_local_points(
            self.F.handle, self.mp.handle, self.n, p(self.slots, _i32p), None, C.byref(P), 0.5, TH, NNRATIO, 0, 0.0,
            p(self.sf, _f32p), 8, p(self.tb, _u8p), p(self.tm, _i32p), p(self.in_view, _u8p), p(self.px, _f32p),
            p(self.py, _f32p), C.byref(self.ntm))

    def update5(self, L):
        f, c = self.f, self.churn
        return L.vsg_mappoints_update(self.mp.handle, len(c), p(c, _i32p), p(self.u_pos, _f32p), p(self.u_nrm, _f32p),
                                      p(self.u_min, _f32p), p(self.u_max, _f32p), p(self.u_desc, _u8p), None)

    def stage_churn(self):
        f, c = self.f, self.churn
        self.u_pos, self.u_nrm = np.ascontiguousarray(f["world_pos"][c]), np.ascontiguousarray(f["normal"][c])
        self.u_min, self.u_max = np.ascontiguousarray(f["min_dist"][c]), np.ascontiguousarray(f["max_dist"][c])
        self.u_desc = np.ascontiguousarray(f["desc"][c])


def stats(us):
    a = np.sort(np.asarray(us))
    return {"median_us": round(float(np.median(a)), 1), "p10_us": round(float(a[int(0.1 * len(a))]), 1),
            "p90_us": round(float(a[int(0.9 * len(a))]), 1)}


def latency(calls):
    L, H = orb.load_library(), host_side()
    out = {"calls": calls, "features": 1000, "th": TH, "sizes": {}}
    for n in (1000, 2000, 4000):
        c = Case(n)
        c.stage_churn()
        t = {k: [] for k in ("A", "A2", "B", "B5")}
        nm = {}
        for k in range(calls + 20):
            P = c.pose_at(k)
            for name in ("A", "B", "A2", "B5"):
                c.reset()
                t0 = time.perf_counter()
                if name == "B5":
                    rc = c.update5(L)
                    assert rc == 0
                r = c.A(L, H, P) if name[0] == "A" else c.B(L, P)
                dt = (time.perf_counter() - t0) * 1e6
                assert r >= 0, (name, r)
                nm[name] = (r, c.tm.copy())
                if k >= 20:
                    t[name].append(dt)
            # the variants compute the same thing (the churn rewrites the values the slots hold)
            assert nm["A"][0] == nm["B"][0] == nm["B5"][0] and np.array_equal(nm["A"][1], nm["B"][1])
        res = {k: stats(v) for k, v in t.items()}
        res["nmatches_last"], res["n_to_match_last"] = int(nm["B"][0]), int(c.ntm.value)
        res["a_vs_a_median_gap_us"] = round(abs(res["A"]["median_us"] - res["A2"]["median_us"]), 1)
        out["sizes"][str(n)] = res
    print(json.dumps(out))


def trace():
    L = orb.load_library()
    c = Case(4000)
    for k in range(10):
        c.reset()
        assert c.B(L, c.pose_at(k)) >= 0
    print({"n": 4000, "nmatches": int((c.tm >= 0).sum()), "n_to_match": c.ntm.value})


if __name__ == "__main__":
    if sys.argv[1] == "latency":
        latency(int(sys.argv[2]) if len(sys.argv) > 2 else 200)
    else:
        trace()
