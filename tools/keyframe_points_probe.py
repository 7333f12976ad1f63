#!/usr/bin/env python3
"""Warm latency of Fuse(pKF, vpMapPoints, th) with the map points resident on the device, next to what a caller does
without them.  Runs on the GPU box; every run is a fresh child process, the variants alternating call by call inside it.

A resident 1000-feature KeyFrame (640x480, TUM1 intrinsics) and 500 / 1000 / 2000 candidate map points, a tenth of them
flagged isBad() / IsInKeyFrame(pKF).  The points lie in front of the camera with normals along their viewing rays; the
KeyFrame's features sit where a subset projects, with slightly changed descriptors, so the search fuses a real share.
Host clock around the blocking calls, straight through ctypes with preallocated arrays on both sides:

  A   the caller-side path: the per-point loop of ORBmatcher.cc:1194-1241 on the host (tools/keyframe_points_cpu.cpp, the
      kernel's own arithmetic compiled -O2, one thread) + the gather of descriptors + vsg_frame_fuse
  A2  A again: the run's own A-vs-A spread
  B   vsg_frame_fuse_points: store resident, only the pose changes (a small rotation per call, the same for every
      variant: LocalMapping::SearchInNeighbors fuses one candidate list into 20-30 neighbours, one pose each)

usage: keyframe_points_probe.py [calls] [out.json]  -> runs the child, writes the record (default
                                                       profiles/keyframe_points_latency.json)
       keyframe_points_probe.py child [calls]       -> one JSON object on stdout (medians, 10-90 % range, microseconds)"""
import ctypes as C
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

_f32p, _u8p, _i32p = (C.POINTER(t) for t in (C.c_float, C.c_uint8, C.c_int32))
TH, NFEAT = 3.0, 1000


def host_side(orb):
    out = ROOT / "tools" / "_bin"
    out.mkdir(exist_ok=True)
    so = out / "libkeyframe_points_cpu.so"
    csrc = ROOT / "visual_sgraphs_amd" / "csrc"
    src = [ROOT / "tools" / "keyframe_points_cpu.cpp", csrc / "vsg_project.h", csrc / "vsg_frustum.h", csrc / "vsg_math.h"]
    if not so.exists() or any(f.stat().st_mtime > so.stat().st_mtime for f in src):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", str(csrc), "-o", str(so),
                               str(src[0])])
    L = C.CDLL(str(so))
    L.kp_host_side.argtypes = [C.POINTER(orb.FramePose), _f32p, C.c_int, _u8p, _f32p, _f32p, _f32p, _f32p, _u8p, C.c_float,
                               _f32p, _i32p, _u8p, _f32p, _f32p, _f32p, _f32p, _i32p]
    return L


def p(a, t):
    return a.ctypes.data_as(t)


class Case:
    def __init__(self, orb, fr, n):
        rng = np.random.default_rng(n)
        self.n = n
        self.pose = fr.scenario(3, "tum1", n=1)[0]
        self.bounds = (0.0, 0.0, 640.0, 480.0)
        po = self.pose
        R, t = po["Rcw"].astype(np.float64), po["tcw"].astype(np.float64)
        # n points in front of the camera, a tenth of them outside the image
        px, py, z = rng.uniform(-40, 680, n), rng.uniform(-30, 510, n), rng.uniform(1, 8, n)
        Pc = np.stack([(px - po["cx"]) / po["fx"] * z, (py - po["cy"]) / po["fy"] * z, z], 1)
        self.pos = np.ascontiguousarray(((Pc - t) @ R).astype(np.float32))
        PO = self.pos.astype(np.float64) - po["Ow"]
        dist = np.linalg.norm(PO, axis=1)
        self.normal = np.ascontiguousarray((PO / dist[:, None]).astype(np.float32))
        oct_of = rng.integers(0, 8, n)
        self.max_dist = (dist * 1.2 ** (oct_of - 0.5)).astype(np.float32)  # the predicted level is the feature's octave
        self.min_dist = (self.max_dist / np.float32(1.2) ** np.float32(7)).astype(np.float32)
        self.desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        self.skip = (rng.random(n) < 0.1).astype(np.uint8)
        src = rng.integers(0, n, NFEAT)
        keys = np.zeros(NFEAT, orb.KP_DTYPE)
        keys["x"], keys["y"] = px[src] + rng.normal(0, 0.7, NFEAT), py[src] + rng.normal(0, 0.7, NFEAT)
        keys["octave"], keys["angle"] = oct_of[src], rng.uniform(0, 360, NFEAT)
        d = self.desc[src].copy()
        d[:, :2] ^= rng.integers(0, 256, (NFEAT, 2), dtype=np.uint8)
        self.F = orb.Frame(NFEAT + 1)
        self.F.upload(keys, d, self.bounds)
        self.slots = np.arange(n, dtype=np.int32)
        self.mp = orb.MapPoints(n)
        self.mp.update(self.slots, world_pos=self.pos, normal=self.normal, min_dist=self.min_dist, max_dist=self.max_dist,
                       desc=self.desc)
        self.sf = (np.float32(1.2) ** np.arange(8, dtype=np.float32)).astype(np.float32)
        self.inv2 = (np.float32(1) / (self.sf * self.sf)).astype(np.float32)
        self.b = np.array(self.bounds, np.float32)
        z_ = np.zeros
        self.index, self.qd = z_(n, np.int32), z_((n, 32), np.uint8)
        self.u, self.v, self.ur, self.rad, self.lvl = (z_(n, np.float32), z_(n, np.float32), z_(n, np.float32),
                                                       z_(n, np.float32), z_(n, np.int32))
        self.bi, self.bd = z_(n, np.int32), z_(n, np.int32)
        self.fr, self.orb = fr, orb
        self.nproj = 0

    def pose_at(self, k):
        """The camera turned by a small angle about its y axis: the pose of call k."""
        a = 0.002 * (k % 50)
        Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        po = self.pose
        R = (Ry @ po["Rcw"].astype(np.float64)).astype(np.float32)
        t = (Ry @ po["tcw"].astype(np.float64)).astype(np.float32)
        return self.orb.FramePose.make(**self.fr.make_pose(R, t, po["fx"], po["fy"], po["cx"], po["cy"], po["mbf"]))

    def A(self, L, H, P):
        m = H.kp_host_side(C.byref(P), p(self.b, _f32p), self.n, p(self.skip, _u8p), p(self.pos, _f32p), p(self.normal, _f32p),
                           p(self.min_dist, _f32p), p(self.max_dist, _f32p), p(self.desc, _u8p), TH, p(self.sf, _f32p),
                           p(self.index, _i32p), p(self.qd, _u8p), p(self.u, _f32p), p(self.v, _f32p), p(self.ur, _f32p),
                           p(self.rad, _f32p), p(self.lvl, _i32p))
        self.nproj = m
        r = L.vsg_frame_fuse(self.F.handle, m, p(self.qd, _u8p), p(self.u, _f32p), p(self.v, _f32p), p(self.ur, _f32p),
                             p(self.rad, _f32p), p(self.lvl, _i32p), 0, p(self.inv2, _f32p), 8, p(self.bi, _i32p),
                             p(self.bd, _i32p))
        bi, bd = np.full(self.n, -1, np.int32), np.full(self.n, 256, np.int32)  # compacted entries -> queries
        bi[self.index[:m]], bd[self.index[:m]] = self.bi[:m], self.bd[:m]
        return r, bi, bd

    def B(self, L, P):
        r = L.vsg_frame_fuse_points(self.F.handle, self.mp.handle, self.n, p(self.slots, _i32p), p(self.skip, _u8p), C.byref(P),
                                    TH, p(self.sf, _f32p), p(self.inv2, _f32p), 8, p(self.bi, _i32p), p(self.bd, _i32p), None,
                                    None, None, None, None)
        return r, self.bi.copy(), self.bd.copy()


def stats(us):
    a = np.sort(np.asarray(us))
    return {"median_us": round(float(np.median(a)), 1), "p10_us": round(float(a[int(0.1 * len(a))]), 1),
            "p90_us": round(float(a[int(0.9 * len(a))]), 1)}


def child(calls):
    import frustum_reference as fr
    from visual_sgraphs_amd import orb
    L, H = orb.load_library(), host_side(orb)
    out = {"calls": calls, "features": NFEAT, "th": TH, "sizes": {}}
    for n in (500, 1000, 2000):
        c = Case(orb, fr, n)
        t = {k: [] for k in ("A", "A2", "B")}
        res_of = {}
        for k in range(calls + 20):
            P = c.pose_at(k)
            for name in ("A", "B", "A2"):
                # the scatter of A's compacted results back to the queries is outside the clock: the walk that follows reads
                # either layout
                t0 = time.perf_counter()
                got = c.A(L, H, P) if name[0] == "A" else c.B(L, P)
                dt = (time.perf_counter() - t0) * 1e6
                assert got[0] >= 0, (name, got[0])
                res_of[name] = got
                if k >= 20:
                    t[name].append(dt)
            a, b = res_of["A"], res_of["B"]  # the variants compute the same thing
            assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
        res = {k: stats(v) for k, v in t.items()}
        res["projected_last"], res["fused_last"] = int(c.nproj), int(res_of["B"][0])
        res["a_vs_a_median_gap_us"] = round(abs(res["A"]["median_us"] - res["A2"]["median_us"]), 1)
        # the resident call is "not slower" when its 10-90 % range does not lie wholly above the caller-side path's
        res["resident_not_slower"] = bool(res["B"]["p10_us"] <= max(res["A"]["p90_us"], res["A2"]["p90_us"]))
        res["resident_faster"] = bool(res["B"]["p90_us"] < min(res["A"]["p10_us"], res["A2"]["p10_us"]))
        out["sizes"][str(n)] = res
    print(json.dumps(out))


def main(argv):
    if argv and argv[0] == "child":
        return child(int(argv[1]) if len(argv) > 1 else 200)
    calls = int(argv[0]) if argv else 200
    dest = Path(argv[1]) if len(argv) > 1 else ROOT / "profiles" / "keyframe_points_latency.json"
    r = subprocess.run([sys.executable, str(Path(__file__).resolve()), "child", str(calls)], capture_output=True, text=True,
                       timeout=900)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        return r.returncode
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    dest.parent.mkdir(parents=True, exist_ok=True)
    dest.write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
