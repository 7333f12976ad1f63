#!/usr/bin/env python3
"""Warm latency of SearchByProjection(CurrentFrame, LastFrame, th, bMono) with the map points resident on the device, next
to what a caller does without them.  Runs on the GPU box; every run is a fresh child process, the variants alternating call
by call inside it.

A resident 1000-feature current frame (640x480, TUM1 intrinsics) and last frames whose features carry 500 / 1000 / 2000
slots (a quarter more features carry none).  The points lie in front of the camera; the current frame's features sit
where a subset projects, with slightly changed descriptors, so the search matches a real share.  Host clock around the
blocking calls, straight through ctypes with preallocated arrays on both sides:

  A   the caller-side path: the projection loop of ORBmatcher.cc:1686-1715 on the host (tools/track_last_cpu.cpp, the
      kernel's own arithmetic compiled -O2, one thread) + the gather of descriptors + vsg_frame_search_by_projection_last
  A2  A again: the run's own A-vs-A spread
  B   vsg_frame_search_last_frame: last frame and store resident, only the two poses change (a small rotation per call,
      the same for every variant)

usage: track_last_probe.py [calls] [out.json]   -> runs the child, writes the record (default profiles/track_last_latency.json)
       track_last_probe.py child [calls]        -> one JSON object on stdout (medians, 10-90 % range, microseconds)"""
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
TH, NFEAT = 7.0, 1000


def host_side(orb):
    out = ROOT / "tools" / "_bin"
    out.mkdir(exist_ok=True)
    so = out / "libtrack_last_cpu.so"
    csrc = ROOT / "visual_sgraphs_amd" / "csrc"
    src = [ROOT / "tools" / "track_last_cpu.cpp", csrc / "vsg_project.h", csrc / "vsg_frustum.h", csrc / "vsg_math.h"]
    if not so.exists() or any(f.stat().st_mtime > so.stat().st_mtime for f in src):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", str(csrc), "-o", str(so),
                               str(src[0])])
    L = C.CDLL(str(so))
    L.tl_host_side.argtypes = [C.POINTER(orb.FramePose), _f32p, C.c_int, _i32p, C.c_void_p, _f32p, _u8p, _u8p, _i32p, _u8p,
                               _u8p, _f32p, _f32p, _f32p, _i32p, _f32p]
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
        self.desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        self.observed = (rng.random(n) < 0.8).astype(np.uint8)
        src = rng.integers(0, n, NFEAT)
        keys = np.zeros(NFEAT, orb.KP_DTYPE)
        keys["x"], keys["y"] = px[src] + rng.normal(0, 2, NFEAT), py[src] + rng.normal(0, 2, NFEAT)
        oct_of = rng.integers(0, 8, n)
        keys["octave"], keys["angle"] = oct_of[src], rng.uniform(0, 360, NFEAT)
        d = self.desc[src].copy()
        d[:, :2] ^= rng.integers(0, 256, (NFEAT, 2), dtype=np.uint8)
        self.F = orb.Frame(NFEAT + 1)
        self.F.upload(keys, d, self.bounds)
        # the last frame: one feature per point plus a quarter without a map point, shuffled
        nl = n + n // 4
        self.slots = np.concatenate([np.arange(n), np.full(n // 4, -1)]).astype(np.int32)
        rng.shuffle(self.slots)
        self.lk = np.zeros(nl, orb.KP_DTYPE)
        self.lk["x"], self.lk["y"] = rng.uniform(1, 639, nl), rng.uniform(1, 479, nl)
        self.lk["octave"] = np.where(self.slots >= 0, oct_of[np.maximum(self.slots, 0)], rng.integers(0, 8, nl))
        self.lk["angle"] = rng.uniform(0, 360, nl)
        self.L = orb.Frame(nl + 1)
        self.L.upload(self.lk, rng.integers(0, 256, (nl, 32), dtype=np.uint8), self.bounds)
        self.mp = orb.MapPoints(n)
        self.mp.update(np.arange(n), world_pos=self.pos, desc=self.desc, observed=self.observed)
        self.sf = (np.float32(1.2) ** np.arange(8, dtype=np.float32)).astype(np.float32)
        self.b = np.array(self.bounds, np.float32)
        self.mb = float(po["mbf"] / po["fx"])
        z_ = np.zeros
        self.index, self.qd, self.qo = z_(nl, np.int32), z_((nl, 32), np.uint8), z_(nl, np.uint8)
        self.u, self.v, self.ur, self.oc, self.an = (z_(nl, np.float32), z_(nl, np.float32), z_(nl, np.float32),
                                                     z_(nl, np.int32), z_(nl, np.float32))
        self.tb, self.tm, self.dir = z_(NFEAT, np.uint8), z_(NFEAT, np.int32), C.c_int(0)
        self.fr, self.orb = fr, orb
        self.last_pose = orb.FramePose.make(**po)
        self.nproj = 0

    def pose_at(self, k):
        """The camera turned by a small angle about its y axis: the pose of call k."""
        a = 0.002 * (k % 50)
        Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        po = self.pose
        R = (Ry @ po["Rcw"].astype(np.float64)).astype(np.float32)
        t = (Ry @ po["tcw"].astype(np.float64)).astype(np.float32)
        return self.orb.FramePose.make(**self.fr.make_pose(R, t, po["fx"], po["fy"], po["cx"], po["cy"], po["mbf"]))

    def reset(self):
        self.tb[:] = 0
        self.tm[:] = -1

    def A(self, L, H, P):
        m = H.tl_host_side(C.byref(P), p(self.b, _f32p), len(self.slots), p(self.slots, _i32p), self.lk.ctypes.data_as(C.c_void_p),
                           p(self.pos, _f32p), p(self.desc, _u8p), p(self.observed, _u8p), p(self.index, _i32p),
                           p(self.qd, _u8p), p(self.qo, _u8p), p(self.u, _f32p), p(self.v, _f32p), p(self.ur, _f32p),
                           p(self.oc, _i32p), p(self.an, _f32p))
        self.nproj = m
        return L.vsg_frame_search_by_projection_last(
            self.F.handle, m, p(self.qd, _u8p), p(self.qo, _u8p), p(self.u, _f32p), p(self.v, _f32p), p(self.ur, _f32p), None,
            None, p(self.oc, _i32p), p(self.an, _f32p), TH, 0, p(self.sf, _f32p), 8, 1, p(self.tb, _u8p), p(self.tm, _i32p))

    def B(self, L, P):
        return L.vsg_frame_search_last_frame(
            self.F.handle, self.L.handle, self.mp.handle, p(self.slots, _i32p), C.byref(P), C.byref(self.last_pose), self.mb, 1,
            TH, p(self.sf, _f32p), 8, 1, p(self.tb, _u8p), p(self.tm, _i32p), C.byref(self.dir), None, None, None, None)


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
        nm = {}
        for k in range(calls + 20):
            P = c.pose_at(k)
            for name in ("A", "B", "A2"):
                c.reset()
                t0 = time.perf_counter()
                r = c.A(L, H, P) if name[0] == "A" else c.B(L, P)
                dt = (time.perf_counter() - t0) * 1e6
                assert r >= 0, (name, r)
                tm = c.tm.copy()
                if name[0] == "A":  # compacted indices -> last-frame features
                    tm[tm >= 0] = c.index[tm[tm >= 0]]
                nm[name] = (r, tm)
                if k >= 20:
                    t[name].append(dt)
            assert nm["A"][0] == nm["B"][0] and np.array_equal(nm["A"][1], nm["B"][1])  # the variants compute the same thing
        res = {k: stats(v) for k, v in t.items()}
        res["last_features"], res["projected_last"], res["nmatches_last"] = len(c.slots), int(c.nproj), int(nm["B"][0])
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
    dest = Path(argv[1]) if len(argv) > 1 else ROOT / "profiles" / "track_last_latency.json"
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
