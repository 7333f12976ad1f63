"""The host build of the fused pyramid's tile geometry (tests/_pyrseamcore, csrc/vsg_geometry.h) through ctypes: the
per-(tile, level) records k_pyramid reads and the seam-column helper it shares with the host."""
import ctypes as C
import functools
import subprocess
from pathlib import Path

import numpy as np

DIR = Path(__file__).resolve().parent / "_pyrseamcore"
TILINGS = (0, 1, 2)


@functools.lru_cache(maxsize=None)
def lib():
    subprocess.check_call(["make", "-C", str(DIR)], stdout=subprocess.DEVNULL)
    L = C.CDLL(str(DIR / "libvsg_pyrseamcore.so"))
    L.ps_build.argtypes = [C.c_int, C.c_float] + [C.c_int] * 5
    L.ps_level.argtypes = [C.c_int, C.c_void_p]
    L.ps_tiling.argtypes = [C.c_int, C.c_void_p]
    L.ps_tile_level.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.ps_seam.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    return L


def seam(ox0, ox1):
    """pyr_seam / pyr_seam_column of an owned column range: ((a0, a1, nl, n), [seam columns])."""
    desc, cols = np.zeros(4, np.int32), np.zeros(16, np.int32)
    n = lib().ps_seam(ox0, ox1, desc.ctypes.data, cols.ctypes.data)
    return tuple(int(v) for v in desc), [int(c) for c in cols[:n]]


class Geometry:
    """build_geometry of one (w, h, nlevels, scale factor): levels [(w, h, pitch, img_off)], and per tiling its
    {ntiles, lds, ok, threads, rec_bytes} and records[tile][level] = dict(need, own, pitch, img_off, ncg, nrg, chunk, tab).
    Read out completely here: the library keeps one geometry at a time."""

    def __init__(self, w, h, nl, sf):
        L = lib()
        self.w, self.h, self.nl, self.sf = w, h, nl, sf
        self.rc = L.ps_build(500, sf, nl, 20, 7, h, w)
        self.levels, self.tilings = [], {}
        if self.rc != 0:
            return
        buf = np.zeros(16, np.int32)
        for l in range(nl):
            L.ps_level(l, buf.ctypes.data)
            self.levels.append(tuple(int(v) for v in buf[:4]))
        for ti in TILINGS:
            L.ps_tiling(ti, buf.ctypes.data)
            nt, lds, ok, threads, rec_bytes = (int(v) for v in buf[:5])
            recs = []
            for t in range(nt):
                per_level = []
                for l in range(nl):
                    L.ps_tile_level(ti, t, l, buf.ctypes.data)
                    v = [int(x) for x in buf[:14]]
                    per_level.append(dict(need=tuple(v[0:4]), own=tuple(v[4:8]), pitch=v[8], img_off=v[9], ncg=v[10],
                                          nrg=v[11], chunk=v[12], tab=v[13]))
                recs.append(per_level)
            self.tilings[ti] = dict(ntiles=nt, lds=lds, ok=bool(ok), threads=threads, rec_bytes=rec_bytes, records=recs)


@functools.lru_cache(maxsize=None)
def geometry(w, h, nl, sf):
    return Geometry(w, h, nl, sf)
