#!/usr/bin/env python3
"""Warm latency of the device-resident KeyFrameDatabase (vsg_kfdb_*) next to a std::list restatement on the CPU
(tools/kfdb_cpu.cpp, built by tools/Makefile).  Runs on the GPU box.

For 1 000, 5 000 and 50 000 keyframes of ~800 Zipf-distributed word ids (10^6-word vocabulary, so the lists of the
frequent words are long; L1 scoring): add per keyframe, DetectRelocalizationCandidates and DetectNBestCandidates per
query, wall time from the host call to the returned candidates.  Both sides run the same query sequence from the same
state, so their candidate lists must agree: the checksums are compared.

usage: kfdb_latency.py [sizes ...]   (default 1000 5000 50000); prints one JSON line per size."""
import ctypes as C
import json
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from visual_sgraphs_amd import orb, synth  # noqa: E402

WORDS, NQ, WARM = 800, 20, 3


def zipf_bows(rng, n, nwords, a=1.1):
    ids = np.empty((n, WORDS), np.int32)
    for k in range(n):
        u = np.unique(np.minimum(rng.zipf(a, 3 * WORDS) - 1, nwords - 1))
        while len(u) < WORDS:
            u = np.unique(np.concatenate([u, np.minimum(rng.zipf(a, WORDS) - 1, nwords - 1)]))
        ids[k] = np.sort(rng.permutation(u)[:WORDS])
    vals = rng.random((n, WORDS)) + 0.05
    return ids, vals / vals.sum(axis=1, keepdims=True)


def run(voc, n, rng):
    ids, vals = zipf_bows(rng, n + NQ + WARM, voc.nwords)
    with tempfile.NamedTemporaryFile(suffix=".bin", delete=False) as f:
        f.write(np.array([n, NQ, WORDS, voc.nwords, WARM], np.int32).tobytes())
        for k in range(n + NQ + WARM):
            f.write(ids[k].astype(np.uint32).tobytes() + vals[k].tobytes())
        path = f.name
    cpu = json.loads(subprocess.check_output([str(ROOT / "tools" / "_bin" / "kfdb_cpu"), path], timeout=900))
    Path(path).unlink()

    db = orb.KeyFrameDatabase(voc)
    L, h = db._L, db._h
    f64p, u64p = C.POINTER(C.c_double), C.POINTER(C.c_uint64)
    t0 = time.perf_counter()
    for k in range(n):
        a, v = ids[k], vals[k]
        orb._check(L.vsg_kfdb_add(h, k + 1, 0, a.ctypes.data_as(orb._i32p), v.ctypes.data_as(f64p), WORDS), "add")
    add_ms = (time.perf_counter() - t0) / n * 1e3
    db._seen.update(range(1, n + 1))
    db.set_covisibility({k + 1: [u + 1 for d in range(1, 6) for u in (k + d, k - d) if 0 <= u < n] for k in range(n)})
    # warm-up: the thread's arena grows to its steady size (query ids no timed query uses; the CPU side replays them,
    # since queries leave state behind)
    for w in range(WARM):
        db.DetectRelocalizationCandidates(3000000 + w, (ids[n + NQ + w], vals[n + NQ + w]), 0)
        db.DetectNBestCandidates(4000000 + w, (ids[n + NQ + w], vals[n + NQ + w]), [], 0, 3)
    qbow = [(ids[(q * 7919) % n], vals[(q * 7919) % n]) if q % 2 == 0 else (ids[n + q], vals[n + q]) for q in range(NQ)]
    sum_r, t_r = 0, []
    for q in range(NQ):
        t0 = time.perf_counter()
        out = db.DetectRelocalizationCandidates(1000000 + q, qbow[q], 0)
        t_r.append(time.perf_counter() - t0)
        sum_r += sum(x * (i + 1) * (q + 1) for i, x in enumerate(out))
    sum_n, t_n = 0, []
    for q in range(NQ):
        k = (q * 7919) % n
        conn = [u + 1 for d in range(1, 6) for u in (k + d, k - d) if 0 <= u < n]
        t0 = time.perf_counter()
        loop, _ = db.DetectNBestCandidates(2000000 + q, (ids[k], vals[k]), conn, 0, 3)
        t_n.append(time.perf_counter() - t0)
        sum_n += sum(x * (i + 1) * (q + 1) for i, x in enumerate(loop))
    db.close()
    gpu = dict(add_ms=round(add_ms, 4), reloc_ms=round(float(np.mean(t_r)) * 1e3, 4),
               reloc_ms_median=round(float(np.median(t_r)) * 1e3, 4), nbest_ms=round(float(np.mean(t_n)) * 1e3, 4),
               nbest_ms_median=round(float(np.median(t_n)) * 1e3, 4))
    same = cpu["reloc_checksum"] == sum_r % 2 ** 64 and cpu["nbest_checksum"] == sum_n % 2 ** 64
    return dict(n_kf=n, words=WORDS, queries=NQ, zipf_a=1.1, gpu=gpu,
                cpu={k: cpu[k] for k in ("add_ms", "reloc_ms", "nbest_ms")}, outputs_agree=same)


def main():
    sizes = [int(x) for x in sys.argv[1:]] or [1000, 5000, 50000]
    voc = orb.ORBVocabulary(synth.synthetic_vocabulary(10, 6, seed=7))  # 10^6 words, L1 scoring
    rng = np.random.default_rng(11)
    ok = True
    for n in sizes:
        r = run(voc, n, rng)
        ok &= r["outputs_agree"]
        print(json.dumps(r), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
