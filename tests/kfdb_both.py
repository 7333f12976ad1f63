"""The GPU KeyFrameDatabase and the restatement (tests/kfdb_reference.py) driven by the same operations: after every
query the returned lists AND the six KeyFrame members the queries read and write (vsg_debug_kfdb_state) are compared,
floats as bits."""
import struct

import numpy as np

import kfdb_reference as kr
from visual_sgraphs_amd import orb

INVALID = -6  # VSG_ERR_INVALID


def with_scoring(blob, scoring):
    """The same vocabulary image with another scoring type (the third int of the header)."""
    return blob[:8] + struct.pack("<i", scoring) + blob[12:]


def ref_state(k):
    """The six members of a restatement KeyFrame, in the order of KeyFrameDatabase.debug_state, scores as float32 bits"""
    return (k.mnRelocQuery, k.mnRelocWords, int(np.float32(k.mRelocScore).view(np.uint32)),
            k.mnPlaceRecognitionQuery, k.mnPlaceRecognitionWords, int(np.float32(k.mPlaceRecognitionScore).view(np.uint32)))


def gpu_state(db, kf_id):
    """The same of the device database; None for an id it never saw"""
    try:
        rq, rw, rs, pq, pw, ps = db.debug_state(kf_id)
    except orb.VsgError as e:
        assert e.code == INVALID
        return None
    return rq, rw, int(rs.view(np.uint32)), pq, pw, int(ps.view(np.uint32))


FRESH = (0, 0, 0, 0, 0, 0)


class Both:
    """The GPU database and the restatement, driven by the same operations.  `sample`: the keyframe ids whose state is
    compared after every query (None: every keyframe the restatement knows)."""

    def __init__(self, voc, sample=None):
        self.gpu = orb.KeyFrameDatabase(voc)
        self.ref = kr.KeyFrameDatabase(voc.scoring)
        self.sample = sample
        self.n_queries = 0
        self.n_states = 0

    def close(self):
        self.gpu.close()

    def add(self, kf, bow, m):
        self.gpu.add(kf, bow, m)
        self.ref.add(kf, *bow, m)

    def erase(self, kf):
        self.gpu.erase(kf)
        self.ref.erase(kf)

    def clear(self):
        self.gpu.clear()
        self.ref.clear()

    def clear_map(self, m):
        self.gpu.clearMap(m)
        self.ref.clearMap(m)

    def set_map(self, kfs, maps):
        self.gpu.set_map(kfs, maps)
        for k, m in zip(kfs, maps):
            self.ref.set_map(k, m)

    def set_covisibility(self, neigh):
        self.gpu.set_covisibility(neigh)
        for k, n in neigh.items():
            self.ref.set_covisibility(k, n)

    def check_state(self, why=""):
        """Every (sampled) keyframe of the restatement has the same six members on the device.  A keyframe only the
        restatement knows (it makes one for an erase of an id never seen) must be untouched."""
        for kf_id in (self.ref.kfs if self.sample is None else self.sample):
            want = ref_state(self.ref.kf(kf_id))
            got = gpu_state(self.gpu, kf_id)
            assert got == want or (got is None and want == FRESH), (why, kf_id, got, want)
            self.n_states += 1

    def state(self, kf):
        got = gpu_state(self.gpu, kf)
        assert got == ref_state(self.ref.kf(kf)), (kf, got)
        return got[0], got[1], got[3], got[4]

    def reloc(self, qid, bow, m):
        got = self.gpu.DetectRelocalizationCandidates(qid, bow, m)
        want = self.ref.DetectRelocalizationCandidates(qid, *bow, m)
        assert got == want, (qid, got, want)
        self.n_queries += 1
        self.check_state(("reloc", qid))
        return got

    def nbest(self, qid, bow, conn, m, n, bad=()):
        got = self.gpu.DetectNBestCandidates(qid, bow, conn, m, n, bad)
        want = self.ref.DetectNBestCandidates(qid, *bow, conn, m, n, bad)
        assert got == want, (qid, got, want)
        self.n_queries += 1
        self.check_state(("nbest", qid))
        return got
