"""vsg::KeyFrameDatabase and vsg::ORBVocabulary::score of include/vsg_orb_adaptor.hpp from plain C++: the check program
of tests/_adaptor_kfdb compiles against the header, and without a device it says so instead of computing anything.  The
comparison with the restatement is the gpu test of tests/test_gpu_kfdb_edges.py."""
import subprocess
from pathlib import Path

from visual_sgraphs_amd import orb

ROOT = Path(__file__).resolve().parent.parent
ADAPTOR = ROOT / "tests" / "_adaptor_kfdb"


def test_cpp_adaptor_compiles_and_fails_loudly_without_device():
    L = orb.load_library()
    subprocess.check_call(["make", "-C", str(ADAPTOR)], stdout=subprocess.DEVNULL)
    adaptor = (ROOT / "include" / "vsg_orb_adaptor.hpp").read_text()
    for name in ("class KeyFrameDatabase", "void add(uint64_t kf_id, int32_t map_id, const BowVector &bow)", "void SetMap(",
                 "void SetCovisibility(", "DetectRelocalizationCandidates(uint64_t frame_id", "void DetectNBestCandidates(",
                 "double score(const std::map<unsigned, double> &v1"):
        assert name in adaptor, name
    if L.vsg_device_count() <= 0:
        r = subprocess.run([str(ADAPTOR / "kfdb_check"), "/dev/null", "/dev/null", "/dev/null"], capture_output=True, text=True)
        assert r.returncode == 3 and "no CPU fallback" in r.stdout


def test_debug_state_hook_is_bound_and_documented():
    L = orb.load_library()
    assert hasattr(L, "vsg_debug_kfdb_state") and "vsg_debug_kfdb_state" in orb.EXPORTS
    assert hasattr(orb.KeyFrameDatabase, "debug_state")
    assert L.vsg_debug_kfdb_state(None, 1, None, None, None) == -6  # VSG_ERR_INVALID: refused before any device call
