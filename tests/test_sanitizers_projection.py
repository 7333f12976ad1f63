"""The projection geometry of the motion-model and relocalisation searches (visual_sgraphs_amd/csrc/vsg_project.h through
tests/_projectcore) under AddressSanitizer + UndefinedBehaviorSanitizer, as tests/test_sanitizers.py does for the host core:
the `asan` target is built and tests/test_projection_reference.py runs against it in a child interpreter with libasan
preloaded; any report fails the run."""
from test_sanitizers import _run_under_asan


def test_projectcore_is_clean_under_asan_and_ubsan():
    _run_under_asan("test_projection_reference.py", {"VSG_PROJECTCORE_ASAN": "1"})
