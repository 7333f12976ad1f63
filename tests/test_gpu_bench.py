"""bench.py at N = 1 on a small batch: a plain run prints the headline line and measures or checks nothing else; --full adds
the serialized per-kernel pass (roofline), the parity gate against the CPU oracle and the CPU baselines, after the same
timed steps with the same outputs."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
SMALL = ["--gpus", "1", "--batch", "16", "--steps", "3", "--warmup", "2", "--ramp-steps", "2"]
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("parity", "roofline", "cpu_baseline", "cpu_baseline_2_threads", "cpu_baseline_all_cores", "host_api",
             "matcher_latency", "other_configs", "content_sweep")


def _bench(args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, str(ROOT / "bench.py")] + SMALL + args, capture_output=True, text=True,
                       timeout=600, env=env, cwd=str(ROOT))
    assert r.returncode == 0, r.stderr[-1500:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    out = tmp_path_factory.mktemp("plain")
    return _bench(["--dump-outputs", str(out)]), out


def test_plain_run_is_the_headline_line(plain):
    d, out = plain
    assert all(k in d for k in HEADLINE)
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["unit"] == "frames/s" and d["higher_is_better"] is True
    assert d["steps"] == 3 and d["warmup"] == 2 and d["n_gpus"] == 1 and d["full"] is False
    assert not set(FULL_ONLY) & set(d)
    assert d["outputs_dumped"]["frames"] == 16 and (out / "descriptors.npy").exists()


def test_full_run_adds_the_checks_after_the_same_steps(plain, tmp_path):
    d = _bench(["--full", "--no-extras", "--cpu-seconds", "1", "--dump-outputs", str(tmp_path)])
    assert all(k in d for k in HEADLINE) and d["full"] is True
    assert d["parity"]["bit_exact_vs_oracle"] is True and d["parity"]["frames_checked"] == 16
    assert "serialized_pass" in d["parity"] and d["roofline"]["stage_ms"]
    assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline_all_cores"]["value"] > 0
    # what the timed steps computed does not depend on what runs after them
    _, out = plain
    assert d["outputs_dumped"]["files"] == plain[0]["outputs_dumped"]["files"]
    for name in d["outputs_dumped"]["files"]:
        assert np.array_equal(np.load(tmp_path / f"{name}.npy"), np.load(out / f"{name}.npy")), name
