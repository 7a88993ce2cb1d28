"""GPU: bench.py's plain run and its --full run, on a small scene and frame.

A plain run prints the headline line and nothing that takes a run of its own; --full adds the counters, the roofline block and the
other side measurements after the timed region.  Both runs time the same steps on the same seeded inputs, so what they dump agrees."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--tris", "20000", "--width", "256", "--height", "256"]
HEADLINE_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench(args, dump_dir):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *SMALL, *args, "--dump-outputs", str(dump_dir)],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-4000:]
    return json.loads(lines[0])


@pytest.mark.parametrize("workload", ["primary", "shaded"])
def test_plain_and_full_runs(tmp_path, workload):
    pytest.importorskip("torch")
    plain = _bench(["--workload", workload], tmp_path / "plain")
    full = _bench(["--workload", workload, "--full", "--no-cpu-baseline"], tmp_path / "full")
    for line in (plain, full):
        for k in HEADLINE_KEYS:
            assert k in line, (k, line)
        assert line["unit"] == "Mrays/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
        assert line["value"] > 0 and line["ms_per_step"] > 0 and line["steps"] == 3 and line["warmup"] == 1
    # what the plain run leaves out; `extras` is not checked here, since the custom frame size of SMALL skips it in both runs
    for k in ("roofline", "cpu_baseline"):
        assert k not in plain, k
    assert "roofline" in full and full["roofline"]["algorithmic_bytes_per_launch"] > 0
    if workload == "primary":
        assert "gather_ms_max_over_ranks" in full["config"] and "gather_ms_max_over_ranks" not in plain["config"]
        assert full["config"]["rays_entering_tree_rank0"] > 0
    else:
        assert "exactly_sized_frame_ms" in full["config"] and "exactly_sized_frame_ms" not in plain["config"]
    names = sorted(os.listdir(tmp_path / "plain"))
    assert names and names == sorted(os.listdir(tmp_path / "full"))
    for n in names:
        a, b = np.load(tmp_path / "plain" / n), np.load(tmp_path / "full" / n)
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), n
