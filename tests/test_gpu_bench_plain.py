"""bench.py --gpus 1 as a plain run and with --full: a plain run prints the headline line and does nothing the figure does not
need (no checksums, no traffic passes, no CPU baseline); --full adds them."""
import json
import os
import subprocess
import sys

import pytest

# bench.py is a GPU process of its own next to the workers (pytest.ini)
pytestmark = pytest.mark.xdist_group("gpu_procs")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _line(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--size", "16"] + list(extra)
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert len(r.stdout.strip().splitlines()) == 1, r.stdout[-2000:]
    line = json.loads(r.stdout)
    assert line["metric"] == "element stiffness assemblies/sec (3D p=3 Poisson, 256^3 elems)" and line["unit"] == "elements/s"
    assert line["higher_is_better"] is True and line["dtype"] == "f64" and line["steps"] == 2 and line["warmup"] == 1
    assert line["value"] > 0 and abs(line["value"] * line["ms_per_step"] / 1e3 - 16 ** 3) < 1e-6 * 16 ** 3
    assert len(line["per_step"]["ms"]) == 2 and line["roofline"]["avg_launch_ms"] > 0
    return line


@pytest.mark.gpu
def test_bench_plain_run_is_lean():
    line = _line()
    assert line["config"]["checksum"] is None and line["config"]["checksum_check"] is None
    assert line["roofline"]["traffic"] is None and line["roofline"]["traffic_source"] is None
    assert "cpu_baseline" not in line and "speedup_vs_cpu" not in line


@pytest.mark.gpu
def test_bench_full_adds_checksums():
    line = _line("--full", "--no-cpu-baseline", "--no-live-traffic")
    cs = line["config"]["checksum"]
    assert len(cs) == 4 and all(x == x for x in cs) and cs[1] > 0
    assert "cpu_baseline" not in line
