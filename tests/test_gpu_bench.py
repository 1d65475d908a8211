"""bench.py on one GPU: a plain run does only the headline (set-up, warm-up, timed steps, the line); --full adds the runs of
its own (all-fp64 repetition, assembly timed alone, CPU baseline) on the same timed steps."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _line(extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--cells", "48,12,12", "--steps", "2", "--warmup", "1"] + extra,
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{") and '"metric"' in ln]
    assert r.returncode == 0 and len(lines) == 1, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    return json.loads(lines[0])


def test_bench_plain_run_is_the_headline_only_and_full_adds_the_secondary_figures():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no HIP device is visible")
    plain = _line([])
    full = _line(["--full"])
    for d in (plain, full):
        assert d["value"] > 0 and d["ms_per_step"] > 0 and d["steps"] == 2 and d["warmup"] == 1
        assert d["unit"] == "M-DOF/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
        assert d["roofline"]["fine_level_spmv_kernels"]
    assert plain["all_f64_preconditioner"] is None and plain["cpu_baseline"] is None
    assert plain["roofline"]["assembly_kernels"] is None
    assert full["all_f64_preconditioner"]["value"] > 0 and full["cpu_baseline"]["value"] > 0
    assert full["roofline"]["assembly_kernels"]["avg_ms"] > 0
    # the timed steps are the same Newton sequence either way
    lp, lf = plain["config"]["newton_log_fnorm_kspits_reason"], full["config"]["newton_log_fnorm_kspits_reason"]
    assert [c for _, _, c in lp] == [c for _, _, c in lf]
    assert all(abs(b1 - b2) <= 3 for (_, b1, _), (_, b2, _) in zip(lp, lf))
