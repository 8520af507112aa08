"""bench.py as a command: a plain run reports the headline and writes --dump-outputs, and nothing else; --full adds the other
plans mode and the CPU baseline (here on a tiny set, --extras 0)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--config", "rs90", "--maps", "8", "--steps", "2", "--warmup", "1"]


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *SMALL, *args],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_reports_the_headline_only(tmp_path):
    d = _bench("--dump-outputs", str(tmp_path / "dump"))
    assert d["unit"] == "ms" and d["higher_is_better"] is False and d["dtype"] == "f64"
    assert d["steps"] == 2 and d["warmup"] == 1
    assert d["value"] == d["ms_per_step"] > 0
    assert d["analysing_run_ms"] == d["value"] and d["resolve_ms"] is None
    assert not {"cpu_baseline", "cg_spmv_stream", "e2e_cli"} & set(d)
    for name in ("stno", "stVal"):
        assert os.path.exists(tmp_path / "dump" / f"{name}.npy")


def test_full_run_adds_the_other_mode_and_the_cpu_baseline():
    d = _bench("--full", "--extras", "0")
    assert d["value"] == d["ms_per_step"] == d["analysing_run_ms"] > 0
    assert d["resolve_ms"] > 0
    cb = d["cpu_baseline"]
    assert cb["value"] > 0
    assert cb["pose_param_max_rel_err_vs_oracle"] < cb["parity_tolerance"]
    assert cb["feature_param_max_rel_err_vs_oracle"] < cb["parity_tolerance"]
