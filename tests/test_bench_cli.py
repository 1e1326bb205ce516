"""bench.py's command line: a plain run measures the headline only, `--full` adds every other leg."""
import json
import os
import subprocess
import sys

import pytest

from tests.helpers import ROOT

EXTRA_LEGS = ("no_cpu_baseline", "no_per_pivot", "no_other_configs", "no_colpart_baseline", "no_colpart_ab")


def _parse(monkeypatch, *argv):
    monkeypatch.setenv("OPENBLAS_NUM_THREADS", "1")      # (what importing bench.py sets; undone after the test)
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_leaves_out_every_extra_leg(monkeypatch):
    args = _parse(monkeypatch, "--gpus", "1", "--steps", "20", "--warmup", "5")
    assert not args.full
    assert all(getattr(args, leg) for leg in EXTRA_LEGS)
    assert (args.steps, args.warmup) == (20, 5)


def test_full_run_keeps_the_extra_legs_and_their_switches(monkeypatch):
    args = _parse(monkeypatch, "--gpus", "1", "--steps", "20", "--warmup", "5", "--full")
    assert args.full
    assert not any(getattr(args, leg) for leg in EXTRA_LEGS)
    args = _parse(monkeypatch, "--full", "--no-cpu-baseline", "--no-colpart-ab")
    assert args.no_cpu_baseline and args.no_colpart_ab
    assert not (args.no_per_pivot or args.no_other_configs or args.no_colpart_baseline)


@pytest.mark.gpu
def test_plain_run_prints_the_headline_only():
    """`bench.py --gpus 1 --steps 20 --warmup 5`: one JSON line with the headline fields, none of the
    records `--full` adds, and no warm blocks behind the short timed region (so no roofline)."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20",
                          "--warmup", "5"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec["value"] > 0 and rec["unit"] == "pivots/s" and rec["higher_is_better"] is True
    assert rec["dtype"] == "f64" and rec["ms_per_step"] > 0 and (rec["steps"], rec["warmup"]) == (20, 5)
    assert abs(rec["value"] - 1e3 / rec["ms_per_step"]) <= 1e-9 * rec["value"]
    for key in ("per_pivot_kernel", "cpu_baseline", "parity_in_run", "other_configs", "steady_state_pivots_per_s"):
        assert key not in rec, key
    assert rec["roofline"] is None
