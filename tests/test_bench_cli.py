"""bench.py's command line (no GPU): the options every run of the benchmark relies on are there,
and a step count that could not be timed is refused before anything touches a device."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT


def _bench(args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args,
                          capture_output=True, text=True, timeout=120)


def test_bench_help_lists_full_and_dump_outputs():
    r = _bench(["--help"])
    assert r.returncode == 0, r.stderr[-2000:]
    for opt in ("--gpus", "--steps", "--warmup", "--full", "--dump-outputs"):
        assert opt in r.stdout


@pytest.mark.parametrize("args", [["--steps", "0"], ["--steps", "-3"], ["--warmup", "-1"]])
def test_bench_refuses_untimed_runs(args):
    r = _bench(["--gpus", "1"] + args)
    assert r.returncode == 2
    assert "--steps must be >= 1" in r.stderr
