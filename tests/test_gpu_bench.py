"""bench.py's multi-rank path (GPU only): ``bench.py --gpus 2`` started without a launcher
spawns its two ranks itself; with LDPC_BENCH_BACKEND=gloo both share the one GPU of the test
box.  The all-reduced counters must equal two single-process decodes of the rank slices
(global Philox offsets 0 and B), and the JSON line must report the whole job."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_bench_spawns_ranks_and_reduces(cuda_device):
    import torch
    sys.path.insert(0, ROOT)
    import bench
    from ldpc_error_floor_amd.decoder import NMSDecoder
    B, steps = 4096, 2
    env = dict(os.environ, LDPC_BENCH_BACKEND="gloo")
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--batch",
                        str(B), "--steps", str(steps), "--warmup", "1", "--no-cpu-baseline"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["config"]["parallelism"] == "dp2"
    assert out["fer_at_snr"]["frames"] == 2 * B * steps
    assert out["counters"]["rank_offsets"] == [0, B]
    cfg = bench.CONFIGS["C2"]
    proto, g, W, cp = bench.load_problem(config="C2")
    dec = NMSDecoder(proto, 24, W, 2, 5, device=cuda_device)
    cnt = torch.zeros(4, dtype=torch.int64, device=cuda_device)
    for off in (0, B):
        llr = dec.awgn(B, float(cp.sigma(cfg["snr"])), seed=1076, offset=off)
        dec.decode(llr, T=cfg["T"], app=False, counters=cnt)
    want = [steps * v for v in cnt.cpu().tolist()]
    c = out["counters"]
    assert [c["bit_err_last"], c["frame_err_last"], c["frame_err_all"], c["loss2"]] == want


def _bench_line(args):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_bench_plain_run_dumps_last_step(cuda_device, tmp_path):
    """A plain run times --steps decodes and nothing else; --dump-outputs writes the counters
    of the last timed decode alone, which one decode of the same Philox batch reproduces."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    from ldpc_error_floor_amd.decoder import NMSDecoder
    B, steps = 4099, 3                       # not a multiple of the 32-codeword pack
    out = _bench_line(["--gpus", "1", "--batch", str(B), "--steps", str(steps), "--warmup", "1",
                       "--dump-outputs", str(tmp_path / "dump")])
    assert out["steps"] == steps and out["fer_at_snr"]["frames"] == B * steps
    assert out["ms_per_step"] > 0 and out["unit"] == "codewords/s" and out["higher_is_better"]
    # value = B / (seconds per step); ms_per_step is rounded to 0.001 ms, value to 0.1
    ms = out["ms_per_step"]
    assert B / ((ms + 0.00051) / 1e3) - 0.1 <= out["value"] <= B / ((ms - 0.00051) / 1e3) + 0.1
    for moved in ("e2e_with_rng", "cpu_baseline", "companions"):
        assert moved not in out
    assert os.listdir(tmp_path / "dump") == ["counters.npy"]
    got = np.load(tmp_path / "dump" / "counters.npy")
    assert got.dtype == np.float64 and got.shape == (4,)
    cfg = bench.CONFIGS["C2"]
    proto, g, W, cp = bench.load_problem(config="C2")
    dec = NMSDecoder(proto, 24, W, 2, 5, device=cuda_device)
    llr = dec.awgn(B, float(cp.sigma(cfg["snr"])), seed=1076)
    want = dec.decode(llr, T=cfg["T"], app=False, counters=True).counters.cpu().tolist()
    assert got.tolist() == want and want[1] > 0
    c = out["counters"]
    assert [c["bit_err_last"], c["frame_err_last"], c["frame_err_all"], c["loss2"]] == \
        [steps * v for v in want]


def test_bench_full_adds_the_sweep_step(cuda_device):
    """--full reports what a plain run leaves out (here the sweep step; the CPU baseline and the
    companions belong to the default-size run) beside the same headline fields."""
    out = _bench_line(["--gpus", "1", "--batch", "4096", "--steps", "2", "--warmup", "1", "--full",
                       "--no-cpu-baseline"])
    assert out["steps"] == 2 and out["ms_per_step"] > 0
    assert out["e2e_with_rng"]["ms_per_step"] > 0 and out["e2e_with_rng"]["codewords_per_s"] > 0
    assert "cpu_baseline" not in out and "companions" not in out


def test_bench_rank_failure_propagates():
    """A rank that fails makes the launcher exit non-zero (and stops the other rank)."""
    env = dict(os.environ, LDPC_BENCH_BACKEND="gloo")
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2",
                        "--config", "C2", "--iters", "999", "--batch", "256", "--steps", "1",
                        "--no-cpu-baseline"], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode != 0
    assert "exited with status" in r.stderr
