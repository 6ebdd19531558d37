"""``--weights FILE --sharing a,b,c [--T n]`` of tools/floor_events.py and tools/sweep_c5.py (CPU, no
GPU): the file's weights decoded with the given sharing replace the config's; graph, lifting,
puncturing and shortening stay the config's.  ``weights_from_file`` builds the tables; the sweep
tool runs here with the oracle-backed stand-in decoder."""
import json
import os
import sys

import numpy as np
import pytest

from _helpers import OracleDecoder
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
SHIPPED = os.path.join(ROOT, "ldpc_error_floor_amd", "data", "Weights",
                       "C0_wman_N0576_R34_z24_Opt_Weight_End20.txt")


def _cascade_file(path, T=22, seed=3):
    """A [3,3,3] file of T rows per kind with alpha' != alpha in the last two rows."""
    from ldpc_error_floor_amd.weights import read_weight_file
    wf = read_weight_file(SHIPPED)
    rs = np.random.RandomState(seed)
    a = np.concatenate([wf.blocks[0][:20, 0], rs.uniform(0.5, 1.0, T - 20)])
    u = np.concatenate([wf.blocks[0][:20, 0], rs.uniform(0.2, 0.5, T - 20)])
    b = np.concatenate([wf.blocks[2][:20, 0], rs.uniform(0.8, 1.1, T - 20)])
    with open(path, "w") as f:
        f.write("3 3 3\n\n")
        for blk in (a, u, b):
            f.write("".join(f"{x!r}\n" for x in blk.tolist()) + "\n")
    return a, u, b


def test_weights_from_file(tmp_path):
    import bench
    from ldpc_error_floor_amd.weights import weights_from_file
    proto, g, W0, cp = bench.load_problem(config="C2")
    W = weights_from_file(SHIPPED, (3, 0, 3), g)
    assert W.T == 20 and W.alpha_ucn is None
    assert np.array_equal(W.alpha, W0.alpha) and np.array_equal(W.beta, W0.beta)
    W = weights_from_file(SHIPPED, ("3", "3", "3"), g, 12)
    assert W.T == 12 and np.array_equal(W.alpha_ucn, W.alpha) and np.array_equal(W.alpha, W0.alpha[:12])
    with pytest.raises(ValueError):
        weights_from_file(SHIPPED, (3, 3, 3), g, 21)           # the file holds 20 rows
    with pytest.raises(ValueError):
        weights_from_file(SHIPPED, (3, 3), g)
    path = str(tmp_path / "cascade.txt")
    a, u, b = _cascade_file(path)
    W = weights_from_file(path, (3, 3, 3), g)
    assert W.T == 22
    assert np.array_equal(W.alpha[:, 0], a.astype(np.float32)) and np.array_equal(W.alpha_ucn[:, 5], u.astype(np.float32))
    assert np.array_equal(W.beta[:, 7], b.astype(np.float32))
    assert (W.alpha_ucn[20:] != W.alpha[20:]).all() and np.array_equal(W.alpha_ucn[:20], W.alpha[:20])


@pytest.mark.parametrize("tool", ["floor_events", "sweep_c5"])
def test_the_options_go_together(tool, capsys):
    mod = __import__(tool)
    base = ["--config", "C2"] + (["--snr", "3.0"] if tool == "floor_events" else [])
    a = mod.parse(base + ["--weights", SHIPPED, "--sharing", "3,3,3", "--T", "12"])
    assert (a.weights, a.sharing, a.T) == (SHIPPED, "3,3,3", 12)
    a = mod.parse(base)
    assert a.weights is None and a.sharing is None and a.T is None
    for bad in (["--weights", SHIPPED], ["--sharing", "3,3,3"], ["--T", "12"]):
        with pytest.raises(SystemExit):
            mod.parse(base + bad)
    capsys.readouterr()


def test_sweep_tool_takes_the_file(tmp_path, monkeypatch):
    """The sweep of C2 with a 22-iteration cascade file: the stand-in decoder gets the file's
    weights (T = 22, alpha' set), and the counters are those of the oracle with them."""
    import bench
    import sweep_c5
    from ldpc_error_floor_amd.weights import weights_from_file
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("LDPC_SWEEP_BACKEND", "gloo")
    path = str(tmp_path / "cascade.txt")
    _cascade_file(path)
    seen = []

    class Standin(OracleDecoder):
        def set_weights(self, W):
            self.W, self.T = W, W.T
            seen.append(W)

    def make(config, device, batch):
        proto, g, W, cp = bench.load_problem(config=config)
        return Standin(proto, bench.CONFIGS[config]["z"], W)

    args = ["--config", "C2", "--deep-snrs", "2.0", "--deep", "16", "--batch", "8"]
    out = str(tmp_path / "file")
    assert sweep_c5.main(args + ["--out", out, "--weights", path, "--sharing", "3,3,3"], make_decoder=make) == 0
    assert len(seen) == 1 and seen[0].T == 22 and seen[0].alpha_ucn is not None
    with open(os.path.join(out, "sweep_c2.json")) as f:
        j = json.load(f)
    assert "cascade.txt as [3,3,3], T=22" in j["workload"]
    proto, g, W0, cp = bench.load_problem(config="C2")
    ref = make("C2", None, 8)
    ref.set_weights(weights_from_file(path, (3, 3, 3), g))
    out0 = str(tmp_path / "config")
    assert sweep_c5.main(args + ["--out", out0], make_decoder=lambda *a: ref) == 0
    with open(os.path.join(out0, "sweep_c2.json")) as f:
        j0 = json.load(f)
    keys = ("codewords", "frame_err_last", "frame_err_any_iter", "bit_err_last")
    assert [j["deep"][0][k] for k in keys] == [j0["deep"][0][k] for k in keys]
    assert j["deep"][0]["frame_err_last"] > 0
