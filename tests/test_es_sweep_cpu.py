"""fer_sweep(early_stop=True) on CPU: a stand-in decoder (the oracle with the early-stop reference
of tests/_es_ref.py applied) exercises the sweep's own logic -- the [nSNR, T] histogram kept beside
the counters, its independence of the batch size, the checkpoint state and key, and the refusals."""
import json
import os

import numpy as np
import pytest

from _es_ref import es_reference
from _helpers import OracleDecoder
from conftest import GOLDEN, ROOT
from oracle import nms_oracle
from ldpc_error_floor_amd.fer import fer_sweep
from ldpc_error_floor_amd.metrics import Counters

SIGMAS = [0.6, 0.55]      # wman at T = 8: frames stop anywhere from iteration 2 on, some never
T = 8
N_CW = 150


class EsOracleDecoder(OracleDecoder):
    """OracleDecoder with ``decode(early_stop=True, iter_hist=...)`` and ``supports_early_stop``."""
    es = True

    def supports_early_stop(self, T=None):
        return self.es

    def decode(self, llr, T=None, counters=None, early_stop=False, iter_hist=None, **kw):
        if not early_stop:
            return super().decode(llr, T=T, counters=counters, **kw)
        T = T or self.T
        x = np.asarray(llr.cpu().numpy(), np.float32)
        out = nms_oracle.decode(x.reshape(x.shape[0], -1), self.proto, self.z, self.W.alpha,
                                self.W.alpha_ucn, self.W.beta, T, self.dt, self.q, graph=self.g)
        r = es_reference(out["hard"], out["synd"], self.target_bits)
        if counters is not None:
            counters += self.torch.from_numpy(r["counters"])
        if iter_hist is not None:
            iter_hist += self.torch.from_numpy(r["iter_hist"])


@pytest.fixture(scope="module")
def dec():
    from ldpc_error_floor_amd.code import TannerGraph, load_base_graph
    from ldpc_error_floor_amd.weights import expand_weights
    d = np.load(os.path.join(GOLDEN, "results_wman_303.npz"))
    proto = load_base_graph(os.path.join(ROOT, "ldpc_error_floor_amd", "data", "BaseGraph",
                                         "wman_N0576_R34_z24.txt"))
    W = expand_weights((3, 0, 3), {0: d["w0"], 2: d["w2"]}, T, TannerGraph(proto, 24))
    return EsOracleDecoder(proto, 24, W)


def _tuples(res):
    return [(c.bit_err_last, c.frame_err_last, c.frame_err_all, c.loss2, c.iter_hist.tolist()) for c in res]


@pytest.fixture(scope="module")
def full(dec):
    return _tuples(fer_sweep(dec, SIGMAS, N_CW, 32, seed=1076, early_stop=True))


class Stop(Exception):
    pass


def _interrupt_after(n):
    calls = {"n": 0}

    def progress(si, done, total):
        calls["n"] += 1
        if calls["n"] == n:
            raise Stop()
    return progress


def test_histogram_beside_the_counters(dec, full):
    res = fer_sweep(dec, SIGMAS, N_CW, 32, seed=1076, early_stop=True)
    for c in res:
        assert c.iter_hist.dtype == np.int64 and c.iter_hist.shape == (T,)
        assert int(c.iter_hist.sum()) == N_CW and c.loss2 == 0
        want = float((c.iter_hist * np.arange(1, T + 1)).sum()) / N_CW
        assert c.mean_iterations == pytest.approx(want) and 1.0 <= want <= T
    # the frames stop at several different iterations, and some before T
    for c in res:
        assert sum(1 for x in c.iter_hist if x) >= 3 and c.iter_hist[:T - 1].sum() > 0 and c.iter_hist[T - 1] > 0


def test_batch_size_does_not_change_the_result(dec, full):
    assert _tuples(fer_sweep(dec, SIGMAS, N_CW, 50, seed=1076, early_stop=True)) == full


def test_without_the_mode_nothing_changes(dec):
    res = fer_sweep(dec, SIGMAS[:1], 40, 32, seed=1076)
    assert res[0].iter_hist is None and res[0].mean_iterations is None
    assert Counters.from_array([1, 2, 3, 4], 10, 5).iter_hist is None


def test_checkpointed_resume_equals_uninterrupted(dec, full, tmp_path):
    ck = str(tmp_path / "es.ckpt")
    with pytest.raises(Stop):
        fer_sweep(dec, SIGMAS, N_CW, 32, seed=1076, early_stop=True, checkpoint=ck, checkpoint_every=2,
                  progress=_interrupt_after(7))
    st = json.load(open(ck))
    assert st["done"] is False and st["key"]["early_stop"] is True
    assert np.asarray(st["iter_hist"]).shape == (len(SIGMAS), T) and np.asarray(st["iter_hist"]).sum() > 0
    res = fer_sweep(dec, SIGMAS, N_CW, 32, seed=1076, early_stop=True, checkpoint=ck, checkpoint_every=2,
                    resume=True)
    assert _tuples(res) == full and json.load(open(ck))["done"] is True


def test_resume_with_the_other_mode_is_refused(dec, tmp_path):
    ck = str(tmp_path / "a.ckpt")
    with pytest.raises(Stop):
        fer_sweep(dec, SIGMAS, N_CW, 32, seed=1076, early_stop=True, checkpoint=ck, checkpoint_every=1,
                  progress=_interrupt_after(2))
    with pytest.raises(ValueError, match="checkpoint is for"):
        fer_sweep(dec, SIGMAS, N_CW, 32, seed=1076, checkpoint=ck, resume=True)
    ck2 = str(tmp_path / "b.ckpt")
    with pytest.raises(Stop):
        fer_sweep(dec, SIGMAS, N_CW, 32, seed=1076, checkpoint=ck2, checkpoint_every=1,
                  progress=_interrupt_after(2))
    assert "early_stop" not in json.load(open(ck2))["key"]      # keys without the mode stay as they were
    with pytest.raises(ValueError, match="checkpoint is for"):
        fer_sweep(dec, SIGMAS, N_CW, 32, seed=1076, early_stop=True, checkpoint=ck2, resume=True)


def test_uncor_path_with_early_stop_raises(dec, tmp_path):
    with pytest.raises(ValueError, match="uncor"):
        fer_sweep(dec, SIGMAS, N_CW, 32, early_stop=True, uncor_path=str(tmp_path / "U.txt"))


def test_decoder_without_the_mode_is_refused_at_once(dec, monkeypatch):
    monkeypatch.setattr(dec, "es", False)
    calls = []
    monkeypatch.setattr(dec, "awgn", lambda *a, **k: calls.append(1))
    with pytest.raises(ValueError, match="early_stop"):
        fer_sweep(dec, SIGMAS, N_CW, 32, early_stop=True)
    assert not calls
    with pytest.raises(ValueError, match="early_stop"):
        fer_sweep(OracleDecoder(dec.proto, 24, dec.W), SIGMAS, N_CW, 32, early_stop=True)
