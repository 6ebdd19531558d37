"""The bit-sliced builds with the weights frozen in kind (csrc/ldpc_bs_kernel.h, WF; GPU
only).  Where the geometry-frozen build of wman would run and every iteration's check table and
channel table is one of the fixed set (or the identity channel table), the launch takes a build that
has no other path for either table and reads the ids from LDS words inside the T loop.  The tables
are the same tables, so every output must equal, bit for bit, that of the same call with
LDPC_BS_WF=0 (read at every launch), which is checked against the flood kernel once per T and
weight set, and the oracle's counters on the golden fixture.

  wman z = 24, B = 1, 33 and 167 (one ragged pack; two; six, looping back by ticket with
  LDPC_BS_GRID=1), T = 1, 2, 20, LDPC_BS_GRID = 1 and unset, decode and decode_awgn.
  Weights: the shipped C2 set, and a synthetic set -- alpha through -0.3, 0, 0.03, 0.5, 0.75, 1.0,
  1.5, 2.5 over the iterations, beta = 1 (the identity channel table) at iterations 0, 2, 5 and 19,
  C2's beta elsewhere.
  "Everything": counters, frame flags, iter_wrong; every iteration's hard decisions and the word
  mode run the export builds, which have no such build: last_wf() is False there and the results
  are the reference's.
  NMSDecoder.last_wf() says which build ran: asserted after every decode.
  One pack with an LLR off the quantizer grid goes to the fix-up path in either build.
"""
import os

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
DATA = os.path.join(ROOT, "ldpc_error_floor_amd", "data")
SIZES = [1, 33, 167]
ITERS = [1, 2, 20]
GRIDS = ["1", None]                     # LDPC_BS_GRID; None: unset
SNR = 3.5
SEED, OFFSET = 31, 7177
NAME = "bsl[p32,w9,d15,v6,l4]"
SYNTH_ALPHA = [-0.3, 0.0, 0.03, 0.5, 0.75, 1.0, 1.5, 2.5]
SYNTH_ID = [0, 2, 5, 19]                # iterations whose beta is 1
_cache = {}


def _graph():
    if "graph" not in _cache:
        from ldpc_error_floor_amd.code import CodeParams, TannerGraph, load_base_graph
        proto = load_base_graph(os.path.join(DATA, "BaseGraph", "wman_N0576_R34_z24.txt"))
        _cache["graph"] = (proto, TannerGraph(proto, 24), float(CodeParams(proto, 24).sigma(SNR)))
    return _cache["graph"]


def _weights(kind):
    """c2: the trained C2 weights.  synth: alpha[t] = SYNTH_ALPHA[(t + 3) % 8] (iteration 0 weighs
    with 0.5: the later ones then have messages to weigh), C2's beta but 1 at SYNTH_ID."""
    from ldpc_error_floor_amd.weights import DecoderWeights, expand_weights, read_weight_file
    proto, g, _ = _graph()
    wf = read_weight_file(os.path.join(DATA, "Weights", "C0_wman_N0576_R34_z24_Opt_Weight_End20.txt"))
    W = expand_weights((3, 0, 3), {0: wf.blocks[0], 2: wf.blocks[2]}, 20, g)
    if kind == "c2":
        return W
    a = np.array([SYNTH_ALPHA[(t + 3) % 8] for t in range(20)], np.float32)
    beta = W.beta.copy()
    beta[SYNTH_ID] = 1.0
    return DecoderWeights(alpha=np.ascontiguousarray(np.repeat(a[:, None], g.E, axis=1)), alpha_ucn=None, beta=beta)


def _dec(device, kind):
    if ("dec", kind) not in _cache:
        from ldpc_error_floor_amd.decoder import NMSDecoder
        proto, _, _ = _graph()
        _cache["dec", kind] = NMSDecoder(proto, 24, _weights(kind), 2, 5, device=device)
    return _cache["dec", kind]


def _llr(device, n):
    """The first n rows of one stream, never written to."""
    if "llr" not in _cache:
        _cache["llr"] = _dec(device, "c2").awgn(max(SIZES), _graph()[2], seed=SEED, offset=OFFSET)
    return _cache["llr"][:n]


def _set(monkeypatch, name, value):
    if value is None:
        monkeypatch.delenv(name, raising=False)
    else:
        monkeypatch.setenv(name, value)


def _env(monkeypatch, wf=None, grid=None):
    _set(monkeypatch, "LDPC_BS_WF", wf)
    _set(monkeypatch, "LDPC_BS_GRID", grid)
    for name in ("LDPC_BS_AFIX", "LDPC_BS_NOBFIX", "LDPC_BS_FROZEN"):
        monkeypatch.delenv(name, raising=False)


def _np(r, keys=("counters", "flags", "iter_wrong")):
    return {k: getattr(r, k).cpu().numpy() for k in keys}


def _decode(dec, llr, T, wf, kernel="fused"):
    """The decode build's outputs; wf: what last_wf() must say (None: another kernel)."""
    r = dec.decode(llr, T=T, app=False, counters=True, flags=True, kernel=kernel, iter_wrong=True)
    if wf is not None:
        assert dec.last_kernel() == NAME, dec.last_kernel()
        assert dec.last_frozen() and dec.last_afix()
        assert dec.last_wf() == wf, (dec.last_wf(), wf)
    return _np(r)


def _exports(dec, llr, T, kernel="fused"):
    """Every iteration's hard decisions and the word mode: the export builds, never a WF build."""
    h = dec.decode(llr, T=T, app=False, hard=True, counters=True, kernel=kernel)
    out = dict(hard=h.hard, hard_counters=h.counters)
    if kernel == "fused":
        assert dec.last_kernel() == NAME and not dec.last_wf()
        w = dec.decode(llr, T=T, hard_last=True, word_flags=True, counters=True, flags=True)
        assert not dec.last_wf()
        out.update(word=w.hard_last, word_flags=w.word_flags, word_counters=w.counters, word_frame_flags=w.flags)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _same(got, want, what):
    assert sorted(got) == sorted(want)
    for k in want:
        assert np.array_equal(got[k], want[k]), (k,) + what


def _reference(device, monkeypatch, kind, n, T):
    """LDPC_BS_WF=0 with the default grid, computed once per shape and shared; the largest batch of
    each T is checked against flood, hard decisions included."""
    if ("ref", kind, n, T) not in _cache:
        dec = _dec(device, kind)
        _env(monkeypatch, wf="0")
        old = _decode(dec, _llr(device, n), T, wf=False)
        if n == max(SIZES):
            old.update(_exports(dec, _llr(device, n), T))
            fl = _decode(dec, _llr(device, n), T, wf=None, kernel="flood")
            fl.update(_exports(dec, _llr(device, n), T, kernel="flood"))
            for k in fl:
                assert np.array_equal(old[k], fl[k]), (k, kind, n, T)
            assert np.array_equal(old["word"].view(np.uint32), old["hard"][T - 1].view(np.uint32)), (kind, n, T)
            assert old["iter_wrong"][0].any(), (kind, n, T)      # (not trivial: iteration 0 leaves frame errors)
        _cache["ref", kind, n, T] = old
    return _cache["ref", kind, n, T]


@pytest.mark.parametrize("T", ITERS)
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["c2", "synth"])
def test_decode_equals_the_other_builds(cuda_device, monkeypatch, kind, n, grid, T):
    dec = _dec(cuda_device, kind)
    ref = _reference(cuda_device, monkeypatch, kind, n, T)
    _env(monkeypatch, wf="0", grid=grid)
    old = _decode(dec, _llr(cuda_device, n), T, wf=False)
    _env(monkeypatch, wf=None, grid=grid)
    new = _decode(dec, _llr(cuda_device, n), T, wf=True)
    _env(monkeypatch, wf="1", grid=grid)
    on = _decode(dec, _llr(cuda_device, n), T, wf=True)
    keys = ("counters", "flags", "iter_wrong")
    _same(old, {k: ref[k] for k in keys}, ("LDPC_BS_WF=0 vs reference", kind, n, grid, T))
    _same(new, {k: ref[k] for k in keys}, ("WF vs reference", kind, n, grid, T))
    _same(on, {k: ref[k] for k in keys}, ("LDPC_BS_WF=1 vs reference", kind, n, grid, T))
    if n == max(SIZES):
        # the export and word builds fall back, whatever the switch says
        _same(_exports(dec, _llr(cuda_device, n), T), {k: v for k, v in ref.items() if k not in keys},
              ("exports", kind, n, grid, T))


@pytest.mark.parametrize("T", ITERS)
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("kind", ["c2", "synth"])
def test_decode_awgn_equals_the_other_builds(cuda_device, monkeypatch, kind, grid, T):
    """The in-prologue channel build: the same stream as the float LLRs, so the same reference."""
    dec = _dec(cuda_device, kind)
    sigma = _graph()[2]
    for n in SIZES:
        ref = _reference(cuda_device, monkeypatch, kind, n, T)
        for wf in ("0", None):
            _env(monkeypatch, wf=wf, grid=grid)
            got = dec.decode_awgn(n, sigma, SEED, offset=OFFSET, T=T, counters=True, flags=True, iter_wrong=True)
            assert dec.last_kernel() == NAME + "+gen", dec.last_kernel()
            assert dec.last_frozen() and dec.last_afix() and dec.last_wf() == (wf is None)
            _same(_np(got), {k: ref[k] for k in ("counters", "flags", "iter_wrong")}, ("awgn", kind, n, grid, T, wf))


def test_synthetic_weights_exercise_the_tables(cuda_device, monkeypatch):
    """The synthetic set is not decoded the same whatever the tables: other frame errors than the
    trained set's."""
    a = _reference(cuda_device, monkeypatch, "c2", 167, 20)
    b = _reference(cuda_device, monkeypatch, "synth", 167, 20)
    assert not np.array_equal(a["iter_wrong"], b["iter_wrong"])
    assert not np.array_equal(a["hard"], b["hard"])


def test_golden_fixture_counters(cuda_device, monkeypatch):
    """The oracle's counters on the wman golden fixture (B = 24, T = 20), from the WF build."""
    from ldpc_error_floor_amd.code import TannerGraph
    from ldpc_error_floor_amd.decoder import NMSDecoder
    from ldpc_error_floor_amd.weights import expand_weights
    d = np.load(os.path.join(ROOT, "tests", "golden", "wman_303_q5_snr2.0.npz"))
    z, T = int(d["z"]), int(d["T"])
    W = expand_weights((3, 0, 3), {0: d["w0"], 2: d["w2"]}, T, TannerGraph(d["proto"], z))
    ref = d["app_x2"].astype(np.float32) / 2
    hd = ref >= 0
    wrong = hd.any(axis=2)
    pos = (ref[-1] > 0).any(axis=1)
    want = [int(hd[-1].sum()), int(wrong[-1].sum()), int(wrong.all(axis=0).sum()),
            int(2 * pos.sum() + (wrong[-1] & ~pos).sum())]
    dec = NMSDecoder(d["proto"], z, W, 2, 5, device=cuda_device)
    for wf in (None, "0"):
        _env(monkeypatch, wf=wf)
        r = dec.decode(d["llr"], app=False, counters=True, flags=True, iter_wrong=True)
        assert dec.last_kernel() == NAME and dec.last_wf() == (wf is None)
        assert r.counters.cpu().tolist() == want, (wf, r.counters.cpu().tolist(), want)
        iw = r.iter_wrong.cpu().numpy().view(np.uint32).reshape(T, -1)[:, 0]
        assert [int(x) for x in iw] == [int(sum(int(b) << i for i, b in enumerate(wrong[t]))) for t in range(T)], wf


@pytest.mark.parametrize("grid", GRIDS)
def test_off_grid_pack_takes_the_fixup(cuda_device, monkeypatch, grid):
    """One LLR off the quantizer grid in the second of six packs: that pack goes to the fix-up
    kernel, the others stay, and the results equal LDPC_BS_WF=0's and flood's."""
    dec = _dec(cuda_device, "c2")
    llr = _llr(cuda_device, 167).clone()
    llr[40, 17] += 0.123
    _env(monkeypatch, wf="0", grid=grid)
    old = _decode(dec, llr, 20, wf=False)
    _env(monkeypatch, wf=None, grid=grid)
    new = _decode(dec, llr, 20, wf=True)
    fl = _decode(dec, llr, 20, wf=None, kernel="flood")
    _same(new, old, ("off grid", grid))
    _same(new, fl, ("off grid vs flood", grid))
