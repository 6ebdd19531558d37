"""The geometry-frozen builds of the wman bit-sliced kernel on the GPU (csrc/ldpc_bs_frozen.h,
DESIGN 3.3): the decode and the in-prologue channel build with the pack geometry as compile-time
constants must give, bit for bit, what oracle.nms_oracle gives and what the generic build
(LDPC_BS_FROZEN=0) gives for the same call -- `counters`, `frame_flags` and `iter_wrong`.

  wman N576 z = 24, the trained C2 weights, 3.5 dB; QMS q = 5 and -5 (q = 4 once: qmax is a
  run-time argument, so the frozen build serves it too, which the case asserts).
  B = 1 (one ragged pack), 33 (two packs), 167 (six packs, the last of 7 codewords).
  T = 1, 2, 3, 20: no fold of the frame-error words, one, the first of words zeroed before, the
  flagship's count; every T <= 20 runs the frozen build (RED is sized for 20 words).
  LDPC_BS_GRID = 1, 2, unset: with 1 and 2 a workgroup decodes several packs in sequence through
  the frozen pack loop.
  decode (LLRs in HBM) and decode_awgn (the channel generated in the kernel's prologue).

Each case first asserts through NMSDecoder.last_frozen() that the frozen build served the default
call and the generic build the forced one.  The LLRs are oracle.philox_oracle's, the stream
decode_awgn generates, so one oracle run per grid (167 codewords, 20 iterations) serves every case:
a case (B, T) is its [:T, :B] corner.  One more case puts a single LLR off the quantizer grid, so
that its pack takes the v5 fixup; there the reference is the flood kernel, which decodes any float
input."""
import os

import numpy as np
import pytest

from _helpers import counters_from_app, flags_from_app
from conftest import ROOT
from oracle import nms_oracle, philox_oracle

pytestmark = pytest.mark.gpu
DATA = os.path.join(ROOT, "ldpc_error_floor_amd", "data")
SEED, OFFSET = 29, 4099
SNR = 3.5
BMAX, TMAX = 167, 20
SIZES = [1, 33, 167]
GRIDS = ["1", "2", None]               # LDPC_BS_GRID; None: unset, the resident workgroups
NAME = "bsl[p32,w9,d15,v6,l4]"
_cache = {}


def _code():
    if "code" not in _cache:
        from ldpc_error_floor_amd.code import CodeParams, TannerGraph, load_base_graph
        from ldpc_error_floor_amd.weights import expand_weights, read_weight_file
        proto = load_base_graph(os.path.join(DATA, "BaseGraph", "wman_N0576_R34_z24.txt"))
        wf = read_weight_file(os.path.join(DATA, "Weights", "C0_wman_N0576_R34_z24_Opt_Weight_End20.txt"))
        W = expand_weights((3, 0, 3), {0: wf.blocks[0], 2: wf.blocks[2]}, TMAX, TannerGraph(proto, 24))
        _cache["code"] = (proto, W, float(CodeParams(proto, 24).sigma(SNR)))
    return _cache["code"]


def _oracle(q):
    """(LLRs [167, 576], the oracle's outputs [20, 167, .]) of grid q: computed once, left unchanged."""
    if ("oracle", q) not in _cache:
        proto, W, sigma = _code()
        llr = philox_oracle.awgn_qms_llr(BMAX, proto.shape[1] * 24, sigma, SEED, OFFSET, q)
        out = nms_oracle.decode(llr, proto, 24, W.alpha, W.alpha_ucn, W.beta, TMAX, 2, q)
        out["wrong"] = (out["app"] >= 0).any(axis=2)
        _cache["oracle", q] = (llr, out)
    return _cache["oracle", q]


def _dec(device, q):
    if ("dec", q) not in _cache:
        from ldpc_error_floor_amd.decoder import NMSDecoder
        proto, W, _ = _code()
        dec = NMSDecoder(proto, 24, W, 2, q, device=device)
        assert dec.kernel_info()[1] == NAME, dec.kernel_info()
        _cache["dec", q] = dec
    return _cache["dec", q]


def _llr(device, q):
    import torch
    if ("llr", q) not in _cache:
        _cache["llr", q] = torch.from_numpy(_oracle(q)[0]).to(device)
    return _cache["llr", q]


def _set(monkeypatch, name, value):
    if value is None:
        monkeypatch.delenv(name, raising=False)
    else:
        monkeypatch.setenv(name, value)


def _run(dec, llr, B, T, gen):
    """(counters, flags, iter_wrong [T, B]) of one call, and whether the frozen build served it."""
    if gen:
        r = dec.decode_awgn(B, _code()[2], SEED, offset=OFFSET, T=T, counters=True, flags=True, iter_wrong=True)
        assert dec.last_kernel() == NAME + "+gen", dec.last_kernel()
    else:
        r = dec.decode(llr[:B], T=T, app=False, counters=True, flags=True, iter_wrong=True)
        assert dec.last_kernel() == NAME, dec.last_kernel()
    return (r.counters.cpu().numpy(), r.flags.cpu().numpy(), r.frame_errors(B)), dec.last_frozen()


def _check(device, monkeypatch, q, B, T, grid, gen):
    dec, llr = _dec(device, q), _llr(device, q)
    want = {k: v[:T, :B] for k, v in _oracle(q)[1].items()}
    ref = counters_from_app(want["app"]), flags_from_app(want["app"]), want["wrong"]
    _set(monkeypatch, "LDPC_BS_GRID", grid)
    _set(monkeypatch, "LDPC_BS_FROZEN", None)
    got, fz = _run(dec, llr, B, T, gen)
    assert fz, ("the frozen build serves the default call", q, B, T, grid, gen)
    _set(monkeypatch, "LDPC_BS_FROZEN", "0")
    gen0, fz0 = _run(dec, llr, B, T, gen)
    assert not fz0, ("LDPC_BS_FROZEN=0 forces the generic build", q, B, T, grid, gen)
    for k, g, g0, w in zip(("counters", "flags", "iter_wrong"), got, gen0, ref):
        assert np.array_equal(g, w), ("frozen vs oracle", k, q, B, T, grid, gen)
        assert np.array_equal(g0, w), ("generic vs oracle", k, q, B, T, grid, gen)
        assert np.array_equal(g, g0), ("frozen vs generic", k, q, B, T, grid, gen)


@pytest.mark.parametrize("gen", [False, True], ids=["decode", "decode_awgn"])
@pytest.mark.parametrize("T", [1, 2, 3, 20])
@pytest.mark.parametrize("q", [5, -5])
def test_frozen_equals_oracle_and_generic(cuda_device, monkeypatch, q, T, gen):
    """Every size on every grid (nine pairs of calls per case)."""
    wrong = _oracle(q)[1]["wrong"]
    assert 0 < wrong[TMAX - 1].sum() + wrong[2].sum() < 2 * BMAX       # the outputs are not trivial
    for B in SIZES:
        for grid in GRIDS:
            _check(cuda_device, monkeypatch, q, B, T, grid, gen)


def test_q4_runs_the_frozen_build(cuda_device, monkeypatch):
    """q = 4 (qmax 7): the grid's largest magnitude stays a run-time argument of the frozen
    builds, so they serve it; same comparison, six packs on two workgroups."""
    _check(cuda_device, monkeypatch, 4, 167, 20, "2", False)


def test_off_grid_pack_takes_the_fixup(cuda_device, monkeypatch):
    """One LLR off the q-grid in pack 2 of six, on a grid of two workgroups (the pack is the second
    of its workgroup's three): the frozen kernel flags the pack, the v5 fixup decodes it, and the
    result equals the flood kernel's and the generic build's."""
    dec = _dec(cuda_device, 5)
    llr = _llr(cuda_device, 5).clone()
    llr[2 * 32 + 5, 17] += 0.1
    T = 20
    _set(monkeypatch, "LDPC_BS_GRID", "2")
    _set(monkeypatch, "LDPC_BS_FROZEN", None)
    got, fz = _run(dec, llr, BMAX, T, False)
    assert fz
    _set(monkeypatch, "LDPC_BS_FROZEN", "0")
    gen0, fz0 = _run(dec, llr, BMAX, T, False)
    assert not fz0
    fl = dec.decode(llr, T=T, app=False, counters=True, flags=True, iter_wrong=True, kernel="flood")
    assert dec.last_kernel() == "flood" and not dec.last_frozen()
    ref = fl.counters.cpu().numpy(), fl.flags.cpu().numpy(), fl.frame_errors(BMAX)
    # without the fixup the flagged pack is left alone: the frozen kernel did flag it
    _set(monkeypatch, "LDPC_BS_FROZEN", None)
    monkeypatch.setenv("LDPC_BS_FIXUP", "0")
    import torch
    flags = torch.full((BMAX,), 255, dtype=torch.uint8, device=cuda_device)
    r = dec.decode(llr, T=T, app=False, counters=True, flags=flags, iter_wrong=True)
    assert dec.last_frozen() and np.all(r.flags.cpu().numpy()[64:96] == 255)
    for k, g, g0, w in zip(("counters", "flags", "iter_wrong"), got, gen0, ref):
        assert np.array_equal(g, w), ("frozen vs flood", k)
        assert np.array_equal(g, g0), ("frozen vs generic", k)
