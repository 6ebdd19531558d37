"""The check phase's weight table through the fixed set's immediate truth tables (csrc/
ldpc_bs_kernel.h, AFX / beta_asm; GPU only).  Where alpha is one value per iteration, the
grid is q = 5 or -5 and every iteration's table Q(relu(alpha m)) is one of the 210 of
csrc/ldpc_beta_tabs.h, the pack-loop instances of the bit-sliced kernel (wman) weigh both minima
with two computed calls instead of a mux tree over table words in LDS.  The table is the same
table, so every output must equal, bit for bit, that of the LDS path (LDPC_BS_AFIX=0, read at every
launch), which is checked against the flood kernel once per T and weight set.

  wman z = 24, B = 33 and 167 (two and six packs, the last ragged), T = 1, 2, 20, the geometry-frozen
  decode build and the generic one (LDPC_BS_FROZEN=0), LDPC_BS_GRID = 1 and unset.
  Weights: the shipped C2 set, and a synthetic set whose alpha runs through -0.3, 0, 0.03, 0.5,
  0.75, 1.0, 1.5, 2.5 over the iterations (the all-zero table, a nearly-zero one, exact halves,
  the identity, saturation).
  "Everything": counters, frame flags, iter_wrong (the decode build), every iteration's hard
  decisions (the export build), the word mode's rows, flags and counters.
  NMSDecoder.last_afix() says which path ran: asserted after every decode.
  Per-row alpha, UCN weights and q = 4 keep the LDS path whatever the switch says; decode_awgn and
  decode_q8 take the new one; the 802.11n instance (UCN-compiled) is not touched.
"""
import os

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
DATA = os.path.join(ROOT, "ldpc_error_floor_amd", "data")
SIZES = [33, 167]
ITERS = [1, 2, 20]
GRIDS = ["1", None]                     # LDPC_BS_GRID; None: unset
SNR = 3.5
SEED, OFFSET = 31, 7177
NAME = "bsl[p32,w9,d15,v6,l4]"
SYNTH_ALPHA = [-0.3, 0.0, 0.03, 0.5, 0.75, 1.0, 1.5, 2.5]
_cache = {}


def _graph():
    if "graph" not in _cache:
        from ldpc_error_floor_amd.code import CodeParams, TannerGraph, load_base_graph
        proto = load_base_graph(os.path.join(DATA, "BaseGraph", "wman_N0576_R34_z24.txt"))
        _cache["graph"] = (proto, TannerGraph(proto, 24), float(CodeParams(proto, 24).sigma(SNR)))
    return _cache["graph"]


def _weights(kind):
    """c2: the trained C2 weights.  synth: C2's beta, alpha[t] = SYNTH_ALPHA[(t + 3) % 8] (iteration
    0 weighs with 0.5: the later ones then have messages to weigh).  rows: synth's alpha times
    1 or 0.75 by proto row (per-row alpha).  ucn: synth with alpha' = alpha / 2."""
    from ldpc_error_floor_amd.weights import DecoderWeights, expand_weights, read_weight_file
    proto, g, _ = _graph()
    wf = read_weight_file(os.path.join(DATA, "Weights", "C0_wman_N0576_R34_z24_Opt_Weight_End20.txt"))
    W = expand_weights((3, 0, 3), {0: wf.blocks[0], 2: wf.blocks[2]}, 20, g)
    if kind == "c2":
        return W
    a = np.array([SYNTH_ALPHA[(t + 3) % 8] for t in range(20)], np.float32)
    alpha = np.repeat(a[:, None], g.E, axis=1)
    if kind == "rows":
        alpha = (alpha * np.where(np.asarray(g.pe_row) % 2 == 0, 1.0, 0.75).astype(np.float32)[None, :]).astype(np.float32)
    ucn = (alpha * np.float32(0.5)).astype(np.float32) if kind == "ucn" else None
    return DecoderWeights(alpha=np.ascontiguousarray(alpha), alpha_ucn=ucn, beta=W.beta.copy())


def _dec(device, kind, q=5):
    if ("dec", kind, q) not in _cache:
        from ldpc_error_floor_amd.decoder import NMSDecoder
        proto, _, _ = _graph()
        _cache["dec", kind, q] = NMSDecoder(proto, 24, _weights(kind), 2, q, device=device)
    return _cache["dec", kind, q]


def _llr(device, n, q=5):
    """The first n rows of one stream per grid, never written to."""
    if ("llr", q) not in _cache:
        _cache["llr", q] = _dec(device, "c2", q).awgn(max(SIZES), _graph()[2], seed=SEED, offset=OFFSET)
    return _cache["llr", q][:n]


def _set(monkeypatch, name, value):
    if value is None:
        monkeypatch.delenv(name, raising=False)
    else:
        monkeypatch.setenv(name, value)


def _env(monkeypatch, afix=None, grid=None, frozen=None):
    _set(monkeypatch, "LDPC_BS_AFIX", afix)
    _set(monkeypatch, "LDPC_BS_GRID", grid)
    _set(monkeypatch, "LDPC_BS_FROZEN", frozen)


def _outputs(dec, llr, T, kernel="fused", afix=None, frozen=None, word=True, name=NAME):
    """Everything the bit-sliced builds return, as numpy.  afix / frozen: what last_afix() /
    last_frozen() must say (None: not asserted, another kernel).  The export and word builds are
    generic either way and take the same path as the decode build."""
    r = dec.decode(llr, T=T, app=False, counters=True, flags=True, kernel=kernel, iter_wrong=True)
    if afix is not None:
        assert dec.last_kernel() == name, dec.last_kernel()
        assert dec.last_afix() == afix, (dec.last_afix(), afix)
    if frozen is not None:
        assert dec.last_frozen() == frozen, (dec.last_frozen(), frozen)
    h = dec.decode(llr, T=T, app=False, hard=True, counters=True, kernel=kernel)
    if afix is not None:
        assert dec.last_afix() == afix, ("export", dec.last_afix(), afix)
    out = dict(counters=r.counters, flags=r.flags, iter_wrong=r.iter_wrong, hard=h.hard, hard_counters=h.counters)
    if kernel == "fused" and word:
        w = dec.decode(llr, T=T, hard_last=True, word_flags=True, counters=True, flags=True)
        if afix is not None:
            assert dec.last_afix() == afix, ("word", dec.last_afix(), afix)
        out.update(word=w.hard_last, word_flags=w.word_flags, word_counters=w.counters, word_frame_flags=w.flags)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _same(got, want, what):
    assert sorted(got) == sorted(want)
    for k in want:
        assert np.array_equal(got[k], want[k]), (k,) + what


def _reference(device, monkeypatch, kind, n, T):
    """The LDS-table path (LDPC_BS_AFIX=0) with the default build and grid, computed once per shape
    and shared; the larger batch of each T is checked against flood."""
    if ("ref", kind, n, T) not in _cache:
        dec = _dec(device, kind)
        _env(monkeypatch, afix="0")
        old = _outputs(dec, _llr(device, n), T, afix=False, frozen=True)
        if n == max(SIZES):
            fl = _outputs(dec, _llr(device, n), T, kernel="flood")
            for k in fl:
                assert np.array_equal(old[k], fl[k]), (k, kind, n, T)
            assert np.array_equal(old["word"].view(np.uint32), old["hard"][T - 1].view(np.uint32)), (kind, n, T)
        # (not trivial: iteration 0 leaves frame errors)
        assert old["iter_wrong"][0].any(), (kind, n, T)
        _cache["ref", kind, n, T] = old
    return _cache["ref", kind, n, T]


@pytest.mark.parametrize("T", ITERS)
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("build", ["frozen", "generic"])
@pytest.mark.parametrize("kind", ["c2", "synth"])
def test_fixed_tables_equal_lds_tables(cuda_device, monkeypatch, kind, build, n, grid, T):
    dec = _dec(cuda_device, kind)
    ref = _reference(cuda_device, monkeypatch, kind, n, T)
    fz = build == "frozen"
    env = None if fz else "0"
    _env(monkeypatch, afix="0", grid=grid, frozen=env)
    old = _outputs(dec, _llr(cuda_device, n), T, afix=False, frozen=fz)
    _env(monkeypatch, afix=None, grid=grid, frozen=env)
    new = _outputs(dec, _llr(cuda_device, n), T, afix=True, frozen=fz)
    _env(monkeypatch, afix="1", grid=grid, frozen=env)
    on = dec.decode(_llr(cuda_device, n), T=T, app=False, counters=True, flags=True, iter_wrong=True)
    assert dec.last_afix()
    _same(old, ref, ("LDS tables vs reference", kind, build, n, grid, T))
    _same(new, ref, ("fixed tables vs reference", kind, build, n, grid, T))
    assert np.array_equal(on.counters.cpu().numpy(), ref["counters"])


def test_synthetic_weights_exercise_the_tables(cuda_device, monkeypatch):
    """The synthetic set is not decoded the same whatever the table: with the iterations of
    alpha <= 0 (all messages zero) it leaves other frame errors than the trained set."""
    a = _reference(cuda_device, monkeypatch, "c2", 167, 20)
    b = _reference(cuda_device, monkeypatch, "synth", 167, 20)
    assert not np.array_equal(a["iter_wrong"], b["iter_wrong"])
    assert not np.array_equal(a["hard"], b["hard"])


@pytest.mark.parametrize("case", ["rows", "ucn", "q4"])
def test_other_requests_keep_the_lds_tables(cuda_device, monkeypatch, case):
    """Per-row alpha (the same instance, one table per row), UCN weights (the UCN instance) and
    q = 4 (magnitudes saturate at 7: no fixed set): the switch changes nothing, last_afix() is
    False, and the results equal flood's."""
    kind, q = ("c2", 4) if case == "q4" else (case, 5)
    dec = _dec(cuda_device, kind, q)
    n, T = 167, 20
    llr = _llr(cuda_device, n, q)
    name = dec.kernel_info()[1]
    assert name.startswith("bsl[p32,w9,d15,v6,l4"), name
    assert name.endswith(",ucn]") == (case == "ucn"), name
    word = case == "rows"
    _env(monkeypatch, afix="0")
    old = _outputs(dec, llr, T, afix=False, word=word, name=name)
    _env(monkeypatch, afix=None)
    new = _outputs(dec, llr, T, afix=False, word=word, name=name)
    _env(monkeypatch, afix="1")
    on = _outputs(dec, llr, T, afix=False, word=word, name=name)
    fl = _outputs(dec, llr, T, kernel="flood")
    _same(new, old, (case,))
    _same(on, old, (case, "switch on"))
    for k in fl:
        assert np.array_equal(new[k], fl[k]), (k, case)


@pytest.mark.parametrize("T", [2, 20])
@pytest.mark.parametrize("kind", ["c2", "synth"])
def test_in_kernel_channel_and_int8_take_the_fixed_tables(cuda_device, monkeypatch, kind, T):
    """decode_awgn (the in-prologue channel builds, frozen and generic) and decode_q8 (the int8
    builds) equal the float decode's reference and follow the switch."""
    dec = _dec(cuda_device, kind)
    sigma = _graph()[2]
    for n in SIZES:
        ref = _reference(cuda_device, monkeypatch, kind, n, T)
        for afix in (None, "0"):
            for frozen in (None, "0"):
                _env(monkeypatch, afix=afix, frozen=frozen)
                got = dec.decode_awgn(n, sigma, SEED, offset=OFFSET, T=T, counters=True, flags=True, iter_wrong=True)
                assert dec.last_kernel() == NAME + "+gen", dec.last_kernel()
                assert dec.last_afix() == (afix is None) and dec.last_frozen() == (frozen is None)
                for k in ("counters", "flags", "iter_wrong"):
                    assert np.array_equal(getattr(got, k).cpu().numpy(), ref[k]), ("awgn", k, kind, n, T, afix, frozen)
            _env(monkeypatch, afix=afix)
            q8 = dec.quantize_q8(_llr(cuda_device, n))
            got = dec.decode_q8(q8, T=T, counters=True, flags=True, iter_wrong=True)
            assert dec.last_kernel().startswith(NAME), dec.last_kernel()
            assert dec.last_afix() == (afix is None)
            for k in ("counters", "flags", "iter_wrong"):
                assert np.array_equal(getattr(got, k).cpu().numpy(), ref[k]), ("q8", k, kind, n, T, afix)
            w = dec.decode_q8(q8, T=T, hard_last=True, word_flags=True, counters=True, flags=True)
            assert dec.last_afix() == (afix is None)
            assert np.array_equal(w.hard_last.cpu().numpy(), ref["word"]), ("q8 word", kind, n, T, afix)


def test_80211n_is_untouched(cuda_device, monkeypatch):
    """802.11n decodes on a UCN-compiled instance, which has no fixed-table check phase: one small
    decode equals flood with the switch either way, and last_afix() is False."""
    from ldpc_error_floor_amd.code import CodeParams, TannerGraph, load_base_graph
    from ldpc_error_floor_amd.decoder import NMSDecoder
    from ldpc_error_floor_amd.weights import expand_weights, read_weight_file
    proto = load_base_graph(os.path.join(DATA, "BaseGraph", "802_11n_N648_R56_z27.txt"))
    wf = read_weight_file(os.path.join(DATA, "Results", "WIFI", "Weights_Iter50.txt"))
    W = expand_weights((3, 3, 3), dict(wf.blocks), 24, TannerGraph(proto, 27))
    dec = NMSDecoder(proto, 27, W, 2, 5, device=cuda_device)
    llr = dec.awgn(33, float(CodeParams(proto, 27).sigma(4.5)), seed=SEED, offset=OFFSET)
    name = dec.kernel_info()[1]
    assert name.startswith("bsl[p32,w12,d24,v4,l4"), name
    fl = _outputs(dec, llr, 24, kernel="flood")
    for afix in (None, "0"):
        _env(monkeypatch, afix=afix)
        got = _outputs(dec, llr, 24, afix=False, word=False, name=name)
        for k in fl:
            assert np.array_equal(got[k], fl[k]), (k, afix)
