"""The generic one-chunk bit-sliced instance {D 16, DV 8, LPC 4} (csrc/ldpc_bs_kernel.h, the
second entry of kBsInst; kernel name `bsl[p32,w<n>,d16,v8,l4]`) against the CPU oracle, bit for
bit (GPU only).  It serves every one-chunk, non-UCN graph past the wman instance (check degree
16, or variable degree 7-8), and none of the tuned workloads or fixture graphs: the synthetic
graphs of tests/_helpers.py reach it.

  dense16 z = 16   4 x 16, all edges: check degree 16, 256 variables and 4 x 64 check lanes on 4
                   waves, no idle check lane (cn_dmin = the check degree)
  vdeg8   z = 21   8 x 16, variable degrees 8 / 3, check degrees 3 .. 9: 336 variables, 672
                   check lanes on 11 waves, the last check chunk ragged (cn_dmin = 0)
  dense16 z = 4    256 edges, 5 KB of slots: less than the 4 * AWGN_TAB_W bytes the in-prologue
                   channel's tables need, so decode_awgn generates the channel into HBM

QMS is integer arithmetic on a grid and oracle.nms_oracle restates it exactly, so every
comparison is equality, of `fused` (the bit-sliced kernel, its export build, its v5 fixup and the
v5 kernel for APP) and of `flood` alike: the two GPU kernels share the host graph tables and the
weight upload, so comparing them with each other would miss a fault common to both.

LLRs are dec.awgn's (Philox, on the q-bit grid).  One oracle run per (graph, q, weights, SNR) of
B = 167 codewords and 20 iterations is shared: codeword b of iteration t depends on neither B
nor T, so a case of (B, T) is its [:T, :B] corner (B = 1: the first codeword whose frame error
changes between the first and the last iteration).  Every case first checks the oracle's own
output so that it cannot pass trivially: the frames wrong at the last iteration are more than 0
and fewer than B, and their count differs from iteration 0's.  One codeword cannot be "some but
not all", and one iteration has no earlier one, so with B = 1 the first condition and with T = 1
the second is taken on the shared 167-codeword run instead.  The SNR is 4.0 dB except where that
leaves a condition empty on vdeg8 (rate 1/2): 6.5 dB for one iteration (at 4.0 dB all 167 are
still wrong after it) and 2.5 dB for 20 (at 4.0 dB at most 2 of 167 stay wrong)."""
import itertools
import os

import numpy as np
import pytest

from _helpers import (awgn_tab_w, counters_from_app, dense16, flags_from_app, row_col_weights,
                      vdeg8)
from conftest import ROOT
from oracle import nms_oracle

pytestmark = pytest.mark.gpu
DATA = os.path.join(ROOT, "ldpc_error_floor_amd", "data")
BMAX, TMAX = 167, 20          # six packs, the last of 7 codewords
SEED, OFFSET = 29, 4099       # the channel's seed and first global codeword index
GRAPH_SEED, WEIGHT_SEED = 1, 7
GRAPHS = {"dense16": (dense16, 16), "vdeg8": (vdeg8, 21), "dense16z4": (dense16, 4)}
GENERIC = "d16,v8,l4"
QS = [5, -5, 4, 3]
WEIGHTS = ["flat", "rowcol"]
BS = [1, 33, 167]
TS = [1, 3, 20]
GRIDS = ["1", "2", "4", "0", None]     # LDPC_BS_GRID; None: unset, the resident workgroups
_cache = {}


def _snr(gname, T):
    if gname == "vdeg8":
        return 6.5 if T == 1 else 2.5 if T == TMAX else 4.0
    return 4.0


def _pairwise_cases():
    """(q, weights, B, T): every (q, weights) pair with two (B, T) pairs each, dealt so that all
    nine (B, T) pairs, every (q, B), (q, T), (weights, B) and (weights, T) pair occur."""
    out = [(5, "flat", 33, 3)]             # (the narrow case the instance first ran on a GPU)
    for i, (q, wk) in enumerate(itertools.product(QS, WEIGHTS)):
        a = i + i // 3
        out.append((q, wk, BS[i % 3], TS[a % 3]))
        out.append((q, wk, BS[(i + 1) % 3], TS[(a + 2) % 3]))
    out.append((5, "flat", 167, 20))       # (the largest case at the tuned kernels' q and weights)
    out.append((3, "rowcol", 1, 3))
    return out


CASES = _pairwise_cases()


def _graph(gname):
    if ("graph", gname) not in _cache:
        from ldpc_error_floor_amd.code import CodeParams, TannerGraph
        fn, z = GRAPHS[gname]
        proto = fn(GRAPH_SEED, z)
        _cache["graph", gname] = (proto, z, TannerGraph(proto, z), CodeParams(proto, z),
                                  nms_oracle.lifted_edges(proto, z))
    return _cache["graph", gname]


def _weights(tg, wk):
    from ldpc_error_floor_amd.weights import flat_weights
    return flat_weights(tg, TMAX, 0.75, 1.0) if wk == "flat" else row_col_weights(tg, TMAX, WEIGHT_SEED)


def _dec(device, gname, q, wk):
    """One decoder per (graph, q, weights); the planner must give it the generic instance."""
    key = ("dec", gname, q, wk)
    if key not in _cache:
        from ldpc_error_floor_amd.decoder import NMSDecoder
        proto, z, tg, _, _ = _graph(gname)
        dec = NMSDecoder(proto, z, _weights(tg, wk), 2, q, device=device)
        name = dec.kernel_info()[1]
        assert name.startswith("bsl[p32,") and GENERIC in name, name
        _cache[key] = dec
    return _cache[key]


def _llr(dec, gname, q, snr):
    """dec.awgn's LLRs of the 167 codewords, on the device and on the host."""
    key = ("llr", gname, q, snr)
    if key not in _cache:
        x = dec.awgn(BMAX, float(_graph(gname)[3].sigma(snr)), seed=SEED, offset=OFFSET)
        _cache[key] = (x, x.cpu().numpy())
    return _cache[key]


def _oracle(gname, q, W, llr, key):
    """The oracle's APP / hard decisions / syndromes [TMAX, 167, .] and wrong frames [TMAX, 167]."""
    if key not in _cache:
        proto, z, _, _, g = _graph(gname)
        out = nms_oracle.decode(llr, proto, z, W.alpha, W.alpha_ucn, W.beta, TMAX, 2, q, graph=g)
        out["wrong"] = (out["app"] >= 0).any(axis=2)
        _cache[key] = out
    return _cache[key]


def _not_trivial(wrong, shared):
    """The conditions of the module docstring on a case's wrong frames [T, B] (`shared`: those
    of the 167-codeword run it is a corner of)."""
    T, B = wrong.shape
    last = int(wrong[-1].sum())
    first_cond = wrong if B > 1 else shared[:T]
    n = int(first_cond[-1].sum())
    assert 0 < n < first_cond.shape[1], (n, first_cond.shape)
    second = wrong if T > 1 else shared
    assert int(second[-1].sum()) != int(second[0].sum()), (T, B, last)


def _expect(dec, gname, q, wk, B, T, llr=None, tag=""):
    """(LLR tensor [B, n], the oracle's outputs cut to [T, B]) of one case, checked not trivial.
    `llr`: (tensor, numpy) of 167 codewords instead of the channel's (`tag` names them)."""
    snr = _snr(gname, T)
    x, xh = llr if llr is not None else _llr(dec, gname, q, snr)
    ref = _oracle(gname, q, dec.weights, xh, ("oracle", gname, q, wk, snr, tag))
    b0 = 0
    if B == 1:       # a codeword whose frame error changes over the iterations (T = 1: any)
        b0 = int(np.argmax(ref["wrong"][0] != ref["wrong"][T - 1]))
    want = {k: v[:T, b0:b0 + B] for k, v in ref.items()}
    _not_trivial(want["wrong"], ref["wrong"])
    return x[b0:b0 + B], want


def _is_generic(name):
    return name.startswith("bsl[p32,") and GENERIC in name


def _check_counters_only(dec, llr, T, want, kernel, is_kernel=_is_generic):
    B = llr.shape[0]
    r = dec.decode(llr, T=T, app=False, counters=True, flags=True, kernel=kernel, iter_wrong=True)
    name = dec.last_kernel()
    if kernel == "fused":
        assert is_kernel(name), name
    assert np.array_equal(r.counters.cpu().numpy(), counters_from_app(want["app"])), (kernel, name)
    assert np.array_equal(r.flags.cpu().numpy(), flags_from_app(want["app"])), (kernel, name)
    assert np.array_equal(r.frame_errors(B), want["wrong"]), (kernel, name)


def _check_export(dec, llr, T, want, kernel, is_kernel=_is_generic):
    from ldpc_error_floor_amd.decoder import unpack_bits
    r = dec.decode(llr, T=T, app=False, hard=True, synd=True, counters=True, kernel=kernel)
    name = dec.last_kernel()
    if kernel == "fused":
        assert is_kernel(name), name
    assert np.array_equal(unpack_bits(r.hard.cpu().numpy(), dec.n_vars), want["hard"]), (kernel, name)
    assert np.array_equal(unpack_bits(r.synd.cpu().numpy(), dec.n_checks), want["synd"]), (kernel, name)
    assert np.array_equal(r.counters.cpu().numpy(), counters_from_app(want["app"])), (kernel, name)


def _check_app(dec, llr, T, want, kernel):
    r = dec.decode(llr, T=T, app=True, kernel=kernel)
    assert np.array_equal(r.app.cpu().numpy(), want["app"]), (kernel, dec.last_kernel())


def _check_all(dec, llr, T, want, is_kernel=_is_generic):
    """Every output of `fused`: the counters-only build, the export build and the APP."""
    _check_counters_only(dec, llr, T, want, "fused", is_kernel)
    _check_export(dec, llr, T, want, "fused", is_kernel)
    _check_app(dec, llr, T, want, "fused")


def _set_grid(monkeypatch, grid):
    if grid is None:
        monkeypatch.delenv("LDPC_BS_GRID", raising=False)
    else:
        monkeypatch.setenv("LDPC_BS_GRID", grid)


@pytest.mark.parametrize("q,wk,B,T", CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("gname", ["dense16", "vdeg8"])
def test_counters_only_equals_oracle(cuda_device, gname, q, wk, B, T):
    """counters, frame flags and per-iteration frame errors of the bit-sliced kernel and of
    flood, each against the oracle (the first GPU run of the instance was dense16, q = 5, flat
    weights, B = 33, T = 3, alone)."""
    dec = _dec(cuda_device, gname, q, wk)
    llr, want = _expect(dec, gname, q, wk, B, T)
    _check_counters_only(dec, llr, T, want, "fused")
    _check_counters_only(dec, llr, T, want, "flood")


def test_the_case_list_covers_every_pair():
    pairs = lambda i, j: {(c[i], c[j]) for c in CASES}                    # noqa: E731
    assert pairs(2, 3) == set(itertools.product(BS, TS))
    assert pairs(0, 1) == set(itertools.product(QS, WEIGHTS))
    for i, a in ((0, QS), (1, WEIGHTS)):
        assert pairs(i, 2) == set(itertools.product(a, BS)) and pairs(i, 3) == set(itertools.product(a, TS))


@pytest.mark.parametrize("wk,B,T", [("flat", 167, 20), ("rowcol", 33, 3)])
@pytest.mark.parametrize("gname", ["dense16", "vdeg8"])
def test_export_build_equals_oracle(cuda_device, gname, wk, B, T):
    """hard=True, synd=True at q = 5: every iteration's hard decisions and syndromes."""
    dec = _dec(cuda_device, gname, 5, wk)
    llr, want = _expect(dec, gname, 5, wk, B, T)
    _check_export(dec, llr, T, want, "fused")
    _check_export(dec, llr, T, want, "flood")


@pytest.mark.parametrize("q,wk,B,T", [(5, "flat", 167, 20), (-5, "rowcol", 33, 3), (3, "rowcol", 167, 3)])
@pytest.mark.parametrize("gname", ["dense16", "vdeg8"])
def test_app_equals_oracle(cuda_device, gname, q, wk, B, T):
    """decode(app=True): the v5 kernel where it serves the graph, and flood."""
    dec = _dec(cuda_device, gname, q, wk)
    llr, want = _expect(dec, gname, q, wk, B, T)
    _check_app(dec, llr, T, want, "flood")
    if not dec.supports("fused", T):
        pytest.skip("no fused kernel serves this graph: flood alone compared")
    _check_app(dec, llr, T, want, "fused")


@pytest.mark.parametrize("T", [3, 20])
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"grid{g}")
@pytest.mark.parametrize("wk", WEIGHTS)
@pytest.mark.parametrize("gname", ["dense16", "vdeg8"])
def test_pack_loop_equals_oracle(cuda_device, gname, wk, grid, T, monkeypatch):
    """Six packs (the last of 7 codewords) through 1, 2, 4, 6 and the resident workgroups."""
    dec = _dec(cuda_device, gname, 5, wk)
    llr, want = _expect(dec, gname, 5, wk, BMAX, T)
    _set_grid(monkeypatch, grid)
    _check_all(dec, llr, T, want)


@pytest.mark.parametrize("grid", ["1", "0"])
@pytest.mark.parametrize("gname", ["dense16", "vdeg8"])
def test_off_grid_llrs_inside_a_pack_sequence(cuda_device, gname, grid, monkeypatch):
    """One LLR of pack 2 moved off the q-grid and one of the ragged last pack set to 30.0 (past
    the grid's largest value): those packs go to the v5 fixup, on a graph of check degree up to
    16, and the result equals the oracle's on the modified LLRs."""
    T = TMAX
    dec = _dec(cuda_device, gname, 5, "rowcol")
    x, _ = _llr(dec, gname, 5, _snr(gname, T))
    if ("offgrid", gname) not in _cache:
        y = x.clone()
        y[2 * 32 + 5, 17] += 0.1
        y[5 * 32 + 3, 40] = 30.0
        _cache["offgrid", gname] = (y, y.cpu().numpy())
    llr, want = _expect(dec, gname, 5, "rowcol", BMAX, T, llr=_cache["offgrid", gname], tag="offgrid")
    _set_grid(monkeypatch, grid)
    # with the fixup switched off the bit-sliced kernel leaves exactly those two packs' frame
    # flags untouched, and every other pack's are already the oracle's
    import torch
    monkeypatch.setenv("LDPC_BS_FIXUP", "0")
    flags = torch.full((BMAX,), 255, dtype=torch.uint8, device=cuda_device)
    dec.decode(llr, T=T, app=False, counters=True, flags=flags, kernel="fused", iter_wrong=True)
    assert _is_generic(dec.last_kernel()), dec.last_kernel()
    f = flags.cpu().numpy()
    fixed = np.r_[64:96, 160:BMAX]
    keep = np.r_[0:64, 96:160]
    assert np.all(f[fixed] == 255)
    assert np.array_equal(f[keep], flags_from_app(want["app"])[keep])
    monkeypatch.delenv("LDPC_BS_FIXUP")
    _check_all(dec, llr, T, want)


@pytest.mark.parametrize("T", [3, 20])
@pytest.mark.parametrize("q,wk", [(5, "rowcol"), (4, "flat")])
@pytest.mark.parametrize("gname", ["dense16", "vdeg8", "dense16z4"])
def test_in_kernel_channel_equals_oracle(cuda_device, gname, q, wk, T):
    """decode_awgn against the oracle on dec.awgn's LLRs of the same seed and offset.  The
    channel is generated in the kernel's prologue ("+gen") where the slot region holds the
    sampler's tables, 4 * AWGN_TAB_W bytes (bs_q8_ok): 20 KB and 24 KB of slots do, the 5 KB of
    dense16 at z = 4 do not, and there the channel goes through HBM."""
    dec = _dec(cuda_device, gname, q, wk)
    _, want = _expect(dec, gname, q, wk, BMAX, T)
    _, z, tg, cp, _ = _graph(gname)
    in_kernel = 20 * tg.E * z >= 4 * awgn_tab_w()          # (20 B per edge slot)
    assert in_kernel == (gname != "dense16z4")
    assert dec.generates_channel_in_kernel(T) == in_kernel
    r = dec.decode_awgn(BMAX, float(cp.sigma(_snr(gname, T))), SEED, offset=OFFSET, T=T, counters=True,
                        flags=True, iter_wrong=True)
    name = dec.last_kernel()
    assert _is_generic(name) and name.endswith("+gen") == in_kernel, name
    assert np.array_equal(r.counters.cpu().numpy(), counters_from_app(want["app"])), name
    assert np.array_equal(r.flags.cpu().numpy(), flags_from_app(want["app"])), name
    assert np.array_equal(r.frame_errors(BMAX), want["wrong"]), name


@pytest.mark.parametrize("grid", ["1", "4"])
def test_wman_lpc2_instance_under_the_pack_loop(cuda_device, grid, monkeypatch):
    """The wman instance with two lanes per check (LDPC_BS_LPC=2; `d15,v6,l2`), which the pack
    loop serves too: per-row weights, q = 4, B = 167, T = 20."""
    from ldpc_error_floor_amd.code import CodeParams, TannerGraph, load_base_graph
    from ldpc_error_floor_amd.decoder import NMSDecoder
    monkeypatch.setenv("LDPC_BS_LPC", "2")
    is_lpc2 = lambda name: name.startswith("bsl[p32,") and name.endswith("d15,v6,l2]")   # noqa: E731
    if "wman" not in _cache:
        proto = load_base_graph(os.path.join(DATA, "BaseGraph", "wman_N0576_R34_z24.txt"))
        W = row_col_weights(TannerGraph(proto, 24), TMAX, WEIGHT_SEED)
        dec = NMSDecoder(proto, 24, W, 2, 4, device=cuda_device)
        llr = dec.awgn(BMAX, float(CodeParams(proto, 24).sigma(3.5)), seed=SEED, offset=OFFSET)
        out = nms_oracle.decode(llr.cpu().numpy(), proto, 24, W.alpha, None, W.beta, TMAX, 2, 4)
        out["wrong"] = (out["app"] >= 0).any(axis=2)
        _not_trivial(out["wrong"], out["wrong"])
        _cache["wman"] = (dec, llr, out)
    dec, llr, want = _cache["wman"]
    assert is_lpc2(dec.kernel_info()[1]), dec.kernel_info()
    _set_grid(monkeypatch, grid)
    _check_all(dec, llr, TMAX, want, is_lpc2)
