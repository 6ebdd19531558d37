"""The pack loop's tickets (csrc/ldpc_bs_kernel.h, BS_RED_NEXT; GPU only): a workgroup of the wman
bit-sliced kernel takes pack blockIdx.x first and every later pack from a counter, so which
workgroup decodes which pack depends on timing.  Every output is indexed by pack or summed by
integer atomics, so whatever the grid the results must equal, bit for bit, those of the fixed
stride (LDPC_BS_TICKETS=0) and of one workgroup per pack (LDPC_BS_GRID=0), which is checked against
the flood kernel once per shape.

  B = 167 and 325: 6 and 11 packs, the last ragged (7 and 5 codewords).  Grids 2 and 3 with 11 packs
  are the smallest cases in which workgroups race for tickets and take unequal shares.
  LDPC_BS_GRID = 1, 2, 3, unset (unset: min(packs, resident) = one workgroup per pack, no ticket).
  T = 1, 3, 20.
  "Everything": counters, frame flags, iter_wrong (the decode build), every iteration's hard
  decisions and their counters (the export build), the word mode's rows, flags and counters.
  The main comparison runs with the geometry-frozen decode build and with the generic one
  (LDPC_BS_FROZEN=0), on every size, grid and T.

What these tests cannot tell: that a ticket was taken at all.  The outputs do not depend on the
order of the packs, so a build that fell back to the stride would pass every case here.  That the
path is live shows only in a stamp build's per-workgroup records (tools/wg_tail.py; the committed
dump profiles/r10/wg_C2_tickets.txt has 38 to 48 packs per workgroup where the stride gives 42 or
43).
"""
import os

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
DATA = os.path.join(ROOT, "ldpc_error_floor_amd", "data")
SIZES = [167, 325]
SNR = 3.5
SEED, OFFSET = 29, 4099
GRIDS = ["1", "2", "3", None]           # LDPC_BS_GRID; None: unset
ITERS = [1, 3, 20]
NAME = "bsl[p32,w9,d15,v6,l4]"
_cache = {}


def _wman(device):
    """wman N576 z24 with the trained C2 weights, QMS q = 5 (one decoder for the module)."""
    if "dec" not in _cache:
        from ldpc_error_floor_amd.code import CodeParams, TannerGraph, load_base_graph
        from ldpc_error_floor_amd.decoder import NMSDecoder
        from ldpc_error_floor_amd.weights import expand_weights, read_weight_file
        proto = load_base_graph(os.path.join(DATA, "BaseGraph", "wman_N0576_R34_z24.txt"))
        g = TannerGraph(proto, 24)
        wf = read_weight_file(os.path.join(DATA, "Weights", "C0_wman_N0576_R34_z24_Opt_Weight_End20.txt"))
        W = expand_weights((3, 0, 3), {0: wf.blocks[0], 2: wf.blocks[2]}, 20, g)
        dec = NMSDecoder(proto, 24, W, 2, 5, device=device)
        assert dec.kernel_info()[1] == NAME, dec.kernel_info()
        _cache["dec"] = dec
        _cache["sigma"] = float(CodeParams(proto, 24).sigma(SNR))
    return _cache["dec"], _cache["sigma"]


def _llr(device, n):
    """The first n rows of one stream (so B = 167 is a corner of B = 325), never written to."""
    dec, sigma = _wman(device)
    if "llr" not in _cache:
        _cache["llr"] = dec.awgn(max(SIZES), sigma, seed=SEED, offset=OFFSET)
    return _cache["llr"][:n]


def _set(monkeypatch, name, value):
    if value is None:
        monkeypatch.delenv(name, raising=False)
    else:
        monkeypatch.setenv(name, value)


def _env(monkeypatch, grid, tickets=None, frozen=None):
    _set(monkeypatch, "LDPC_BS_GRID", grid)
    _set(monkeypatch, "LDPC_BS_TICKETS", tickets)
    _set(monkeypatch, "LDPC_BS_FROZEN", frozen)


def _outputs(dec, llr, T, kernel="fused", frozen=None, word=True):
    """Everything the bit-sliced builds of the pack loop return, as numpy.  frozen: what
    last_frozen() must say of the decode build (None: not asserted, another kernel); word: with
    the word mode's outputs (it declines inputs off the grid)."""
    r = dec.decode(llr, T=T, app=False, counters=True, flags=True, kernel=kernel, iter_wrong=True)
    if frozen is not None:
        assert dec.last_kernel() == NAME, dec.last_kernel()
        assert dec.last_frozen() == frozen, (dec.last_frozen(), frozen)
    h = dec.decode(llr, T=T, app=False, hard=True, counters=True, kernel=kernel)
    out = dict(counters=r.counters, flags=r.flags, iter_wrong=r.iter_wrong, hard=h.hard, hard_counters=h.counters)
    if kernel == "fused" and word:
        w = dec.decode(llr, T=T, hard_last=True, word_flags=True, counters=True, flags=True)
        out.update(word=w.hard_last, word_flags=w.word_flags, word_counters=w.counters, word_frame_flags=w.flags)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _reference(device, monkeypatch, n, T, key="ref", llr=None, word=True):
    """One workgroup per pack (LDPC_BS_GRID=0: no ticket is taken), checked against flood, computed
    once per shape and shared."""
    dec, _ = _wman(device)
    if (key, n, T) not in _cache:
        _env(monkeypatch, "0")
        x = _llr(device, n) if llr is None else llr
        g0 = _outputs(dec, x, T, frozen=True, word=word)
        fl = _outputs(dec, x, T, kernel="flood")
        for k in fl:
            assert np.array_equal(g0[k], fl[k]), (k, n, T)
        if word:
            assert np.array_equal(g0["word"].view(np.uint32), g0["hard"][T - 1].view(np.uint32)), (n, T)
        # (not trivial, and a skipped pack would show: iteration 0 leaves errors in every pack)
        assert (g0["iter_wrong"][0] != 0).all(), (n, T)
        _cache[key, n, T] = g0
    return _cache[key, n, T]


def _same(got, want, what):
    assert sorted(got) == sorted(want)
    for k in want:
        assert np.array_equal(got[k], want[k]), (k,) + what


@pytest.mark.parametrize("T", ITERS)
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("build", ["frozen", "generic"])
def test_tickets_equal_stride_and_one_workgroup_per_pack(cuda_device, monkeypatch, build, n, grid, T):
    """The main comparison, with the geometry-frozen decode build and, under LDPC_BS_FROZEN=0, with
    the generic one (the export and word builds are generic either way); last_frozen() is asserted
    for each decode."""
    dec, _ = _wman(cuda_device)
    ref = _reference(cuda_device, monkeypatch, n, T)
    fz = build == "frozen"
    env = None if fz else "0"
    _env(monkeypatch, grid, tickets="0", frozen=env)
    stride = _outputs(dec, _llr(cuda_device, n), T, frozen=fz)
    _env(monkeypatch, grid, tickets="1", frozen=env)
    got = _outputs(dec, _llr(cuda_device, n), T, frozen=fz)
    _same(stride, ref, ("stride vs reference", build, n, grid, T))
    _same(got, ref, ("tickets vs reference", build, n, grid, T))
    _same(got, stride, ("tickets vs stride", build, n, grid, T))


@pytest.mark.parametrize("grid", GRIDS[:3])
@pytest.mark.parametrize("n", SIZES)
def test_every_pack_exactly_once(cuda_device, monkeypatch, n, grid):
    """No flag of a valid frame keeps its prefilled 255 and none past the batch is written; the
    host zeroes iter_wrong before every decode, so its sentinel is zero: iteration 0's word of every
    pack is nonzero in the reference (_reference asserts it), and no pack's may be zero here (no
    pack skipped).  The counters equal the reference (a pack decoded twice would add its counts
    twice)."""
    import torch
    dec, _ = _wman(cuda_device)
    T = 20
    ref = _reference(cuda_device, monkeypatch, n, T)
    _env(monkeypatch, grid, tickets="1")
    npk = (n + 31) // 32
    flags = torch.full((n + 32,), 255, dtype=torch.uint8, device=cuda_device)
    r = dec.decode(_llr(cuda_device, n), T=T, app=False, counters=True, flags=flags, iter_wrong=True)
    assert dec.last_kernel() == NAME and dec.last_frozen(), dec.last_kernel()
    f, w, counters = flags.cpu().numpy(), r.iter_wrong.cpu().numpy(), r.counters.cpu().numpy()
    assert w.shape == (T, npk)
    assert not (f[:n] == 255).any() and (f[n:] == 255).all()
    assert (w[0] != 0).all()
    assert np.array_equal(f[:n], ref["flags"])
    assert np.array_equal(w, ref["iter_wrong"])
    assert np.array_equal(counters, ref["counters"])


def test_back_to_back_launches(cuda_device, monkeypatch):
    """The ticket word is zeroed before every launch that uses it: three decodes in a row, then a
    different batch size, then a fixed-stride decode in between, on one decoder."""
    dec, _ = _wman(cuda_device)
    T = 20
    ref = {n: _reference(cuda_device, monkeypatch, n, T) for n in SIZES}
    _env(monkeypatch, "2", tickets="1")
    for _ in range(3):
        _same(_outputs(dec, _llr(cuda_device, 325), T, frozen=True), ref[325], ("repeat",))
    _same(_outputs(dec, _llr(cuda_device, 167), T, frozen=True), ref[167], ("other B",))
    _same(_outputs(dec, _llr(cuda_device, 325), T, frozen=True), ref[325], ("after other B",))
    _env(monkeypatch, "2", tickets="0")
    _same(_outputs(dec, _llr(cuda_device, 325), T, frozen=True), ref[325], ("stride in between",))
    _env(monkeypatch, "3", tickets="1")
    _same(_outputs(dec, _llr(cuda_device, 325), T, frozen=True), ref[325], ("after stride",))
    _same(_outputs(dec, _llr(cuda_device, 167), T, frozen=True), ref[167], ("last",))


@pytest.mark.parametrize("grid", GRIDS[:3])
@pytest.mark.parametrize("bad", [0, 5, 10], ids=["first", "middle", "last"])
def test_off_grid_pack_takes_a_ticket_too(cuda_device, monkeypatch, bad, grid):
    """One float LLR off the q-grid in pack `bad` of 11: the pack leaves through the loop's
    `continue`, whose condition reads the same ticket.  Without the v5 fixup that pack alone is
    marked and left untouched and the others equal the reference; with it the result is exact
    (the reference of the changed input: one workgroup per pack == flood)."""
    import torch
    dec, _ = _wman(cuda_device)
    T, n = 20, 325
    npk = (n + 31) // 32
    ref = _reference(cuda_device, monkeypatch, n, T)
    llr = _llr(cuda_device, n).clone()
    llr[bad * 32 + 3, 17] += 0.1
    lo, hi = bad * 32, min(bad * 32 + 32, n)
    keep = np.r_[0:lo, hi:n]
    cols = [p for p in range(npk) if p != bad]
    _env(monkeypatch, grid, tickets="1")
    monkeypatch.setenv("LDPC_BS_FIXUP", "0")
    flags = torch.full((n,), 255, dtype=torch.uint8, device=cuda_device)
    r = dec.decode(llr, T=T, app=False, counters=True, flags=flags, iter_wrong=True)
    assert dec.last_kernel() == NAME and dec.last_frozen(), dec.last_kernel()
    f, w = flags.cpu().numpy(), r.iter_wrong.cpu().numpy()
    assert np.all(f[lo:hi] == 255)
    assert np.array_equal(f[keep], ref["flags"][keep])
    assert np.array_equal(w[:, cols], ref["iter_wrong"][:, cols])
    monkeypatch.delenv("LDPC_BS_FIXUP")
    exact = _reference(cuda_device, monkeypatch, n, T, key=("offgrid", bad), llr=llr, word=False)
    _env(monkeypatch, grid, tickets="1")
    r = dec.decode(llr, T=T, app=False, counters=True, flags=True, iter_wrong=True)
    assert dec.last_kernel() == NAME and dec.last_frozen(), dec.last_kernel()
    h = dec.decode(llr, T=T, app=False, hard=True, counters=True)
    got = dict(counters=r.counters, flags=r.flags, iter_wrong=r.iter_wrong, hard=h.hard, hard_counters=h.counters)
    for k, v in got.items():
        assert np.array_equal(v.cpu().numpy(), exact[k]), (k, bad, grid)
    assert np.array_equal(r.flags.cpu().numpy()[keep], ref["flags"][keep])


@pytest.mark.parametrize("T", [3, 20])
@pytest.mark.parametrize("grid", ["1", "2", None])
def test_in_kernel_channel_with_tickets(cuda_device, monkeypatch, grid, T):
    """decode_awgn (the builds that generate the channel in the prologue, where the ticket is taken
    ahead of the sampler's tables) equals awgn + decode; frozen and generic."""
    dec, sigma = _wman(cuda_device)
    for n in SIZES:
        ref = _reference(cuda_device, monkeypatch, n, T)
        for frozen in (None, "0"):
            _env(monkeypatch, grid, tickets="1", frozen=frozen)
            got = dec.decode_awgn(n, sigma, SEED, offset=OFFSET, T=T, counters=True, flags=True, iter_wrong=True)
            assert dec.last_kernel() == NAME + "+gen", dec.last_kernel()
            assert dec.last_frozen() == (frozen is None)
            for k in ("counters", "flags", "iter_wrong"):
                assert np.array_equal(getattr(got, k).cpu().numpy(), ref[k]), (k, n, grid, T, frozen)
