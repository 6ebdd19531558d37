"""The pack loop of the one-chunk bit-sliced kernel (csrc/ldpc_bs_kernel.h, bs_loops; GPU only): a
workgroup decodes packs blockIdx.x, blockIdx.x + gridDim.x, ... on a grid of LDPC_BS_GRID
workgroups (default: those resident at once; 0: one workgroup per pack).  Whatever the grid, the
APP, hard decisions, frame flags, counters and per-iteration frame-error words must equal those
of one workgroup per pack and of the flood kernel bit for bit: B = 167 is six packs, the last of
7 codewords; grid 1 puts all six through one workgroup, grid 4 splits them 2 / 2 / 1 / 1."""
import os

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
DATA = os.path.join(ROOT, "ldpc_error_floor_amd", "data")
B = 167
SNR = 3.5
SEED, OFFSET = 29, 4099
GRIDS = ["1", "2", "4", "0"]
ITERS = [1, 3, 20]
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
        assert dec.kernel_info()[1].startswith("bsl[p32,w9,"), dec.kernel_info()
        _cache["dec"] = dec
        _cache["sigma"] = float(CodeParams(proto, 24).sigma(SNR))
    return _cache["dec"], _cache["sigma"]


def _llr(device, n=B):
    dec, sigma = _wman(device)
    if ("llr", n) not in _cache:
        _cache["llr", n] = dec.awgn(n, sigma, seed=SEED, offset=OFFSET)
    return _cache["llr", n]


def _outputs(dec, llr, T, kernel):
    """Everything a decode returns, as numpy: counters, flags, iter_wrong (counters-only build),
    the hard decisions of every iteration (the export build) and the APP."""
    r = dec.decode(llr, T=T, app=False, counters=True, flags=True, kernel=kernel, iter_wrong=True)
    name = dec.last_kernel()
    h = dec.decode(llr, T=T, app=False, hard=True, counters=True, kernel=kernel)
    a = dec.decode(llr, T=T, app=True, kernel=kernel)
    out = dict(counters=r.counters, flags=r.flags, iter_wrong=r.iter_wrong, hard=h.hard,
               hard_counters=h.counters, app=a.app)
    return {k: v.cpu().numpy() for k, v in out.items()}, name


def _reference(device, monkeypatch, T, key="ref", llr=None):
    """One workgroup per pack (LDPC_BS_GRID=0) and flood, computed once per T and shared."""
    dec, _ = _wman(device)
    if (key, T) not in _cache:
        monkeypatch.setenv("LDPC_BS_GRID", "0")
        x = _llr(device) if llr is None else llr
        g0, name = _outputs(dec, x, T, "fused")
        assert name.startswith("bsl["), name
        fl, _ = _outputs(dec, x, T, "flood")
        for k in g0:
            assert np.array_equal(g0[k], fl[k]), (k, T)
        _cache[key, T] = g0
    return _cache[key, T]


@pytest.mark.parametrize("T", ITERS)
@pytest.mark.parametrize("grid", GRIDS[:3])
def test_pack_loop_equals_one_workgroup_per_pack_and_flood(cuda_device, grid, T, monkeypatch):
    dec, _ = _wman(cuda_device)
    ref = _reference(cuda_device, monkeypatch, T)
    monkeypatch.setenv("LDPC_BS_GRID", grid)
    got, name = _outputs(dec, _llr(cuda_device), T, "fused")
    assert name.startswith("bsl["), name
    for k in ref:
        assert np.array_equal(got[k], ref[k]), (k, grid, T)


@pytest.mark.parametrize("T", ITERS)
def test_default_grid_equals_one_workgroup_per_pack(cuda_device, T, monkeypatch):
    """No LDPC_BS_GRID: the resident workgroups (more than six packs need: min(packs, resident))."""
    dec, _ = _wman(cuda_device)
    ref = _reference(cuda_device, monkeypatch, T)
    monkeypatch.delenv("LDPC_BS_GRID", raising=False)
    got, _ = _outputs(dec, _llr(cuda_device), T, "fused")
    for k in ref:
        assert np.array_equal(got[k], ref[k]), (k, T)


@pytest.mark.parametrize("grid", GRIDS)
def test_off_grid_pack_inside_a_workgroups_sequence(cuda_device, grid, monkeypatch):
    """One float LLR off the q-grid in pack 2 (with grids 1 and 2 neither the first nor the last
    pack of its workgroup): `bad` is set for that pack only -- with the v5 fixup switched off its
    frame flags stay untouched and every other pack's equal the reference -- the packs after it
    are unchanged, and with the fixup the result is exact."""
    import torch
    dec, _ = _wman(cuda_device)
    T = 20
    ref = _reference(cuda_device, monkeypatch, T)
    llr = _llr(cuda_device).clone()
    llr[2 * 32 + 5, 17] += 0.1
    monkeypatch.setenv("LDPC_BS_GRID", grid)
    monkeypatch.setenv("LDPC_BS_FIXUP", "0")
    flags = torch.full((B,), 255, dtype=torch.uint8, device=cuda_device)
    r = dec.decode(llr, T=T, app=False, counters=True, flags=flags, kernel="fused", iter_wrong=True)
    assert dec.last_kernel().startswith("bsl["), dec.last_kernel()
    f = r.flags.cpu().numpy()
    assert np.all(f[64:96] == 255)
    keep = np.r_[0:64, 96:B]
    assert np.array_equal(f[keep], ref["flags"][keep])
    iw = r.iter_wrong.cpu().numpy()
    cols = [0, 1, 3, 4, 5]
    assert np.array_equal(iw[:, cols], ref["iter_wrong"][:, cols])
    monkeypatch.delenv("LDPC_BS_FIXUP")
    exact = _reference(cuda_device, monkeypatch, T, key="offgrid", llr=llr)   # (grid 0 == flood)
    monkeypatch.setenv("LDPC_BS_GRID", grid)
    got, _ = _outputs(dec, llr, T, "fused")
    for k in exact:
        assert np.array_equal(got[k], exact[k]), (k, grid)
    assert np.array_equal(got["flags"][keep], ref["flags"][keep])


@pytest.mark.parametrize("T", [3, 20])
@pytest.mark.parametrize("grid", GRIDS)
def test_in_kernel_channel_with_pack_loop(cuda_device, grid, T, monkeypatch):
    """decode_awgn (the build that generates the channel in its prologue) on every grid equals
    awgn + decode (tests/test_gpu_channel.py checks it for one workgroup per pack)."""
    dec, sigma = _wman(cuda_device)
    ref = _reference(cuda_device, monkeypatch, T)
    monkeypatch.setenv("LDPC_BS_GRID", grid)
    got = dec.decode_awgn(B, sigma, SEED, offset=OFFSET, T=T, counters=True, flags=True, iter_wrong=True)
    assert dec.last_kernel().startswith("bsl[") and dec.last_kernel().endswith("+gen"), dec.last_kernel()
    for k in ("counters", "flags", "iter_wrong"):
        assert np.array_equal(getattr(got, k).cpu().numpy(), ref[k]), (k, grid, T)


@pytest.mark.parametrize("T", ITERS)
def test_one_pack_no_loop_back(cuda_device, T, monkeypatch):
    """B = 32 on grid 1: one full pack, the loop runs once."""
    dec, sigma = _wman(cuda_device)
    llr = _llr(cuda_device, 32)
    monkeypatch.setenv("LDPC_BS_GRID", "0")
    want, _ = _outputs(dec, llr, T, "fused")
    flood, _ = _outputs(dec, llr, T, "flood")
    monkeypatch.setenv("LDPC_BS_GRID", "1")
    got, name = _outputs(dec, llr, T, "fused")
    assert name.startswith("bsl["), name
    for k in want:
        assert np.array_equal(got[k], want[k]), (k, T)
        assert np.array_equal(got[k], flood[k]), (k, T)
    g8 = dec.decode_awgn(32, sigma, SEED, offset=OFFSET, T=T, counters=True, flags=True, iter_wrong=True)
    for k in ("counters", "flags", "iter_wrong"):
        assert np.array_equal(getattr(g8, k).cpu().numpy(), want[k]), (k, T)
