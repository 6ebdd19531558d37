"""The fold of the per-iteration frame-error words in the one-chunk bit-sliced kernels' T loop
(csrc/ldpc_bs_kernel.h; GPU only).  The variable phase of iteration t ORs every lane's frame-error
word into FLORW words of LDS; in iteration t + 1 one wave -- the last wave where it holds no check
lanes (802.11n), else wave 1 (wman, the synthetic graphs) -- reads them after its own check work,
zeroes them, and stores their OR as iteration t's word (`iter_wrong`) and into the "wrong at every
iteration" word (`counters[2]`, bit 0 of `flags`).  A fold left undone, done twice, or a zeroing
that comes too late shows in exactly these outputs, so `counters`, `flags` and `iter_wrong` are
compared bit for bit with oracle.nms_oracle (QMS is integer arithmetic, the oracle restates it
exactly), and the early-stop builds, which share the loop, with tests/_es_ref.py.

  T = 1 runs no fold, T = 2 exactly one, T = 3 is the first that folds words it zeroed before.
  B = 33 is two packs (the second of one codeword), B = 167 six (the last of 7).
  LDPC_BS_GRID 0 / 1 / 2 / unset: with 1 and 2 a workgroup decodes several packs in sequence, so a
  word left set or a fold left undone would leak into the next pack.

The LLRs are oracle.philox_oracle's (the stream tests/test_gpu_channel.py pins dec.awgn and
decode_awgn to), so every case's expectation is computed on the CPU: one oracle run per (graph,
SNR) of 167 codewords and the graph's largest T, of which a case (B, T) is the [:T, :B] corner.
Before a case looks at the GPU it asserts on the oracle's output that the fold is visible in it:
  (1) at least two iterations have different frame-error sets, each neither empty nor all B;
  (2) at least one frame is wrong at some iteration and right at the last.
Both need two iterations, so a T = 1 case takes them on the T = 2 corner of its own rows.  The
SNRs: wman 5.5 dB for T <= 2 (after one iteration 23 of the first 33 frames are wrong, after two
2) and 3.5 dB for T = 3 and 20 (167 -> 163 -> 123 -> ... -> 2 -> 0 wrong of 167); 802.11n with
the trained C3 weights (alpha' differs from alpha from iteration 20 on) 5.5 dB for T = 2 and
4.5 dB for T = 24; the synthetic vdeg8 graph 4.0 dB."""
import os

import numpy as np
import pytest

from _es_ref import es_reference
from _helpers import counters_from_app, flags_from_app, row_col_weights, vdeg8
from conftest import ROOT
from oracle import nms_oracle, philox_oracle

pytestmark = pytest.mark.gpu
DATA = os.path.join(ROOT, "ldpc_error_floor_amd", "data")
SEED, OFFSET = 29, 4099
BMAX = 167
GRIDS = ["0", "1", "2", None]          # LDPC_BS_GRID; None: unset, the resident workgroups
_cache = {}


def _wman():
    from ldpc_error_floor_amd.code import TannerGraph, load_base_graph
    from ldpc_error_floor_amd.weights import expand_weights, read_weight_file
    proto = load_base_graph(os.path.join(DATA, "BaseGraph", "wman_N0576_R34_z24.txt"))
    wf = read_weight_file(os.path.join(DATA, "Weights", "C0_wman_N0576_R34_z24_Opt_Weight_End20.txt"))
    W = expand_weights((3, 0, 3), {0: wf.blocks[0], 2: wf.blocks[2]}, 20, TannerGraph(proto, 24))
    return proto, 24, W, 20, lambda T: 5.5 if T <= 2 else 3.5


def _wifi():
    from ldpc_error_floor_amd.code import TannerGraph, load_base_graph
    from ldpc_error_floor_amd.weights import expand_weights, read_weight_file
    proto = load_base_graph(os.path.join(DATA, "BaseGraph", "802_11n_N648_R56_z27.txt"))
    wf = read_weight_file(os.path.join(DATA, "Results", "WIFI", "Weights_Iter50.txt"))
    W = expand_weights((3, 3, 3), dict(wf.blocks), 24, TannerGraph(proto, 27))
    differs = (W.alpha_ucn != W.alpha).reshape(24, -1).any(axis=1)
    assert not differs[:20].any() and differs[20:].all()       # alpha' switches on at t = 20
    return proto, 27, W, 24, lambda T: 5.5 if T <= 2 else 4.5


def _vdeg8():
    from ldpc_error_floor_amd.code import TannerGraph
    proto = vdeg8(1, 21)
    return proto, 21, row_col_weights(TannerGraph(proto, 21), 20, 7), 20, lambda T: 4.0


# (graph, the kernel that must serve it: the name's start, up to the options that depend on T)
CODES = {"wman": (_wman, "bsl[p32,w9,d15,v6,l4]"), "wifi": (_wifi, "bsl[p32,w12,d24,v4,l4"),
         "vdeg8": (_vdeg8, "bsl[p32,w11,d16,v8,l4]")}


def _code(name):
    if ("code", name) not in _cache:
        _cache["code", name] = CODES[name][0]()
    return _cache["code", name]


def _sigma(name, T):
    from ldpc_error_floor_amd.code import CodeParams
    proto, z, _, _, snr = _code(name)
    return float(CodeParams(proto, z).sigma(snr(T)))


def _oracle(name, T):
    """(LLRs [167, n], the oracle's outputs [TMAX, 167, .]) at the SNR of a T-iteration case:
    computed once, shared and left unchanged."""
    proto, z, W, tmax, snr = _code(name)
    key = ("oracle", name, snr(T))
    if key not in _cache:
        llr = philox_oracle.awgn_qms_llr(BMAX, proto.shape[1] * z, _sigma(name, T), SEED, OFFSET, 5)
        out = nms_oracle.decode(llr, proto, z, W.alpha, W.alpha_ucn, W.beta, tmax, 2, 5)
        out["wrong"] = (out["app"] >= 0).any(axis=2)
        _cache[key] = (llr, out)
    return _cache[key]


def _fold_visible(wrong):
    """The module docstring's conditions (1) and (2) on a case's frame errors [T, B]."""
    T, B = wrong.shape
    sets = {tuple(w) for w in wrong if 0 < int(w.sum()) < B}
    assert len(sets) >= 2, (T, B, wrong.sum(axis=1).tolist())
    assert (wrong.any(axis=0) & ~wrong[-1]).any(), (T, B, wrong.sum(axis=1).tolist())


def _expect(name, B, T):
    """(LLRs [B, n], the oracle's outputs [T, B, .]) of a case, the fold visible in them."""
    llr, out = _oracle(name, T)
    _fold_visible(out["wrong"][:max(T, 2), :B])
    return llr[:B], {k: v[:T, :B] for k, v in out.items()}


def _dec(device, name):
    if ("dec", name) not in _cache:
        from ldpc_error_floor_amd.decoder import NMSDecoder
        proto, z, W, _, _ = _code(name)
        dec = NMSDecoder(proto, z, W, 2, 5, device=device)
        assert dec.kernel_info()[1].startswith(CODES[name][1]), dec.kernel_info()
        _cache["dec", name] = dec
    return _cache["dec", name]


def _set_grid(monkeypatch, grid):
    if grid is None:
        monkeypatch.delenv("LDPC_BS_GRID", raising=False)
    else:
        monkeypatch.setenv("LDPC_BS_GRID", grid)


def _assert_outputs(r, want, B, what):
    got = r.counters.cpu().numpy(), r.flags.cpu().numpy(), r.frame_errors(B)
    ref = counters_from_app(want["app"]), flags_from_app(want["app"]), want["wrong"]
    print(what, "oracle wrong per iteration", want["wrong"].sum(axis=1).tolist(), "counters", ref[0].tolist(),
          "| got", got[0].tolist())
    for k, g, w in zip(("counters", "flags", "iter_wrong"), got, ref):
        assert np.array_equal(g, w), (what, k)


def _check_decode(device, name, B, T):
    import torch
    dec = _dec(device, name)
    llr, want = _expect(name, B, T)
    r = dec.decode(torch.from_numpy(llr).to(device), T=T, app=False, counters=True, flags=True, iter_wrong=True)
    assert dec.last_kernel().startswith(CODES[name][1]), dec.last_kernel()
    _assert_outputs(r, want, B, (name, "decode", B, T))


def _check_decode_awgn(device, name, B, T):
    dec = _dec(device, name)
    _, want = _expect(name, B, T)
    r = dec.decode_awgn(B, _sigma(name, T), SEED, offset=OFFSET, T=T, counters=True, flags=True, iter_wrong=True)
    assert dec.generates_channel_in_kernel(T)
    assert dec.last_kernel().startswith(CODES[name][1]) and dec.last_kernel().endswith("+gen"), dec.last_kernel()
    _assert_outputs(r, want, B, (name, "decode_awgn", B, T))


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"grid{g}")
@pytest.mark.parametrize("B", [33, 167])
@pytest.mark.parametrize("T", [1, 2, 3, 20])
def test_wman_decode(cuda_device, T, B, grid, monkeypatch):
    _set_grid(monkeypatch, grid)
    _check_decode(cuda_device, "wman", B, T)


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"grid{g}")
@pytest.mark.parametrize("B", [33, 167])
@pytest.mark.parametrize("T", [1, 2, 3, 20])
def test_wman_in_prologue_channel(cuda_device, T, B, grid, monkeypatch):
    _set_grid(monkeypatch, grid)
    _check_decode_awgn(cuda_device, "wman", B, T)


@pytest.mark.parametrize("T", [2, 24])
def test_80211n_one_chunk_ucn_instance(cuda_device, T):
    """The instance with idle check waves: its last wave folds.  T = 24 runs four iterations
    whose check phases select alpha' by the syndromes."""
    _check_decode(cuda_device, "wifi", 70, T)
    _check_decode_awgn(cuda_device, "wifi", 70, T)


@pytest.mark.parametrize("grid", ["1", None], ids=lambda g: f"grid{g}")
@pytest.mark.parametrize("T", [3, 20])
def test_generic_instance(cuda_device, T, grid, monkeypatch):
    _set_grid(monkeypatch, grid)
    _check_decode(cuda_device, "vdeg8", BMAX, T)


@pytest.mark.parametrize("name,T", [("wman", 20), ("wman", 3), ("wifi", 24)])
def test_early_stop_builds(cuda_device, name, T):
    """decode(early_stop=True): the ES builds run the same loop and fold, and leave it at a
    barrier that follows the fold.  Every output against the early-stop reference."""
    import torch
    B = 70
    dec = _dec(cuda_device, name)
    assert dec.supports_early_stop()
    llr, want = _expect(name, B, T)
    ref = es_reference(want["hard"], want["synd"], dec.target_bits)
    assert len(set(ref["n_iter"].tolist())) >= 2, ref["n_iter"]
    sentinel = 1234567
    cnt = torch.tensor([0, 0, 0, sentinel], dtype=torch.int64, device=cuda_device)
    r = dec.decode(torch.from_numpy(llr).to(cuda_device), T=T, counters=cnt, flags=True, early_stop=True,
                   n_iter=True, iter_hist=True)
    assert dec.last_kernel().startswith("bsl[") and ",es" in dec.last_kernel(), dec.last_kernel()
    c = r.counters.cpu().numpy()
    got = {"n_iter": r.n_iter.cpu().numpy(), "flags": r.flags.cpu().numpy(),
           "counters": np.array([c[0], c[1], c[2], 0], np.int64), "iter_hist": r.iter_hist.cpu().numpy()}
    print(name, T, "n_iter", np.bincount(ref["n_iter"]).tolist(), "counters", ref["counters"].tolist(),
          "| got", got["counters"].tolist())
    assert c[3] == sentinel
    for k in ("n_iter", "flags", "counters", "iter_hist"):
        assert np.array_equal(got[k], ref[k]), (name, T, k)
