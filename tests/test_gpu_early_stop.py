"""Syndrome-based early termination on the GPU (``decode(early_stop=True)``; the ES
builds of the bit-sliced kernel).  Every output -- n_iter, frame flags, counters[0..2], iter_hist --
must equal the early-stop reference (tests/_es_ref.py on the oracle's per-iteration hard decisions
and syndromes of the same LLR rows) exactly.  The batches are rows of ``dec.awgn`` (on the
quantizer grid), one SNR per 32-frame pack, chosen so that a pack leaves the T loop early, a frame
never stops and the stops differ; each test first asserts that on the oracle side."""
import os

import numpy as np
import pytest

from _es_ref import es_oracle
from conftest import ROOT

pytestmark = pytest.mark.gpu
DATA = os.path.join(ROOT, "ldpc_error_floor_amd", "data")
SEED, OFFSET, B = 7, 123, 70


def _graph(name, z):
    from ldpc_error_floor_amd.code import CodeParams, TannerGraph, load_base_graph
    proto = load_base_graph(os.path.join(DATA, "BaseGraph", name + ".txt"))
    return proto, TannerGraph(proto, z), CodeParams(proto, z)


def _wman(device, sharing=(3, 0, 3), q=5, T=20, seed=3, **kw):
    from ldpc_error_floor_amd.decoder import NMSDecoder
    from ldpc_error_floor_amd.weights import expand_weights, read_weight_file
    proto, g, cp = _graph("wman_N0576_R34_z24", 24)
    if sharing == (3, 0, 3):
        wf = read_weight_file(os.path.join(DATA, "Weights", "C0_wman_N0576_R34_z24_Opt_Weight_End20.txt"))
        W = expand_weights(sharing, {0: wf.blocks[0], 2: wf.blocks[2]}, T, g)
    else:
        rng = np.random.RandomState(seed)
        W = expand_weights(sharing, {0: rng.uniform(0.5, 1.2, (T, g.M)), 2: rng.uniform(0.6, 1.3, (T, g.N))}, T, g)
    return NMSDecoder(proto, 24, W, 2, q, device=device, **kw), cp


def _wifi(device, ucn, T=12):
    """802.11n: flat alpha 0.75, beta 1, or random per-iteration alpha / alpha' / beta (alpha' != alpha
    at every iteration: the check phases select between two tables by the same syndromes that stop
    the frames)."""
    from ldpc_error_floor_amd.decoder import NMSDecoder
    from ldpc_error_floor_amd.weights import expand_weights, flat_weights
    proto, g, cp = _graph("802_11n_N648_R56_z27", 27)
    if not ucn:
        W = flat_weights(g, T, alpha=0.75, beta=1.0)
    else:
        rng = np.random.RandomState(17)
        W = expand_weights((3, 3, 3), {0: rng.uniform(0.6, 0.9, (T, 1)), 1: rng.uniform(0.3, 0.55, (T, 1)),
                                       2: rng.uniform(0.85, 1.1, (T, 1))}, T, g)
        assert W.alpha_ucn is not None and (W.alpha_ucn != W.alpha).all()
    return NMSDecoder(proto, 27, W, 2, 5, device=device), cp


def _rows(dec, cp, snrs, n=B):
    """Rows of ``dec.awgn(n, sigma(snr), SEED, OFFSET)``: pack p (rows 32 p ..) at ``snrs[p]``."""
    import torch
    parts = []
    for p, snr in enumerate(snrs):
        a = dec.awgn(n, float(cp.sigma(snr)), seed=SEED, offset=OFFSET)
        parts.append(a[32 * p:min(n, 32 * p + 32)])
    return torch.cat(parts).contiguous()


def _ref(dec, llr, T=None):
    return es_oracle(llr.cpu().numpy(), dec.graph.proto, dec.z, dec.weights, T or dec.T, dec.q_bit,
                     dec.target_bits)


def _es(dec, llr, T=None, **kw):
    import torch
    sentinel = 1234567
    cnt = torch.tensor([0, 0, 0, sentinel], dtype=torch.int64, device=dec.device)
    r = dec.decode(llr, T=T, counters=cnt, flags=True, early_stop=True, n_iter=True, iter_hist=True, **kw)
    c = r.counters.cpu().numpy()
    assert c[3] == sentinel, "counters[3] is left untouched by the mode"
    assert ",es" in dec.last_kernel() and dec.last_kernel().startswith("bsl["), dec.last_kernel()
    return {"n_iter": r.n_iter.cpu().numpy(), "flags": r.flags.cpu().numpy(),
            "counters": np.array([c[0], c[1], c[2], 0], np.int64), "iter_hist": r.iter_hist.cpu().numpy()}


def _assert_equal(got, ref, what=""):
    print(what, "n_iter", np.bincount(ref["n_iter"]).tolist(), "counters", ref["counters"].tolist(),
          "| got", got["counters"].tolist(), got["iter_hist"].tolist())
    for k in ("n_iter", "flags", "counters", "iter_hist"):
        assert np.array_equal(got[k], ref[k]), (what, k, got[k], ref[k])


def _assert_not_vacuous(ref, T, n=B):
    """On the oracle side: a pack whose frames all stop before T (the workgroup leaves the loop), a
    frame that never stops, and at least three distinct iteration counts."""
    ni = ref["n_iter"].astype(int)
    packs = [ni[p:p + 32] for p in range(0, n, 32)]
    assert any((p < T).all() for p in packs), [p.max() for p in packs]
    assert (ni == T).any()
    assert len(set(ni.tolist())) >= 3, set(ni.tolist())


def test_wman_trained(cuda_device):
    dec, cp = _wman(cuda_device)
    assert dec.supports_early_stop()
    llr = _rows(dec, cp, [4.0, 3.0, 4.0])
    ref = _ref(dec, llr)
    _assert_not_vacuous(ref, 20)
    _assert_equal(_es(dec, llr), ref, "wman")


# 802.11n, T = 12, one SNR per pack.  Flat 0.75: 5.0 dB holds frames with n_iter = 1 (the t = 0
# edge) and 4.0 dB a frame that never stops.  Random UCN weights (seed 17): chosen with the oracle on
# the same rows -- 5.5 dB: every frame of the pack stops within 1-4 iterations; 4.0 and 3.0 dB: packs
# with frames that never stop (3 and 4 of them) among stops from 2 to 11.
@pytest.mark.parametrize("ucn,snrs", [(False, [5.0, 4.0, 3.0]), (True, [5.5, 4.0, 3.0])], ids=["flat", "ucn"])
def test_80211n(cuda_device, ucn, snrs):
    dec, cp = _wifi(cuda_device, ucn)
    assert dec.supports_early_stop()
    llr = _rows(dec, cp, snrs)
    ref = _ref(dec, llr)
    _assert_not_vacuous(ref, 12)
    if not ucn:
        assert (ref["n_iter"] == 1).any()
    got = _es(dec, llr)
    assert (",ucn" in dec.last_kernel()) == ucn
    _assert_equal(got, ref, "802.11n " + ("ucn" if ucn else "flat"))


@pytest.mark.parametrize("T", [1, 2])
def test_one_and_two_iterations(cuda_device, T):
    dec, cp = _wman(cuda_device)
    llr = _rows(dec, cp, [6.0, 3.0], n=33)
    ref = _ref(dec, llr, T)
    assert ref["n_iter"].max() == T and ref["iter_hist"].sum() == 33
    if T == 2:
        assert (ref["n_iter"] == 1).any() and (ref["n_iter"] == 2).any()
    _assert_equal(_es(dec, llr, T), ref, f"T={T}")


@pytest.mark.parametrize("q", [-5, 4, 3])
def test_other_grids_with_per_row_weights(cuda_device, q):
    dec, cp = _wman(cuda_device, sharing=(2, 0, 2), q=q, T=6)
    assert dec.supports_early_stop()
    llr = _rows(dec, cp, [5.0, 3.5], n=64)
    ref = _ref(dec, llr)
    assert len(set(ref["n_iter"].tolist())) >= 2
    _assert_equal(_es(dec, llr), ref, f"q={q}")


def test_result_does_not_depend_on_the_pack(cuda_device):
    import torch
    dec, cp = _wman(cuda_device)
    llr = _rows(dec, cp, [4.0, 3.0, 4.0])
    a = _es(dec, llr)
    perm = np.random.RandomState(1).permutation(B)
    b = _es(dec, llr[torch.from_numpy(perm).to(llr.device)].contiguous())
    assert np.array_equal(b["n_iter"], a["n_iter"][perm]) and np.array_equal(b["flags"], a["flags"][perm])
    assert np.array_equal(b["counters"], a["counters"]) and np.array_equal(b["iter_hist"], a["iter_hist"])
    assert len(set(a["n_iter"].tolist())) >= 3


@pytest.mark.parametrize("offset", [0, 37])
def test_in_kernel_channel_equals_decode_of_awgn(cuda_device, offset):
    dec, cp = _wman(cuda_device)
    sigma = float(cp.sigma(3.5))
    a = dec.decode(dec.awgn(B, sigma, seed=SEED, offset=offset), counters=True, flags=True, early_stop=True,
                   n_iter=True, iter_hist=True)
    assert "+gen" not in dec.last_kernel()
    b = dec.decode_awgn(B, sigma, SEED, offset=offset, counters=True, flags=True, early_stop=True,
                        n_iter=True, iter_hist=True)
    assert dec.last_kernel().endswith(",es]+gen"), dec.last_kernel()
    for k in ("counters", "flags", "n_iter", "iter_hist"):
        assert np.array_equal(getattr(a, k).cpu().numpy(), getattr(b, k).cpu().numpy()), k
    assert len(set(a.n_iter.cpu().numpy().tolist())) >= 3


def test_off_grid_pack_is_marked_not_decoded(cuda_device):
    dec, cp = _wman(cuda_device)
    llr = _rows(dec, cp, [4.0, 3.0, 4.0])
    ref = _ref(dec, llr)
    bad = llr.clone()
    bad[40, 3] += 0.1                       # pack 1 off the grid
    with pytest.raises(ValueError, match="grid"):
        dec.decode(bad, counters=True, early_stop=True)
    got = _es(dec, bad, on_off_grid="mark")
    assert (got["n_iter"][32:64] == 0).all() and (got["flags"][32:64] == 0x80).all()
    keep = np.r_[0:32, 64:B]
    assert np.array_equal(got["n_iter"][keep], ref["n_iter"][keep])
    assert np.array_equal(got["flags"][keep], ref["flags"][keep])
    sub = es_oracle(llr.cpu().numpy()[keep], dec.graph.proto, 24, dec.weights, 20, 5, dec.target_bits)
    assert np.array_equal(got["counters"], sub["counters"]) and np.array_equal(got["iter_hist"], sub["iter_hist"])


def test_unsupported_requests_raise_without_a_launch(cuda_device):
    from ldpc_error_floor_amd.decoder import NMSDecoder
    from ldpc_error_floor_amd.weights import flat_weights
    dec, cp = _wman(cuda_device)
    llr = _rows(dec, cp, [4.0], n=32)
    dec.decode(llr, app=False, counters=True)
    before = dec.last_kernel()
    with pytest.raises(ValueError):
        dec.decode(llr, app=True, early_stop=True)
    with pytest.raises(RuntimeError, match="unsupported"):
        dec.decode(llr, early_stop=True, kernel="flood", on_off_grid="mark")
    assert not dec.supports_early_stop(kernel="flood")
    assert dec.last_kernel() == before          # nothing was served
    # q = 6 (a float-mode kernel) and 5G BG2 (a multi-chunk instance): no early-stop build
    d6, _ = _wman(cuda_device, q=6)
    assert not d6.supports_early_stop()
    with pytest.raises(RuntimeError, match="unsupported"):
        d6.decode(d6.awgn(32, float(cp.sigma(4.0)), seed=SEED), early_stop=True, on_off_grid="mark")
    assert d6.last_kernel() == ""
    proto, g, cp5 = _graph("5G_LDPC_R0.50_n_dec1280_n1024_k512_z64_s513_640", 64)
    d5 = NMSDecoder(proto, 64, flat_weights(g, 4, alpha=0.75), 2, 5, device=cuda_device)
    assert not d5.supports_early_stop()
    with pytest.raises(RuntimeError, match="unsupported"):
        d5.decode(d5.awgn(32, float(cp5.sigma(4.0)), seed=SEED), early_stop=True, on_off_grid="mark")
    assert d5.last_kernel() == ""


def test_default_decode_unchanged_after_an_early_stop_decode(cuda_device):
    """The same process, the same context: a default decode after an early-stop one gives what it
    gives alone (the ES instances have graph tables of their own and are never planned otherwise)."""
    def plain(dec, llr):
        r = dec.decode(llr, app=False, counters=True, flags=True)
        return r.counters.cpu().numpy(), r.flags.cpu().numpy(), dec.last_kernel()
    alone, cp = _wman(cuda_device)
    llr = _rows(alone, cp, [4.0, 3.0, 4.0])
    want = plain(alone, llr)
    dec, _ = _wman(cuda_device)
    _es(dec, llr)
    got = plain(dec, llr)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
    assert ",es" not in got[2] and got[2].startswith("bsl[")
    _es(dec, llr)
    assert plain(dec, llr)[2] == want[2]
