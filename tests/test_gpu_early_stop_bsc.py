"""Syndrome-based early termination on the compressed bit-sliced kernel (5G BG1 n2112, C5: the
early-stop builds of csrc/ldpc_bsc.hip).  Every output -- n_iter, frame flags,
counters[0..2], iter_hist -- must equal the early-stop reference (tests/_es_ref.py on the oracle's
per-iteration hard decisions and syndromes of the same LLR rows) exactly.  The batches are rows of
``dec.awgn(n, sigma, seed=7, offset=123)`` with C5's puncturing and shortening, one SNR per
32-frame pack, chosen with the oracle; each test first asserts on the oracle side what its case is
there for (a pack that leaves the T loop, frames that never stop -- the degree-1 saturation events
of DESIGN 6 --, the stops it names)."""
import functools

import numpy as np
import pytest

from _es_ref import es_oracle

pytestmark = pytest.mark.gpu
SEED, OFFSET = 7, 123
PUNCT, SHORT = (1, 144), (1537, 1584)


def _c5(device, T, q=5, weights="flat", punct=True):
    """C5's graph (z = 72) with flat alpha 0.75 / beta 1, per-row alpha with a beta block of ones
    (sharing (2, 0, 3), RandomState(4)), or a trained beta != 1 (the weights of
    test_bitsliced_compressed_trained_weights)."""
    import bench
    from ldpc_error_floor_amd.decoder import NMSDecoder
    from ldpc_error_floor_amd.weights import expand_weights
    proto, g, W, cp = bench.load_problem(T=T, config="C5")
    rng = np.random.RandomState(4)
    if weights == "rows":
        W = expand_weights((2, 0, 3), {0: rng.uniform(0.5, 1.0, (T, g.M)), 2: np.ones((T, 1))}, T, g)
    elif weights == "beta":
        W = expand_weights((2, 0, 3), {0: rng.uniform(0.5, 1.0, (T, g.M)), 2: rng.uniform(0.7, 1.3, (T, 1))}, T, g)
    dec = NMSDecoder(proto, 72, W, 2, q, device=device)
    if punct:
        dec.punct, dec.short = PUNCT, SHORT
    return dec, cp


def _rows(dec, cp, snrs, n):
    """Rows of ``dec.awgn(n, sigma(snr), SEED, OFFSET)``: pack p (rows 32 p ..) at ``snrs[p]``."""
    import torch
    parts = []
    for p, snr in enumerate(snrs):
        a = dec.awgn(n, float(cp.sigma(snr)), seed=SEED, offset=OFFSET)
        parts.append(a[32 * p:min(n, 32 * p + 32)])
    return torch.cat(parts).contiguous()


def _ref(dec, llr, T=None):
    return es_oracle(llr.cpu().numpy() if hasattr(llr, "cpu") else llr, dec.graph.proto, dec.z, dec.weights,
                     T or dec.T, dec.q_bit, dec.target_bits)


def _es(dec, llr, T=None, **kw):
    import torch
    sentinel = 1234567
    cnt = torch.tensor([0, 0, 0, sentinel], dtype=torch.int64, device=dec.device)
    r = dec.decode(llr, T=T, counters=cnt, flags=True, early_stop=True, n_iter=True, iter_hist=True, **kw)
    c = r.counters.cpu().numpy()
    assert c[3] == sentinel, "counters[3] is left untouched by the mode"
    assert dec.last_kernel().startswith("bsc[") and ",es" in dec.last_kernel(), dec.last_kernel()
    return {"n_iter": r.n_iter.cpu().numpy(), "flags": r.flags.cpu().numpy(),
            "counters": np.array([c[0], c[1], c[2], 0], np.int64), "iter_hist": r.iter_hist.cpu().numpy()}


def _assert_equal(got, ref, what=""):
    print(what, "n_iter", np.bincount(ref["n_iter"]).tolist(), "counters", ref["counters"].tolist(),
          "| got", got["counters"].tolist(), got["iter_hist"].tolist())
    for k in ("n_iter", "flags", "counters", "iter_hist"):
        assert np.array_equal(got[k], ref[k]), (what, k, got[k], ref[k])


@functools.lru_cache(maxsize=None)
def _flat12(device):
    """The flat T = 12 case, shared by the tests that use it: decoder, rows (70 frames at 10, 5 and
    3 dB) and their reference, none of which a test changes."""
    dec, cp = _c5(device, 12)
    llr = _rows(dec, cp, [10.0, 5.0, 3.0], 70)
    return dec, cp, llr, _ref(dec, llr)


def test_c5_flat(cuda_device):
    dec, cp, llr, ref = _flat12(cuda_device)
    assert dec.supports_early_stop()
    ni = ref["n_iter"].astype(int)
    # pack 0 stops entirely at 2-3 iterations (the workgroup leaves the loop); pack 1 at 4-6 with
    # frames that never stop; pack 2 is ragged (6 frames)
    assert set(ni[:32].tolist()) <= {2, 3} and len(set(ni[:32].tolist())) == 2
    assert (ni[32:64] == 12).sum() >= 1 and set(ni[32:64][ni[32:64] < 12].tolist()) <= {4, 5, 6}
    assert len(set(ni[32:64].tolist())) >= 3 and ni.size == 70
    _assert_equal(_es(dec, llr), ref, "C5 flat T=12")


def test_c5_t50(cuda_device):
    """T = 50: 50 syndrome words."""
    dec, cp = _c5(cuda_device, 50)
    llr = _rows(dec, cp, [8.0, 5.0], 33)
    ref = _ref(dec, llr)
    ni = ref["n_iter"].astype(int)
    assert {2, 3, 4, 5} <= set(ni.tolist()) and (ni == 50).sum() >= 1
    _assert_equal(_es(dec, llr), ref, "C5 flat T=50")


@pytest.mark.parametrize("T", [1, 2, 3])
def test_one_two_and_three_iterations(cuda_device, T):
    dec, cp = _c5(cuda_device, T)
    llr = _rows(dec, cp, [10.0, 3.0], 33)
    ref = _ref(dec, llr)
    ni = ref["n_iter"].astype(int)
    assert ref["iter_hist"].sum() == 33
    if T < 3:
        assert (ni == T).all()
    else:
        assert (ni == 2).sum() == 30 and (ni == 3).sum() == 3
    _assert_equal(_es(dec, llr), ref, f"T={T}")


def test_stop_at_the_first_iteration(cuda_device):
    """The t = 0 edge.  With puncturing no C5 frame stops at t = 0 (the punctured bits' APP_0 signs
    come from one check phase alone); without puncturing and shortening pack 0 does, whole."""
    dec, cp = _c5(cuda_device, 3, punct=False)
    llr = _rows(dec, cp, [10.0, 4.0], 33)
    ref = _ref(dec, llr)
    ni = ref["n_iter"].astype(int)
    assert (ni[:32] == 1).all() and ni[32] == 3
    _assert_equal(_es(dec, llr), ref, "t=0 edge")


@pytest.mark.parametrize("q", [4, -5, 3])
def test_per_row_alpha_with_beta_one(cuda_device, q):
    dec, cp = _c5(cuda_device, 8, q=q, weights="rows")
    assert dec.supports_early_stop()
    llr = _rows(dec, cp, [10.0, 5.0], 64)
    ref = _ref(dec, llr)
    ni = ref["n_iter"].astype(int)
    assert (ni[:32] < 8).all() and len(set(ni[32:].tolist())) >= 3
    _assert_equal(_es(dec, llr), ref, f"per-row alpha q={q}")


def test_result_does_not_depend_on_the_pack(cuda_device):
    import torch
    dec, cp, llr, ref = _flat12(cuda_device)
    a = _es(dec, llr)
    perm = np.random.RandomState(1).permutation(70)
    b = _es(dec, llr[torch.from_numpy(perm).to(llr.device)].contiguous())
    assert np.array_equal(b["n_iter"], a["n_iter"][perm]) and np.array_equal(b["flags"], a["flags"][perm])
    assert np.array_equal(b["counters"], a["counters"]) and np.array_equal(b["iter_hist"], a["iter_hist"])
    assert len(set(a["n_iter"].tolist())) >= 3


@pytest.mark.parametrize("offset", [0, 37])
def test_in_kernel_channel_equals_decode_of_awgn(cuda_device, offset):
    dec, cp, _, _ = _flat12(cuda_device)
    sigma = float(cp.sigma(5.0))
    a = dec.decode(dec.awgn(70, sigma, seed=SEED, offset=offset), counters=True, flags=True, early_stop=True,
                   n_iter=True, iter_hist=True)
    assert dec.last_kernel().startswith("bsc[") and dec.last_kernel().endswith(",es]"), dec.last_kernel()
    b = dec.decode_awgn(70, sigma, SEED, offset=offset, counters=True, flags=True, early_stop=True,
                        n_iter=True, iter_hist=True)
    assert dec.last_kernel().startswith("bsc[") and dec.last_kernel().endswith(",es]+gen"), dec.last_kernel()
    for k in ("counters", "flags", "n_iter", "iter_hist"):
        assert np.array_equal(getattr(a, k).cpu().numpy(), getattr(b, k).cpu().numpy()), k
    assert len(set(a.n_iter.cpu().numpy().tolist())) >= 3


def test_off_grid_pack_is_marked_not_decoded(cuda_device):
    dec, cp, llr, ref = _flat12(cuda_device)
    bad = llr.clone()
    bad[40, 300] += 0.1                     # pack 1 off the grid
    with pytest.raises(ValueError, match="grid"):
        dec.decode(bad, counters=True, early_stop=True)
    got = _es(dec, bad, on_off_grid="mark")
    assert (got["n_iter"][32:64] == 0).all() and (got["flags"][32:64] == 0x80).all()
    keep = np.r_[0:32, 64:70]
    assert np.array_equal(got["n_iter"][keep], ref["n_iter"][keep])
    assert np.array_equal(got["flags"][keep], ref["flags"][keep])
    sub = _ref(dec, llr.cpu().numpy()[keep])
    assert np.array_equal(got["counters"], sub["counters"]) and np.array_equal(got["iter_hist"], sub["iter_hist"])


def test_unsupported_requests_raise_without_a_launch(cuda_device):
    """A trained beta != 1 on BG1 (the full-T decode takes the beta-table build of bsc) and the
    flood kernel have no early-stop build."""
    dec, cp = _c5(cuda_device, 10, weights="beta")
    llr = dec.awgn(32, float(cp.sigma(5.0)), seed=SEED)
    dec.decode(llr, app=False, counters=True)
    before = dec.last_kernel()
    assert before.startswith("bsc[")
    assert not dec.supports_early_stop()
    with pytest.raises(RuntimeError, match="unsupported"):
        dec.decode(llr, early_stop=True, on_off_grid="mark")
    assert dec.last_kernel() == before
    flat, _, rows, _ = _flat12(cuda_device)
    flat.decode(rows, app=False, counters=True)
    before = flat.last_kernel()
    assert not flat.supports_early_stop(kernel="flood")
    with pytest.raises(RuntimeError, match="unsupported"):
        flat.decode(rows, early_stop=True, kernel="flood", on_off_grid="mark")
    assert flat.last_kernel() == before


def test_forced_instances(cuda_device, monkeypatch):
    """LDPC_BSC_INST: the other mixed-lane instance (three check chunks per wave, the one taken
    where the two-chunk one does not fit) has the build too and gives the same outputs; a forced
    instance without the build (uniform lanes) is unsupported, not replaced by another."""
    _, cp, llr, ref = _flat12(cuda_device)
    dec, _ = _c5(cuda_device, 12)
    _es(dec, llr)
    assert dec.last_kernel().endswith(",x3/2,es]"), dec.last_kernel()
    monkeypatch.setenv("LDPC_BSC_INST", "3")
    assert dec.supports_early_stop()
    got = _es(dec, llr)
    assert dec.last_kernel().endswith(",x3/3,es]"), dec.last_kernel()
    _assert_equal(got, ref, "forced instance 3")
    sigma = float(cp.sigma(5.0))
    a = dec.decode(dec.awgn(70, sigma, seed=SEED, offset=37), counters=True, flags=True, early_stop=True,
                   n_iter=True, iter_hist=True)
    b = dec.decode_awgn(70, sigma, SEED, offset=37, counters=True, flags=True, early_stop=True,
                        n_iter=True, iter_hist=True)
    assert dec.last_kernel().endswith(",x3/3,es]+gen"), dec.last_kernel()
    for k in ("counters", "flags", "n_iter", "iter_hist"):
        assert np.array_equal(getattr(a, k).cpu().numpy(), getattr(b, k).cpu().numpy()), k
    before = dec.last_kernel()
    monkeypatch.setenv("LDPC_BSC_INST", "0")
    assert not dec.supports_early_stop()
    with pytest.raises(RuntimeError, match="unsupported"):
        dec.decode(llr, early_stop=True, on_off_grid="mark")
    assert dec.last_kernel() == before
    monkeypatch.delenv("LDPC_BSC_INST")
    _assert_equal(_es(dec, llr), ref, "back to the planner's instance")


def test_default_decode_unchanged_after_an_early_stop_decode(cuda_device):
    """The same context: a full-T decode after an early-stop one gives what a fresh decoder gives
    (both kinds share the graph tables; the early-stop plan is never taken otherwise)."""
    def plain(dec, llr):
        r = dec.decode(llr, app=False, counters=True, flags=True)
        return r.counters.cpu().numpy(), r.flags.cpu().numpy(), dec.last_kernel()
    _, cp, llr, _ = _flat12(cuda_device)
    alone, _ = _c5(cuda_device, 12)
    want = plain(alone, llr)
    dec, _ = _c5(cuda_device, 12)
    _es(dec, llr)
    got = plain(dec, llr)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
    assert ",es" not in got[2] and got[2].startswith("bsc[")
    _es(dec, llr)
    assert plain(dec, llr)[2] == want[2]


def test_sweep(cuda_device):
    """fer_sweep(early_stop=True) on C5: batches of 1024 (the last one ragged) against one
    decode_awgn(early_stop=True) over the same global codeword range of each point's stream."""
    import torch
    from ldpc_error_floor_amd.fer import fer_sweep
    dec, cp, _, _ = _flat12(cuda_device)
    n, seed = 3000, 1076
    sig = [float(cp.sigma(s)) for s in (8.0, 5.0)]
    res = fer_sweep(dec, sig, n, 1024, seed=seed, early_stop=True)
    hist = np.stack([c.iter_hist for c in res])
    assert hist.shape == (2, 12) and (hist.sum(axis=1) == n).all(), hist
    for si, s in enumerate(sig):
        cnt = torch.zeros(4, dtype=torch.int64, device=dec.device)
        r = dec.decode_awgn(n, s, seed + 7919 * si, offset=0, counters=cnt, early_stop=True, iter_hist=True)
        assert dec.last_kernel().endswith(",es]+gen"), dec.last_kernel()
        c = r.counters.cpu().numpy()
        assert (int(res[si].bit_err_last), int(res[si].frame_err_last), int(res[si].frame_err_all)) == \
            (int(c[0]), int(c[1]), int(c[2])), (si, c)
        assert np.array_equal(hist[si], r.iter_hist.cpu().numpy()), si
    assert (hist[:, :11].sum(axis=1) > 0).all()      # frames did stop early at both points
