"""The decoded word of the early-stop decode (``decode(early_stop=True, hard_last=True)``,
ldpc_decode_es_word / ldpc_decode_awgn_es_word): each frame's hard decisions at its
own stop iteration and the "not a codeword" flag, against the test-only reference
(tests/_es_word_ref.py on the oracle's per-iteration hard decisions and syndromes), bit for bit.

Inputs as tests/test_gpu_word.py: B = 70 (two full packs and a ragged one of 6), a random nonzero
null-space vector x of H, rows of ``dec.awgn(70, sigma(snr), seed=11, offset=321)`` -- pack p taken
from the batch at ``snrs[p]`` -- times 1 - 2x.  One oracle run per case, shared by the tests that
use it.  The SNRs were chosen with the oracle on the CPU (oracle/philox_oracle.py reproduces the
channel), so that the oracle alone meets what each case is there for:
  1. every frame of pack 0 stops before T - 1, at three or more distinct iterations: the pack that
     leaves the loop early and gets its bits from the newly-done events alone;
  2. six or more frames outside pack 0 never stop and share their pack with frames that do: the
     merge of the last variable phase under the done mask;
  3. the ragged pack holds both kinds;
  4. a frame whose word at its stop iteration differs from iteration T - 1's, or whose syndrome
     reopens after the stop (C2, C2-qm5, C3, C5-rows; see the note at CASES for C5)."""
import functools

import numpy as np
import pytest

from _es_word_ref import es_word_reference
from oracle import nms_oracle
from test_gpu_word import _problem, _rows, null_vector

pytestmark = pytest.mark.gpu
SEED, OFFSET = 11, 321
B = 70
KEYS = ("hard_last", "word_flags", "counters", "flags", "n_iter", "iter_hist")

# name -> (graph, T, q, weights, snrs of packs 0, 1, 2 in dB, condition 4 met)
# C5 with flat weights: at 8, 6, 4, 3 and 2 dB no frame of this batch has a word at its stop
# iteration that differs from iteration T - 1's, and no syndrome reopens (the oracle, T = 12), so the
# case does not ask for condition 4; C5-rows, the same kernel, has both kinds.
CASES = {
    "C2": ("C2", 20, 5, "trained", (4.0, 2.0, 2.0), True),
    "C2-qm5": ("C2", 20, -5, "trained", (4.0, 3.0, 2.0), True),
    "C3": ("C3", 50, 5, "trained", (4.5, 3.0, 3.0), True),
    "C5": ("C5", 12, 5, "flat", (6.0, 3.0, 3.0), False),
    "C5-rows": ("C5", 12, 5, "rows", (6.0, 3.0, 3.0), True),
}


def _new_decoder(device, name):
    from ldpc_error_floor_amd.decoder import NMSDecoder
    gname, T, q, weights, snrs, _ = CASES[name]
    proto, z, g, W, cp, punct, short = _problem(gname, T, weights)
    dec = NMSDecoder(proto, z, W, 2, q, device=device)
    dec.punct, dec.short = punct, short
    return dec, cp


@functools.lru_cache(maxsize=None)
def _case(device, name):
    """Decoder, channel parameters, the LLR rows and their reference; none of which a test changes."""
    gname, T, q, weights, snrs, _ = CASES[name]
    dec, cp = _new_decoder(device, name)
    x = null_vector(dec.graph.proto, dec.z, dec.short)
    llr = _rows(dec, cp, snrs, B, x)
    W = dec.weights
    out = nms_oracle.decode(llr.cpu().numpy(), dec.graph.proto, dec.z, W.alpha, W.alpha_ucn, W.beta, T, 2, q)
    hard, synd = out["hard"].astype(bool), out["synd"].astype(bool)
    ref = es_word_reference(hard, synd, dec.target_bits)
    zero = ~synd.any(axis=2)
    ref["never"] = ~zero.any(axis=0)
    b = np.arange(B)
    ref["differs"] = (hard[ref["stop"], b] != hard[T - 1, b]).any(axis=1)
    ref["reopens"] = np.array([bool((~zero[ref["stop"][i] + 1:, i]).any()) and not ref["never"][i] for i in range(B)])
    return dec, cp, llr, ref


def _oracle_side(name, ref):
    T, cond4 = CASES[name][1], CASES[name][5]
    stop, never = ref["stop"], ref["never"]
    print(name, "stops of pack 0", sorted(set(stop[:32].tolist())), "never per pack",
          [int(never[s:s + 32].sum()) for s in (0, 32, 64)], "differs", int(ref["differs"].sum()),
          "reopens", int(ref["reopens"].sum()), "only zero at T-1", int(((stop == T - 1) & ~never).sum()))
    assert (stop[:32] < T - 1).all() and len(set(stop[:32].tolist())) >= 3                       # 1
    assert int(never[32:].sum()) >= 6                                                            # 2
    for lo, hi in ((32, 64), (64, 70)):                                                          # 2, 3
        assert never[lo:hi].any() and (~never[lo:hi]).any(), (lo, hi)
    if cond4:
        assert (ref["differs"] | ref["reopens"]).any()                                           # 4
    assert ref["hd_stop"].any() and ref["word_flags"].any() and not ref["word_flags"].all()


def _es_word(dec, llr, T=None, hard_last=True, **kw):
    import torch
    sentinel = 1234567
    cnt = torch.tensor([0, 0, 0, sentinel], dtype=torch.int64, device=dec.device)
    r = dec.decode(llr, T=T, early_stop=True, hard_last=hard_last, word_flags=True, counters=cnt, flags=True,
                   n_iter=True, iter_hist=True, **kw)
    name = dec.last_kernel()
    assert name.startswith(("bsl[", "bsc[")) and name.endswith(",es,word]"), name
    c = r.counters.cpu().numpy()
    assert c[3] == sentinel, "counters[3] is left untouched by the mode"
    return {"hard_last": r.hard_last.cpu().numpy().view(np.uint32), "word_flags": r.word_flags.cpu().numpy(),
            "counters": np.array([c[0], c[1], c[2], 0], np.int64), "flags": r.flags.cpu().numpy(),
            "n_iter": r.n_iter.cpu().numpy(), "iter_hist": r.iter_hist.cpu().numpy()}


def _es_only(dec, llr, **kw):
    r = dec.decode(llr, early_stop=True, counters=True, flags=True, n_iter=True, iter_hist=True, **kw)
    assert dec.last_kernel().endswith(",es]"), dec.last_kernel()
    c = r.counters.cpu().numpy()
    return {"counters": np.array([c[0], c[1], c[2], 0], np.int64), "flags": r.flags.cpu().numpy(),
            "n_iter": r.n_iter.cpu().numpy(), "iter_hist": r.iter_hist.cpu().numpy()}


@pytest.mark.parametrize("name", list(CASES))
def test_equals_reference_and_early_stop_decode(cuda_device, name):
    import torch
    dec, cp, llr, ref = _case(cuda_device, name)
    T = CASES[name][1]
    assert dec.supports_hard_last(early_stop=True) and dec.supports_early_stop()
    _oracle_side(name, ref)
    nw = (dec.n_vars + 31) // 32
    sentinel = 0x5A5A5A5A
    own = torch.full((B + 3, nw), sentinel, dtype=torch.int32, device=cuda_device)
    got = _es_word(dec, llr, hard_last=own)
    assert got["hard_last"].shape == (B + 3, nw)
    assert (got["hard_last"][B:] == sentinel).all()                  # rows past B untouched
    assert np.array_equal(got["hard_last"][:B], ref["hard_stop"])
    assert np.array_equal(got["word_flags"] & 1, ref["word_flags"])
    assert not (got["word_flags"] & 0xFE).any()
    assert not (got["word_flags"][got["n_iter"] < T] & 1).any()
    plain = _es_only(dec, llr)
    for k in ("counters", "flags", "n_iter", "iter_hist"):
        assert np.array_equal(got[k], plain[k]), k
        assert np.array_equal(got[k], ref[k]), k


def test_result_does_not_depend_on_the_pack(cuda_device):
    """C2's rows permuted: every frame keeps its word, flag and stop iteration."""
    import torch
    dec, cp, llr, ref = _case(cuda_device, "C2")
    perm = np.random.RandomState(1).permutation(B)
    got = _es_word(dec, llr[torch.from_numpy(perm).to(llr.device)].contiguous())
    assert np.array_equal(got["hard_last"], ref["hard_stop"][perm])
    assert np.array_equal(got["word_flags"], ref["word_flags"][perm])
    assert np.array_equal(got["n_iter"], ref["n_iter"][perm])


@pytest.mark.parametrize("name,snr", [("C2", 2.0), ("C5", 3.0)])
def test_in_kernel_channel_equals_decode_of_awgn(cuda_device, name, snr):
    """``decode_awgn(early_stop=True, hard_last=True)`` (the all-zero codeword's channel generated in
    the kernel) equals ``decode(awgn(same seed and offset), early_stop=True, hard_last=True)``."""
    dec, cp, _, _ = _case(cuda_device, name)
    sigma = float(cp.sigma(snr))
    a = _es_word(dec, dec.awgn(B, sigma, seed=SEED, offset=OFFSET))
    r = dec.decode_awgn(B, sigma, SEED, offset=OFFSET, early_stop=True, hard_last=True, word_flags=True,
                        counters=True, flags=True, n_iter=True, iter_hist=True)
    assert dec.last_kernel().endswith(",es,word]+gen"), dec.last_kernel()
    b = {k: getattr(r, k).cpu().numpy() for k in KEYS}
    b["hard_last"] = b["hard_last"].view(np.uint32)
    b["counters"][3] = 0
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k
    assert a["hard_last"].any() and (a["word_flags"] & 1).any() and not (a["word_flags"] & 1).all()
    with pytest.raises(ValueError, match="does not serve hard_last"):
        dec.decode_awgn(B, sigma, SEED, hard_last=True)


@pytest.mark.parametrize("name", ["C2", "C5"])
def test_off_grid_pack_is_marked_not_decoded(cuda_device, name):
    dec, cp, llr, ref = _case(cuda_device, name)
    clean = _es_word(dec, llr)
    bad = llr.clone()
    bad[40, 300] += 0.1                     # pack 1 off the grid
    with pytest.raises(ValueError, match="grid"):
        dec.decode(bad, early_stop=True, hard_last=True)
    got = _es_word(dec, bad, on_off_grid="mark")
    assert (got["word_flags"][32:64] == 0x80).all() and (got["flags"][32:64] == 0x80).all()
    assert not got["hard_last"][32:64].any() and (got["n_iter"][32:64] == 0).all()
    assert clean["hard_last"][32:64].any()
    keep = np.r_[0:32, 64:70]
    for k in ("hard_last", "word_flags", "flags", "n_iter"):
        assert np.array_equal(got[k][keep], clean[k][keep]), k
    T = CASES[name][1]
    stop = ref["stop"][keep]
    assert np.array_equal(got["iter_hist"], np.bincount(stop, minlength=T))
    want = np.array([ref["hd_stop"][keep][:, :dec.target_bits].sum(), (ref["flags"][keep] >> 1 & 1).sum(),
                     (ref["flags"][keep] & 1).sum(), 0], np.int64)
    assert np.array_equal(got["counters"], want)


def test_unsupported_request_raises_without_a_launch(cuda_device):
    """C4 (5G BG2, a multi-chunk bsl instance) has no early-stop build: LDPC_ERR_UNSUPPORTED, as
    ``early_stop`` alone, with nothing launched and nothing written."""
    import bench
    import torch
    from ldpc_error_floor_amd.decoder import NMSDecoder
    proto, g, W, cp = bench.load_problem(T=4, config="C4")
    cfg = bench.CONFIGS["C4"]
    dec = NMSDecoder(proto, cfg["z"], W, 2, 5, device=cuda_device)
    dec.punct, dec.short = cfg["punct"], cfg["short"]
    sigma = float(cp.sigma(2.0))
    llr = dec.awgn(33, sigma, seed=SEED)
    dec.decode(llr, app=False, counters=True)
    before = dec.last_kernel()
    assert before.startswith("bsl[") and dec.supports_hard_last()
    assert not dec.supports_hard_last(early_stop=True) and not dec.supports_early_stop()
    nw = (dec.n_vars + 31) // 32

    def outs():
        return dict(hard_last=torch.full((33, nw), 0x5A5A5A5A, dtype=torch.int32, device=cuda_device),
                    counters=torch.full((4,), 77, dtype=torch.int64, device=cuda_device),
                    flags=torch.full((33,), 0x55, dtype=torch.uint8, device=cuda_device),
                    iter_hist=torch.full((4,), 99, dtype=torch.int64, device=cuda_device))

    for call in (lambda o: dec.decode(llr, early_stop=True, word_flags=True, n_iter=True, on_off_grid="mark", **o),
                 lambda o: dec.decode_awgn(33, sigma, SEED, early_stop=True, word_flags=True, n_iter=True, **o)):
        o = outs()
        with pytest.raises(RuntimeError, match="unsupported"):
            call(o)
        torch.cuda.synchronize()
        assert (o["hard_last"] == 0x5A5A5A5A).all() and (o["counters"] == 77).all()
        assert (o["flags"] == 0x55).all() and (o["iter_hist"] == 99).all()
        assert dec.last_kernel() == before
    with pytest.raises(RuntimeError, match="unsupported"):
        dec.decode(llr, early_stop=True, on_off_grid="mark")


@pytest.mark.parametrize("name", ["C2", "C5"])
def test_alternating_modes_on_one_context(cuda_device, name):
    """Early stop with the word, early stop alone, the last-iteration word, a plain decode, and the
    first again, on one context: each equals its result on a fresh context (the word scratch, the
    off-grid marks and the graph tables of the two kinds of decode do not interfere)."""
    _, _, llr, ref = _case(cuda_device, name)

    def word(dec):
        r = dec.decode(llr, hard_last=True, word_flags=True, counters=True, flags=True)
        assert dec.last_kernel().endswith(",word]") and ",es" not in dec.last_kernel()
        return {"hard_last": r.hard_last.cpu().numpy(), "word_flags": r.word_flags.cpu().numpy(),
                "counters": r.counters.cpu().numpy(), "flags": r.flags.cpu().numpy()}

    def plain(dec):
        r = dec.decode(llr, app=False, counters=True, flags=True)
        assert "word" not in dec.last_kernel() and ",es" not in dec.last_kernel()
        return {"counters": r.counters.cpu().numpy(), "flags": r.flags.cpu().numpy()}

    modes = [lambda d: _es_word(d, llr), lambda d: _es_only(d, llr), word, plain, lambda d: _es_word(d, llr)]
    want = [m(_new_decoder(cuda_device, name)[0]) for m in modes[:4]]
    want.append(want[0])
    dec, _ = _new_decoder(cuda_device, name)
    for i, m in enumerate(modes):
        got = m(dec)
        for k in want[i]:
            assert np.array_equal(got[k], want[i][k]), (i, k)
    assert np.array_equal(want[0]["hard_last"], ref["hard_stop"])
    # the two word modes differ where a frame's stop-iteration word is not iteration T - 1's
    if CASES[name][5]:
        assert ref["differs"].any() == (not np.array_equal(want[0]["hard_last"], want[2]["hard_last"].view(np.uint32)))
