"""The decoded-word output of the bit-sliced decoders (``decode(hard_last=True)``,
ldpc_decode_word): the last iteration's hard decisions and the per-frame "syndrome
nonzero" flag, against the CPU oracle and against the existing export path, bit for bit.

The inputs carry dense, nonzero decisions (an all-zero-codeword batch at a working SNR decodes to
zeros, and an all-zero output buffer would pass): x is a random nonzero vector of the null space of
H over GF(2) (numpy elimination, H augmented by unit rows on the shortened positions, so x is 0
there), and the LLR rows are those of ``dec.awgn(n, sigma(snr), seed=11, offset=321)`` -- pack p
taken from the batch at ``snrs[p]`` -- times 1 - 2x.  The grids are symmetric, so the rows stay on
the grid, and punctured zeros stay zero.  B = 70: two full packs and a ragged one of 6.

Each case first asserts on the oracle side what it is there for: at least 24 frames of pack 0
decode to x with a zero syndrome, at least 6 frames elsewhere end with a nonzero syndrome.  Then,
all exact: hard_last == the oracle's hard[T-1] packed == decode(hard=True).hard[T-1];
word_flags & 1 == synd[T-1].any(); counters and flags == those of a plain decode of the same rows.
One oracle run per case, shared by the tests that use it."""
import functools

import numpy as np
import pytest

from _helpers import counters_from_app, dense16, row_col_weights, vdeg8
from oracle import nms_oracle

pytestmark = pytest.mark.gpu
SEED, OFFSET = 11, 321
B = 70

# name -> (graph, T, q, weights, snrs of packs 0, 1, 2 in dB)
CASES = {
    "C2": ("C2", 20, 5, "trained", (4.0, 2.0, 1.0)),
    "C3": ("C3", 50, 5, "trained", (4.5, 2.0, 1.0)),
    "C4": ("C4", 20, 5, "trained", (3.0, 1.0, 0.0)),
    "C5": ("C5", 12, 5, "flat", (6.0, 3.0, 2.0)),
    "C2-qm5": ("C2", 20, -5, "trained", (4.0, 2.0, 1.0)),
    "C2-q4": ("C2", 20, 4, "trained", (4.0, 2.0, 1.0)),
    "C2-q3": ("C2", 20, 3, "trained", (4.0, 2.0, 1.0)),
    "C4-ucn": ("C4", 20, 5, "ucn", (3.0, 1.0, 0.0)),          # alpha' != alpha: the UCN instance
    "C4-rowcol": ("C4", 20, 5, "rowcol", (8.0, 1.0, 0.0)),    # per-row alpha, per-column beta
    "C5-rows": ("C5", 12, 5, "rows", (6.0, 3.0, 2.0)),        # bsc: per-row alpha, beta = 1
    "C5-beta": ("C5", 12, 5, "beta", (6.0, 3.0, 2.0)),        # bsc: the beta-table build
    "dense16": ("dense16", 3, 5, "flat", (9.0, 2.0, 0.0)),    # the generic one-chunk instance
    "vdeg8": ("vdeg8", 3, 5, "flat", (9.0, 1.0, -1.0)),
}
SYNTH = {"dense16": (dense16, 16), "vdeg8": (vdeg8, 21)}


def null_vector(proto, z, short, seed=5):
    """A random nonzero x with H x = 0 over GF(2) and x = 0 on the shortened positions (1-based
    inclusive range ``short``, (0, 0): none): Gaussian elimination of H augmented by unit rows."""
    g = nms_oracle.lifted_edges(proto, z)
    M, N = np.asarray(proto).shape
    nv = N * z
    rows = []
    P = np.asarray(proto)
    for i in range(M):
        for h in range(z):
            r = np.zeros(nv, np.uint8)
            for j in range(N):
                if P[i, j] >= 0:
                    r[j * z + (h + int(P[i, j])) % z] ^= 1
            rows.append(r)
    if short[0] > 0:
        for v in range(short[0] - 1, short[1]):
            r = np.zeros(nv, np.uint8)
            r[v] = 1
            rows.append(r)
    A = np.array(rows, np.uint8)
    piv, r0 = [], 0
    for c in range(nv):
        nz = np.nonzero(A[r0:, c])[0]
        if nz.size == 0:
            continue
        p = r0 + int(nz[0])
        if p != r0:
            A[[r0, p]] = A[[p, r0]]
        hit = np.nonzero(A[:, c])[0]
        hit = hit[hit != r0]
        A[hit] ^= A[r0]
        piv.append(c)
        r0 += 1
        if r0 == A.shape[0]:
            break
    free = np.setdiff1d(np.arange(nv), np.array(piv, int))
    assert free.size > 0
    rs = np.random.RandomState(seed)
    while True:
        f = rs.randint(0, 2, free.size).astype(np.uint8)
        if f.any():
            break
    x = np.zeros(nv, np.uint8)
    x[free] = f
    for k, c in enumerate(piv):                      # reduced rows: x[pivot] = sum of its free entries
        x[c] = (A[k, free] & f).sum() & 1
    assert not nms_oracle.syndromes(x[None, None, :].astype(bool), g).any()
    assert x.any() and (short[0] == 0 or not x[short[0] - 1:short[1]].any())
    return x


def pack_bits(bits):
    """[..., n] 0/1 -> [..., ceil(n/32)] uint32, bit v % 32 of word v // 32 (unpack_bits' inverse)."""
    bits = np.asarray(bits).astype(np.uint8)
    n = bits.shape[-1]
    pad = (-n) % 32
    if pad:
        bits = np.concatenate([bits, np.zeros(bits.shape[:-1] + (pad,), np.uint8)], axis=-1)
    by = np.packbits(bits, axis=-1, bitorder="little")
    return np.ascontiguousarray(by).view(np.uint32)


def _problem(gname, T, weights):
    """(proto, z, TannerGraph, DecoderWeights, CodeParams, punct, short)."""
    import bench
    from ldpc_error_floor_amd.code import CodeParams, TannerGraph
    from ldpc_error_floor_amd.weights import expand_weights, flat_weights
    if gname in SYNTH:
        fn, z = SYNTH[gname]
        proto = fn(1, z)
        g = TannerGraph(proto, z)
        return proto, z, g, flat_weights(g, T, 0.75, 1.0), CodeParams(proto, z), (0, 0), (0, 0)
    proto, g, W, cp = bench.load_problem(T=T, config=gname)
    cfg = bench.CONFIGS[gname]
    rs = np.random.RandomState(4)
    if weights == "ucn":
        W = expand_weights((2, 2, 2), {0: rs.uniform(0.5, 1.0, (T, g.M)), 1: rs.uniform(0.5, 1.0, (T, g.M)),
                                       2: rs.uniform(0.7, 1.2, (T, g.N))}, T, g)
        assert W.alpha_ucn is not None and not np.array_equal(W.alpha, W.alpha_ucn)
    elif weights == "rowcol":
        W = row_col_weights(g, T, 7)
    elif weights == "rows":
        W = expand_weights((2, 0, 3), {0: rs.uniform(0.5, 1.0, (T, g.M)), 2: np.ones((T, 1))}, T, g)
    elif weights == "beta":
        W = expand_weights((2, 0, 3), {0: rs.uniform(0.5, 1.0, (T, g.M)), 2: rs.uniform(0.7, 1.3, (T, 1))}, T, g)
    return proto, cfg["z"], g, W, cp, cfg.get("punct", (0, 0)), cfg.get("short", (0, 0))


def _rows(dec, cp, snrs, n, x):
    """Rows of ``dec.awgn(n, sigma(snr), SEED, OFFSET)`` times 1 - 2x: pack p at ``snrs[p]``."""
    import torch
    parts = []
    for p, snr in enumerate(snrs):
        a = dec.awgn(n, float(cp.sigma(snr)), seed=SEED, offset=OFFSET)
        parts.append(a[32 * p:min(n, 32 * p + 32)])
    sign = torch.from_numpy(1.0 - 2.0 * x.astype(np.float32)).to(parts[0].device)
    return (torch.cat(parts) * sign).contiguous()


def _reference(proto, z, W, T, q, llr):
    """The oracle's decode of ``llr``: packed hard[t] / syndrome flags per iteration and the APP."""
    out = nms_oracle.decode(llr, proto, z, W.alpha, W.alpha_ucn, W.beta, T, 2, q)
    return {"hard": out["hard"].astype(np.uint8), "synd_any": out["synd"].any(axis=-1), "app": out["app"]}


@functools.lru_cache(maxsize=None)
def _case(device, name, n=B, reps=1):
    """Decoder, x, the LLR rows (``reps`` times the three packs, the last one ragged) and their
    oracle reference of one case; none of which a test changes."""
    from ldpc_error_floor_amd.decoder import NMSDecoder
    gname, T, q, weights, snrs = CASES[name]
    proto, z, g, W, cp, punct, short = _problem(gname, T, weights)
    dec = NMSDecoder(proto, z, W, 2, q, device=device)
    dec.punct, dec.short = punct, short
    x = null_vector(proto, z, short)
    llr = _rows(dec, cp, snrs * reps, n, x)
    ref = _reference(proto, z, W, T, q, llr.cpu().numpy())
    return dec, x, llr, ref


def _oracle_side(x, ref, T):
    """What the case is there for: pack 0 mostly decodes to x, frames elsewhere do not decode."""
    ok = (ref["hard"][T - 1] == x[None, :]).all(axis=1) & ~ref["synd_any"][T - 1]
    assert int(ok[:32].sum()) >= 24, int(ok[:32].sum())
    assert int(ref["synd_any"][T - 1][32:].sum()) >= 6
    print("equal x per pack", [int(ok[s:s + 32].sum()) for s in range(0, ok.size, 32)], "nonzero syndrome",
          [int(ref["synd_any"][T - 1][s:s + 32].sum()) for s in range(0, ok.size, 32)], "weight", int(x.sum()))


def _word(dec, llr, T=None, **kw):
    r = dec.decode(llr, T=T, hard_last=kw.pop("hard_last", True), word_flags=True, counters=True, flags=True, **kw)
    name = dec.last_kernel()
    assert name.startswith(("bsl[", "bsc[")) and name.endswith(",word]"), name
    return {"hard_last": r.hard_last.cpu().numpy().view(np.uint32), "word_flags": r.word_flags.cpu().numpy(),
            "counters": r.counters.cpu().numpy(), "flags": r.flags.cpu().numpy()}


def _plain(dec, llr, T=None):
    r = dec.decode(llr, T=T, app=False, counters=True, flags=True)
    return r.counters.cpu().numpy(), r.flags.cpu().numpy(), dec.last_kernel()


def _check(dec, llr, ref, T, nb=None):
    """The required equalities on the first ``nb`` rows at ``T`` iterations."""
    nb = llr.shape[0] if nb is None else nb
    rows = llr[:nb].contiguous()
    got = _word(dec, rows, T=T)
    want = pack_bits(ref["hard"][T - 1, :nb])
    assert got["hard_last"].shape == want.shape and want.any()
    assert np.array_equal(got["hard_last"], want)
    old = dec.decode(rows, T=T, app=False, hard=True).hard[T - 1].cpu().numpy().view(np.uint32)
    assert np.array_equal(got["hard_last"], old)
    assert np.array_equal(got["word_flags"] & 1, ref["synd_any"][T - 1, :nb].astype(np.uint8))
    assert not (got["word_flags"] & 0xFE).any()
    cnt, flg, _ = _plain(dec, rows, T=T)
    assert np.array_equal(got["counters"], cnt) and np.array_equal(got["flags"], flg)
    assert np.array_equal(cnt, counters_from_app(ref["app"][:T, :nb, :dec.target_bits]))
    return got


@pytest.mark.parametrize("name", list(CASES))
def test_equals_oracle_and_export_path(cuda_device, name):
    dec, x, llr, ref = _case(cuda_device, name)
    T = CASES[name][1]
    assert dec.supports_hard_last()
    _oracle_side(x, ref, T)
    _check(dec, llr, ref, T)


@pytest.mark.parametrize("nb,T", [(1, 1), (33, 1), (1, 2), (33, 2)])
def test_small_batches_and_one_or_two_iterations(cuda_device, nb, T):
    """Iteration t of codeword b depends on neither B nor T: the [T - 1, :nb] corner of C2's run."""
    dec, x, llr, ref = _case(cuda_device, "C2")
    _check(dec, llr, ref, T, nb)


def test_last_word_padding_and_caller_owned_rows(cuda_device):
    """C3: 648 = 20 * 32 + 8, so the top 24 bits of a row's last word are zero; a caller-owned
    ``hard_last`` of B + 3 rows keeps what it held in the rows at index B and above."""
    import torch
    dec, x, llr, ref = _case(cuda_device, "C3")
    T = CASES["C3"][1]
    sentinel = 0x5A5A5A5A
    own = torch.full((B + 3, 21), sentinel, dtype=torch.int32, device=cuda_device)
    got = _word(dec, llr, hard_last=own)
    assert got["hard_last"].shape == (B + 3, 21)
    assert (got["hard_last"][B:] == sentinel).all()
    assert np.array_equal(got["hard_last"][:B], pack_bits(ref["hard"][T - 1]))
    assert (got["hard_last"][:B, 20] & 0xFF).any() and not (got["hard_last"][:B, 20] >> 8).any()


def test_pack_loop(cuda_device, monkeypatch):
    """C2 with B = 167 (six packs, the last of 7) through 1, 2, one-per-pack and the resident
    workgroups: the export build's pack loop stores each pack at its own row of the scratch."""
    dec, x, llr, ref = _case(cuda_device, "C2", 167, 2)
    T = CASES["C2"][1]
    assert llr.shape[0] == 167
    _oracle_side(x, ref, T)
    want = pack_bits(ref["hard"][T - 1])
    first = None
    for grid in ("1", "2", "0", None):
        if grid is None:
            monkeypatch.delenv("LDPC_BS_GRID", raising=False)
        else:
            monkeypatch.setenv("LDPC_BS_GRID", grid)
        got = _word(dec, llr)
        assert np.array_equal(got["hard_last"], want), grid
        assert np.array_equal(got["word_flags"], ref["synd_any"][T - 1].astype(np.uint8)), grid
        first = first or got
        for k in got:
            assert np.array_equal(got[k], first[k]), (grid, k)
    assert np.array_equal(first["counters"], counters_from_app(ref["app"][:, :, :dec.target_bits]))


def test_off_grid_pack_is_marked_not_decoded(cuda_device):
    dec, x, llr, ref = _case(cuda_device, "C2")
    T = CASES["C2"][1]
    clean = _word(dec, llr)
    bad = llr.clone()
    bad[40, 300] += 0.1                     # pack 1 off the grid
    with pytest.raises(ValueError, match="grid"):
        dec.decode(bad, hard_last=True)
    got = _word(dec, bad, on_off_grid="mark")
    assert (got["word_flags"][32:64] == 0x80).all() and (got["flags"][32:64] == 0x80).all()
    assert not got["hard_last"][32:64].any()
    keep = np.r_[0:32, 64:70]
    for k in ("hard_last", "word_flags", "flags"):
        assert np.array_equal(got[k][keep], clean[k][keep]), k
    assert clean["hard_last"][32:64].any()
    assert np.array_equal(got["counters"], counters_from_app(ref["app"][:T, keep][:, :, :dec.target_bits]))


def test_unsupported_requests_raise_without_a_launch(cuda_device):
    """q = 6, a float mode, the flood kernel and per-edge check weights have no bit-sliced decode."""
    import bench
    from ldpc_error_floor_amd.decoder import NMSDecoder
    from ldpc_error_floor_amd.weights import expand_weights
    proto, g, W, cp = bench.load_problem(T=4, config="C2")
    rs = np.random.RandomState(3)
    per_edge = expand_weights((1, 0, 3), {0: rs.uniform(0.5, 1.0, (4, g.E)), 2: np.ones((4, 1))}, 4, g)
    for kw, weights, kernel in ((dict(decoding_type=2, q_bit=6), W, None), (dict(decoding_type=1, q_bit=5), W, None),
                                (dict(decoding_type=2, q_bit=5), W, "flood"),
                                (dict(decoding_type=2, q_bit=5), per_edge, None)):
        dec = NMSDecoder(proto, 24, weights, device=cuda_device, **kw)
        llr = dec.awgn(33, float(cp.sigma(3.0)), seed=SEED)
        dec.decode(llr, app=False, counters=True, kernel=kernel)
        before = dec.last_kernel()
        assert before and "word" not in before
        assert not dec.supports_hard_last(kernel=kernel)
        with pytest.raises(RuntimeError, match="unsupported"):
            dec.decode(llr, hard_last=True, kernel=kernel, on_off_grid="mark")
        assert dec.last_kernel() == before
    with pytest.raises(ValueError):
        dec.decode(llr, hard_last=True, hard=True)
    with pytest.raises(ValueError):
        dec.decode_awgn(33, 0.5, SEED, hard_last=True)


def test_default_decode_unchanged_after_a_word_decode(cuda_device):
    """The same context: a plain decode after a word decode gives what a fresh decoder gives."""
    from ldpc_error_floor_amd.decoder import NMSDecoder
    dec, x, llr, ref = _case(cuda_device, "C2")
    fresh = NMSDecoder(dec.graph.proto, dec.z, dec.weights, 2, dec.q_bit, device=cuda_device)
    want = _plain(fresh, llr)
    _word(dec, llr)
    got = _plain(dec, llr)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
    assert "word" not in got[2] and got[2].startswith("bsl[")
