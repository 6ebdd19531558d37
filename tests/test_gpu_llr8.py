"""int8 quantized LLRs through the bit-sliced kernels on the GPU (``NMSDecoder.decode_q8``,
ldpc_decode_q8 / ldpc_decode_q8_word).  The defining property: for every valid q8
every output -- counters, frame flags, the per-iteration frame-error words, the decoded word and
its flags -- equals, bit for bit, that of the float decode of the LLRs the bytes stand for.  The
references are the committed fixtures and the float path's outputs, never the int8 builds.

The batches of the tests without a fixture are B = 70 rows (two full packs and a ragged one of 6)
of ``dec.awgn(70, sigma(snr), seed=7, offset=123)``, pack p at ``SNRS[p]`` = 1 / 4 / 7 dB: far
enough apart that frames fail in the first pack and decode in the last on every graph here, which
each test asserts on the float side first (0 < frames wrong at T - 1 < B)."""
import ctypes
import os

import numpy as np
import pytest

from _helpers import counters_from_app, dense16, flags_from_app, row_col_weights, vdeg8
from conftest import ROOT, load_case
from test_gpu_periter import BITSLICED

pytestmark = pytest.mark.gpu
DATA = os.path.join(ROOT, "ldpc_error_floor_amd", "data")
SEED, OFFSET, B = 7, 123, 70
SNRS = (1.0, 4.0, 7.0)
_cache = {}


def pack_bits(bits):
    """[..., n] 0/1 -> [..., ceil(n/32)] uint32, bit v % 32 of word v // 32 (unpack_bits' inverse)."""
    bits = np.asarray(bits).astype(np.uint8)
    pad = (-bits.shape[-1]) % 32
    if pad:
        bits = np.concatenate([bits, np.zeros(bits.shape[:-1] + (pad,), np.uint8)], axis=-1)
    return np.ascontiguousarray(np.packbits(bits, axis=-1, bitorder="little")).view(np.uint32)


def _fixture_decoder(c, device):
    from ldpc_error_floor_amd.decoder import NMSDecoder
    Nt = c["Nt"] if c["Nt"] < c["g"].N else 0
    return NMSDecoder(c["g"].proto, c["z"], c["W"], c["dt"], c["q"], target_node=Nt, device=device)


def _wman_graph():
    from ldpc_error_floor_amd.code import CodeParams, TannerGraph, load_base_graph
    proto = load_base_graph(os.path.join(DATA, "BaseGraph", "wman_N0576_R34_z24.txt"))
    return proto, TannerGraph(proto, 24), CodeParams(proto, 24)


def _wman(device):
    """wman N576 z24 with the trained C2 weights, QMS q = 5 (one decoder for the module)."""
    if "wman" not in _cache:
        from ldpc_error_floor_amd.decoder import NMSDecoder
        from ldpc_error_floor_amd.weights import expand_weights, read_weight_file
        proto, g, cp = _wman_graph()
        wf = read_weight_file(os.path.join(DATA, "Weights", "C0_wman_N0576_R34_z24_Opt_Weight_End20.txt"))
        W = expand_weights((3, 0, 3), {0: wf.blocks[0], 2: wf.blocks[2]}, 20, g)
        _cache["wman"] = (NMSDecoder(proto, 24, W, 2, 5, device=device), cp)
    return _cache["wman"]


def _rows(dec, cp, snrs=SNRS, n=B, seed=SEED, offset=OFFSET):
    """Rows of ``dec.awgn(n, sigma(snr), seed, offset)``: pack p (rows 32 p ..) at ``snrs[p % 3]``."""
    import torch
    parts = []
    for p in range((n + 31) // 32):
        a = dec.awgn(n, float(cp.sigma(snrs[p % len(snrs)])), seed=seed, offset=offset)
        parts.append(a[32 * p:min(n, 32 * p + 32)])
    return torch.cat(parts).contiguous()


def _float_outputs(dec, llr, T=None):
    """The float path's outputs of ``llr``: the counters-only decode and the word mode."""
    r = dec.decode(llr, T=T, app=False, counters=True, flags=True, iter_wrong=True)
    name = dec.last_kernel()
    w = dec.decode(llr, T=T, hard_last=True, word_flags=True, counters=True, flags=True)
    out = dict(counters=r.counters, flags=r.flags, iter_wrong=r.iter_wrong, hard_last=w.hard_last,
               word_flags=w.word_flags, word_counters=w.counters, word_flagsf=w.flags)
    return {k: v.cpu().numpy() for k, v in out.items()}, name


def _q8_outputs(dec, q8, T=None, on_invalid="raise"):
    """``decode_q8``'s outputs of ``q8`` (same keys), and the two kernel names."""
    r = dec.decode_q8(q8, T=T, counters=True, flags=True, iter_wrong=True, on_invalid=on_invalid)
    n1 = dec.last_kernel()
    w = dec.decode_q8(q8, T=T, hard_last=True, word_flags=True, counters=True, flags=True, on_invalid=on_invalid)
    n2 = dec.last_kernel()
    out = dict(counters=r.counters, flags=r.flags, iter_wrong=r.iter_wrong, hard_last=w.hard_last,
               word_flags=w.word_flags, word_counters=w.counters, word_flagsf=w.flags)
    return {k: v.cpu().numpy() for k, v in out.items()}, n1, n2


def _assert_q8_equals_float(dec, llr, prefix, T=None, q8=None, vacuity=True):
    """q8 decode of quantize_q8(llr) == float decode of llr, every output; returns the float side."""
    want, fname = _float_outputs(dec, llr, T)
    nrows = int(llr.shape[0])
    if vacuity:
        assert 0 < int(want["counters"][1]) < nrows, want["counters"]
    assert fname.startswith(prefix), fname
    q8 = dec.quantize_q8(llr) if q8 is None else q8
    got, n1, n2 = _q8_outputs(dec, q8, T)
    assert n1 == fname + "+q8", (n1, fname)
    assert n2 == fname[:-1] + ",word]+q8", (n2, fname)
    for k in want:
        assert np.array_equal(got[k], want[k]), (k, fname)
    return want


# ---- 1. the reference fixtures ---------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(BITSLICED))
def test_reference_fixtures(name, cuda_device):
    """wman, 802.11n with UCN weights, 5G BG2 with puncturing and shortening (the -128 marker on a
    multi-chunk instance with the shortened-bit path) and 5G BG1 on bsc, against the fixtures."""
    c = load_case(name)
    assert c["exact"]
    T, nb = c["T"], c["llr"].shape[0]
    wrong = (c["app"] >= 0).any(axis=2)
    if not (wrong[T - 1].any() and not wrong[T - 1].all()):
        # (no frame wrong, or none right, at T - 1 in this fixture: its comparison still holds, the
        # non-vacuity of the set rests on the other names)
        print(f"{name}: {int(wrong[T - 1].sum())} of {nb} frames wrong at T - 1")
    dec = _fixture_decoder(c, cuda_device)
    q8 = dec.quantize_q8(c["llr"])
    short = np.asarray(c["llr"]) == -dec.clip
    assert np.array_equal(q8.numpy() == -128, short)
    r = dec.decode_q8(q8, counters=True, flags=True, iter_wrong=True)
    assert dec.last_kernel().startswith(BITSLICED[name]) and dec.last_kernel().endswith("+q8"), dec.last_kernel()
    assert np.array_equal(r.counters.cpu().numpy(), counters_from_app(c["app"]))
    assert np.array_equal(r.flags.cpu().numpy(), flags_from_app(c["app"]))
    assert np.array_equal(r.frame_errors(nb), wrong)
    w = dec.decode_q8(q8, hard_last=True, word_flags=True, counters=True, flags=True)
    assert dec.last_kernel().startswith(BITSLICED[name]) and dec.last_kernel().endswith(",word]+q8"), dec.last_kernel()
    assert np.array_equal(w.hard_last.cpu().numpy().view(np.uint32), pack_bits(c["hard"][T - 1]))
    assert np.array_equal(w.word_flags.cpu().numpy(), c["synd"][T - 1].any(axis=-1).astype(np.uint8))
    assert np.array_equal(w.counters.cpu().numpy(), counters_from_app(c["app"]))
    assert np.array_equal(w.flags.cpu().numpy(), flags_from_app(c["app"]))


def test_fixture_set_is_not_vacuous():
    """Some fixture of every kernel prefix has a frame wrong and a frame right at T - 1."""
    mixed = set()
    for name, prefix in BITSLICED.items():
        c = load_case(name)
        wrong = (c["app"] >= 0).any(axis=2)[c["T"] - 1]
        if wrong.any() and not wrong.all():
            mixed.add(prefix)
    assert mixed == set(BITSLICED.values()), mixed


# ---- 2. the instances the fixtures miss ------------------------------------------------------
def test_wman_ucn_instance(cuda_device):
    """kBsInst entry 9: wman with [3,3,3] weights whose alpha' differs from alpha."""
    from ldpc_error_floor_amd.decoder import NMSDecoder
    from test_gpu_bs_wman_ucn import NAME, _cascade
    proto, g, cp = _wman_graph()
    dec = NMSDecoder(proto, 24, _cascade(g), 2, 5, device=cuda_device)
    _assert_q8_equals_float(dec, _rows(dec, cp), NAME)


@pytest.mark.parametrize("gname", ["dense16", "vdeg8"])
def test_generic_instance(gname, cuda_device):
    from ldpc_error_floor_amd.code import CodeParams, TannerGraph
    from ldpc_error_floor_amd.decoder import NMSDecoder
    fn, z = {"dense16": (dense16, 16), "vdeg8": (vdeg8, 21)}[gname]
    proto = fn(1, z)
    g = TannerGraph(proto, z)
    dec = NMSDecoder(proto, z, row_col_weights(g, 20, 7), 2, 5, device=cuda_device)
    assert "d16,v8,l4" in dec.kernel_info()[1], dec.kernel_info()
    _assert_q8_equals_float(dec, _rows(dec, CodeParams(proto, z)), "bsl[p32,")


@pytest.mark.parametrize("q", [-5, 4, 3])
def test_wman_per_row_weights_on_the_other_grids(q, cuda_device):
    from ldpc_error_floor_amd.decoder import NMSDecoder
    proto, g, cp = _wman_graph()
    dec = NMSDecoder(proto, 24, row_col_weights(g, 6, 11), 2, q, device=cuda_device)
    _assert_q8_equals_float(dec, _rows(dec, cp), "bsl[p32,w9,d15,v6,l4]")


# ---- 3. odd row stride -------------------------------------------------------------------------
def test_odd_row_stride_and_unaligned_start(cuda_device):
    """A fully dense 4 x 15 proto with z = 9: n_vars = 135, no multiple of 4, so the rows start at
    every alignment; B = 33 (a full pack and a pack of one); the q8 tensor is a view that starts
    one byte into its storage.  ldpc_debug_bs_bounds has plans for the graph (checked first, on
    the host)."""
    import torch
    from ldpc_error_floor_amd.code import CodeParams, TannerGraph
    from ldpc_error_floor_amd.decoder import NMSDecoder
    from test_bs_bounds import LIB, bounds
    proto = np.random.RandomState(3).randint(0, 9, size=(4, 15)).astype(np.int64)
    L = ctypes.CDLL(LIB)
    L.ldpc_debug_bs_bounds.argtypes = [ctypes.POINTER(ctypes.c_int32), ctypes.c_int32, ctypes.c_int32,
                                       ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                       ctypes.c_int32, ctypes.c_float, ctypes.c_int32,
                                       ctypes.POINTER(ctypes.c_int32), ctypes.c_char_p, ctypes.c_int32]
    n, v, msg = bounds(L, proto, 9, 8)
    assert n >= 1 and v == 0, (n, v, msg)
    g = TannerGraph(proto, 9)
    dec = NMSDecoder(proto, 9, row_col_weights(g, 8, 5), 2, 5, device=cuda_device)
    assert dec.n_vars == 135
    llr = _rows(dec, CodeParams(proto, 9), snrs=(3.0, 3.0), n=33)
    q = dec.quantize_q8(llr)
    store = torch.empty(33 * 135 + 1, dtype=torch.int8, device=cuda_device)
    view = store[1:].view(33, 135)
    view.copy_(q)
    assert view.data_ptr() % 2 == 1 and view.is_contiguous()
    _assert_q8_equals_float(dec, llr, "bsl[p32,", q8=view, vacuity=False)
    got = dec.decode_q8(view, counters=True).counters.cpu().numpy()
    assert np.array_equal(got, dec.decode(llr, app=False, counters=True).counters.cpu().numpy())


# ---- 4. the pack loop --------------------------------------------------------------------------
def test_pack_loop_grids_and_tickets(cuda_device, monkeypatch):
    """wman, B = 167 (six packs, the last of 7) through one, two, one-per-pack and the resident
    workgroups, packs handed out by ticket and by fixed stride: identical, and the float decode's."""
    dec, cp = _wman(cuda_device)
    llr = _rows(dec, cp, n=167)
    q8 = dec.quantize_q8(llr)
    monkeypatch.delenv("LDPC_BS_GRID", raising=False)
    monkeypatch.delenv("LDPC_BS_TICKETS", raising=False)
    want, fname = _float_outputs(dec, llr)
    assert 0 < int(want["counters"][1]) < 167 and fname == "bsl[p32,w9,d15,v6,l4]"
    for tickets in (None, "0"):
        if tickets is None:
            monkeypatch.delenv("LDPC_BS_TICKETS", raising=False)
        else:
            monkeypatch.setenv("LDPC_BS_TICKETS", tickets)
        for grid in ("1", "2", "0", None):
            if grid is None:
                monkeypatch.delenv("LDPC_BS_GRID", raising=False)
            else:
                monkeypatch.setenv("LDPC_BS_GRID", grid)
            got, n1, n2 = _q8_outputs(dec, q8)
            assert n1 == fname + "+q8" and n2 == "bsl[p32,w9,d15,v6,l4,word]+q8"
            for k in want:
                assert np.array_equal(got[k], want[k]), (k, grid, tickets)


# ---- 5. invalid input --------------------------------------------------------------------------
def _marked_expectation(want, nb, T):
    """The float outputs with frames 32..63 taken out: marked 0x80, zero rows, not counted."""
    exp = {k: v.copy() for k, v in want.items()}
    for k in ("flags", "word_flags", "word_flagsf"):
        exp[k][32:64] = 0x80
    exp["hard_last"][32:64] = 0
    exp["iter_wrong"][:, 1] = 0
    return exp


def _counters_of_kept(dec, llr, keep):
    return dec.decode(llr[keep], app=False, counters=True).counters.cpu().numpy()


@pytest.mark.parametrize("case", ["qmax+1", "marker"])
def test_invalid_byte_marks_its_pack(case, cuda_device):
    """A byte past the grid, or a +-clip marker on wman (an instance without the shortened-bit
    path), in pack 1 of 3: "raise" raises naming frame 32; "mark" returns frames 32..63 with 0x80
    and zero rows, the other frames as the float decode has them, and the counters of the kept
    frames alone."""
    import torch
    dec, cp = _wman(cuda_device)
    assert not dec.supports_q8(has_short=True) and dec.supports_q8() and dec.supports_q8(word=True)
    llr = _rows(dec, cp)
    want, _ = _float_outputs(dec, llr)
    assert 0 < int(want["counters"][1]) < B
    q8 = dec.quantize_q8(llr).clone()
    q8[40, 17] = {"qmax+1": 16, "marker": -128}[case]
    with pytest.raises(ValueError, match="frame 32 is the first of 32 frames"):
        dec.decode_q8(q8, counters=True)
    with pytest.raises(ValueError, match="frame 32 is the first of 32 frames"):
        dec.decode_q8(q8, hard_last=True)
    got, n1, n2 = _q8_outputs(dec, q8, on_invalid="mark")
    assert n1.endswith("+q8") and n2.endswith(",word]+q8")
    exp = _marked_expectation(want, B, dec.T)
    keep = torch.tensor([b for b in range(B) if not 32 <= b < 64], device=cuda_device)
    exp["counters"] = exp["word_counters"] = _counters_of_kept(dec, llr, keep)
    for k in exp:
        assert np.array_equal(got[k], exp[k]), (k, case)


def test_bytes_past_the_batch_change_nothing(cuda_device):
    """0x80 in the rows past B of a ragged last pack (the storage goes on behind the batch): the
    kernel reads no row past B and masks the pack's missing frames, so nothing changes and nothing
    is marked."""
    import torch
    dec, cp = _wman(cuda_device)
    llr = _rows(dec, cp)
    want, fname = _float_outputs(dec, llr)
    store = torch.full((96, dec.n_vars), -128, dtype=torch.int8, device=cuda_device)
    store[:B] = dec.quantize_q8(llr)
    got, n1, _ = _q8_outputs(dec, store[:B])
    assert n1 == fname + "+q8"
    for k in want:
        assert np.array_equal(got[k], want[k]), k


# ---- 6. the channel ----------------------------------------------------------------------------
def test_awgn_q8_is_the_channel_quantized(cuda_device):
    """5G BG2 (punctured and shortened ranges): awgn_q8 == the oracle's levels + kmin, 0 on the
    punctured and -128 on the shortened bits, == quantize_q8(awgn)."""
    from oracle import philox_oracle
    c = load_case("g5bg2_222_q5_snr2.0")
    dec = _fixture_decoder(c, cuda_device)
    llr0 = np.asarray(c["llr"])
    n = dec.n_vars
    shortened = np.flatnonzero((llr0 == -dec.clip).all(axis=0))
    punct = np.flatnonzero((llr0 == 0).all(axis=0))
    assert shortened.size and punct.size
    ss, se = int(shortened[0]) + 1, int(shortened[-1]) + 1
    ps, pe = int(punct[0]) + 1, int(punct[-1]) + 1
    assert se - ss + 1 == shortened.size and pe - ps + 1 == punct.size
    sigma, seed = 0.8, 5
    got = dec.awgn_q8(B, sigma, seed, offset=37, punct=(ps, pe), short=(ss, se))
    assert got.dtype.is_floating_point is False and tuple(got.shape) == (B, n)
    llr = dec.awgn(B, sigma, seed, offset=37, punct=(ps, pe), short=(ss, se))
    assert np.array_equal(got.cpu().numpy(), dec.quantize_q8(llr).cpu().numpy())
    lev = philox_oracle.awgn_qms_levels(B, n, sigma, seed, 37, dec.q_bit)
    kmin = philox_oracle.qms_levels(sigma, dec.q_bit)[2]
    want = (np.asarray(lev).astype(np.int64) + int(kmin)).astype(np.int8)
    want[:, ps - 1:pe] = 0
    want[:, ss - 1:se] = -128
    assert np.array_equal(got.cpu().numpy(), want)


# ---- 7. unsupported and unchanged --------------------------------------------------------------
def test_q6_is_unsupported_and_falls_back(cuda_device):
    import torch
    from ldpc_error_floor_amd.decoder import NMSDecoder
    c = load_case("wman_222_q6")
    dec = _fixture_decoder(c, cuda_device)
    assert dec.q_bit == 6 and not dec.supports_q8() and not dec.supports_q8(word=True)
    nb = 40
    rs = np.random.RandomState(2)
    q8 = torch.from_numpy(rs.randint(-9, 10, size=(nb, dec.n_vars)).astype(np.int8)).to(cuda_device)
    want = dec.decode(dec.dequantize_q8(q8), app=False, counters=True, flags=True)
    before = dec.last_kernel()
    cnt = torch.zeros(4, dtype=torch.int64, device=cuda_device)
    with pytest.raises(RuntimeError, match="ldpc_decode_q8"):
        dec._ext.decode_q8(dec._ctx, q8.data_ptr(), nb, dec.T, dec.decoding_type, dec.q_bit, dec.target_bits,
                           dec.clip, 0, cnt.data_ptr(), 0, 0, torch.cuda.current_stream(cuda_device).cuda_stream)
    torch.cuda.synchronize()
    assert dec.last_kernel() == before and not cnt.any().item()
    got = dec.decode_q8(q8, counters=True, flags=True)
    assert dec.last_kernel() == before
    assert np.array_equal(got.counters.cpu().numpy(), want.counters.cpu().numpy())
    assert np.array_equal(got.flags.cpu().numpy(), want.flags.cpu().numpy())


def test_float_decode_is_unchanged_after_a_q8_decode(cuda_device):
    from ldpc_error_floor_amd.decoder import NMSDecoder
    dec, cp = _wman(cuda_device)
    llr = _rows(dec, cp)
    fresh = NMSDecoder(dec.graph.proto, 24, dec.weights, 2, 5, device=cuda_device)
    alone = fresh.decode(llr, app=False, counters=True, flags=True)
    name = fresh.last_kernel()
    dec.decode_q8(dec.quantize_q8(llr), counters=True)
    after = dec.decode(llr, app=False, counters=True, flags=True)
    assert dec.last_kernel() == name and not name.endswith("+q8")
    assert np.array_equal(after.counters.cpu().numpy(), alone.counters.cpu().numpy())
    assert np.array_equal(after.flags.cpu().numpy(), alone.flags.cpu().numpy())
