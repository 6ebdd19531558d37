"""Argument handling of ``NMSDecoder.decode_q8`` and the q8 byte format's host side
on an NMSDecoder shell without a device: ``quantize_q8`` / ``dequantize_q8`` round-trip the grid
values and +-clip on all four grids and refuse anything else under ``strict``; ``decode_q8`` reaches
the native int8 entry points where ``supports_q8`` holds, dequantizes and calls ``decode`` where it
does not or an export the int8 builds lack is asked for, and refuses bad arguments itself."""
import numpy as np
import pytest

from ldpc_error_floor_amd.decoder import NMSDecoder, Q8_GRIDS
from ldpc_error_floor_amd.config import DECODING_MS, DECODING_QMS

N_VARS = 12


class _S:
    """A stream: the native calls take its handle, ``on_invalid="raise"`` waits for it."""
    cuda_stream = 0

    def synchronize(self):
        pass


class _Ext:
    """The extension's q8 entry points, recording their calls."""
    def __init__(self, supported):
        self.supported, self.calls = supported, []

    def q8_supported(self, ctx, T, dt, q, nt, kern, clip, has_short, word):
        return self.supported

    def decode_q8(self, *a):
        self.calls.append(("decode_q8", a))

    def decode_q8_word(self, *a):
        self.calls.append(("decode_q8_word", a))


def shell(monkeypatch, q_bit=5, supported=True, decoding_type=DECODING_QMS):
    import torch
    dec = object.__new__(NMSDecoder)
    dec._torch = torch
    dec.device = torch.device("cpu")
    dec.T, dec.target_bits, dec.n_vars = 10, 8, N_VARS
    dec.decoding_type, dec.q_bit, dec.clip, dec.kernel = decoding_type, q_bit, 20.0, "auto"
    dec._ext = _Ext(supported)
    monkeypatch.setattr(NMSDecoder, "_ensure_ctx", lambda self, B, T: "ctx")
    fell = []
    monkeypatch.setattr(NMSDecoder, "decode", lambda self, llr, **kw: fell.append((llr, kw)) or "float-result")
    return dec, fell


@pytest.mark.parametrize("q_bit", sorted(Q8_GRIDS))
def test_round_trip_of_every_grid_value_and_clip(monkeypatch, q_bit):
    dec, _ = shell(monkeypatch, q_bit)
    step, qmax = Q8_GRIDS[q_bit]
    x = np.array([g * step for g in range(-qmax, qmax + 1)] + [-20.0, 20.0], np.float32)
    q = dec.quantize_q8(x)
    assert q.dtype == dec._torch.int8 and q.shape == x.shape
    assert q.numpy().tolist() == list(range(-qmax, qmax + 1)) + [-128, 127]
    assert np.array_equal(dec.dequantize_q8(q).numpy(), x)
    assert np.array_equal(dec.dequantize_q8(q.numpy()).numpy(), x)


@pytest.mark.parametrize("q_bit", sorted(Q8_GRIDS))
def test_strict_refuses_what_has_no_byte(monkeypatch, q_bit):
    dec, _ = shell(monkeypatch, q_bit)
    step, qmax = Q8_GRIDS[q_bit]
    for bad in (step / 2, (qmax + 1) * step, -(qmax + 1) * step, 19.5, float("nan")):
        x = np.array([0.0, bad, step], np.float32)
        with pytest.raises(ValueError, match="quantize_q8: 1 values"):
            dec.quantize_q8(x)
        q = dec.quantize_q8(x, strict=False).numpy()
        assert q[0] == 0 and q[2] == 1 and -qmax <= q[1] <= qmax


def test_native_path_counters_only(monkeypatch):
    dec, fell = shell(monkeypatch)
    torch = dec._torch
    q8 = torch.zeros((5, N_VARS), dtype=torch.int8)
    res = dec.decode_q8(q8, T=7, counters=True, flags=True, iter_wrong=True, on_invalid="mark", stream=_S())
    assert not fell
    (name, a), = dec._ext.calls
    assert name == "decode_q8"
    assert a[0] == "ctx" and a[1] == q8.data_ptr() and a[2] == 5 and a[3] == 7      # ctx, q8, B, T
    assert a[4] == DECODING_QMS and a[5] == 5 and a[6] == 8                          # mode, q, target bits
    assert a[9] == res.counters.data_ptr() and a[10] == res.flags.data_ptr() and a[11] == res.iter_wrong.data_ptr()
    assert res.iter_wrong.shape == (7, 1) and res.flags.shape == (5,) and res.hard_last is None


def test_native_path_word(monkeypatch):
    dec, fell = shell(monkeypatch)
    torch = dec._torch
    q8 = np.zeros((3, N_VARS), np.int8)
    res = dec.decode_q8(q8, hard_last=True, word_flags=True, on_invalid="mark", stream=_S())
    assert not fell
    (name, a), = dec._ext.calls
    assert name == "decode_q8_word" and a[2] == 3 and a[3] == 10
    assert a[9] == res.hard_last.data_ptr() and a[10] == res.word_flags.data_ptr() and a[11] == 0 and a[12] == 0
    assert res.hard_last.dtype == torch.int32 and res.hard_last.shape == (3, 1)


def test_raise_names_the_first_marked_frame(monkeypatch):
    dec, _ = shell(monkeypatch)
    torch = dec._torch

    def marking(*a):
        flags = a[10]
        import ctypes
        buf = (ctypes.c_uint8 * 70).from_address(flags)
        for b in range(70):
            buf[b] = 0x80 if 32 <= b < 64 else 0
    dec._ext.decode_q8 = marking
    q8 = torch.zeros((70, N_VARS), dtype=torch.int8)
    with pytest.raises(ValueError, match="frame 32 is the first of 32 frames"):
        dec.decode_q8(q8, stream=_S())
    res = dec.decode_q8(q8, stream=_S(), on_invalid="mark", flags=True)
    assert res.flags.tolist() == [0x80 if 32 <= b < 64 else 0 for b in range(70)]


@pytest.mark.parametrize("why", ["unsupported", "app", "hard", "synd", "q6", "float"])
def test_fallback_dequantizes_and_calls_decode(monkeypatch, why):
    kw = {}
    if why == "q6":
        dec, fell = shell(monkeypatch, q_bit=6)
    elif why == "float":
        dec, fell = shell(monkeypatch, decoding_type=DECODING_MS)
    else:
        dec, fell = shell(monkeypatch, supported=why != "unsupported")
        if why != "unsupported":
            kw[why] = True
    assert dec.supports_q8() == (why in ("app", "hard", "synd"))
    step = 1.0 if why in ("q6", "float") else 0.5
    q8 = np.array([[-15, 15, 0, 1, -1, 7, -128, 127, 2, 3, 4, 5]], np.int8)
    assert dec.decode_q8(q8, counters=True, on_invalid="raise", **kw) == "float-result"
    assert not dec._ext.calls
    (llr, got), = fell
    want = q8.astype(np.float32) * step
    want[0, 6], want[0, 7] = -20.0, 20.0
    assert np.array_equal(llr.numpy(), want)
    assert got["counters"] is True and got["on_off_grid"] == "mark"
    for k in ("app", "hard", "synd"):
        assert got[k] == bool(kw.get(k, False))
    # an invalid byte: "raise" names the frame before anything is decoded, "mark" decodes
    bad = np.zeros((3, N_VARS), np.int8)
    bad[2, 4] = 100 if why not in ("q6", "float") else -127
    with pytest.raises(ValueError, match="frame 2 holds a byte that is no q8 value"):
        dec.decode_q8(bad, **kw)
    assert len(fell) == 1
    assert dec.decode_q8(bad, on_invalid="mark", **kw) == "float-result"


def test_bad_arguments(monkeypatch):
    dec, fell = shell(monkeypatch)
    q8 = np.zeros((2, N_VARS), np.int8)
    with pytest.raises(ValueError, match="on_invalid must be"):
        dec.decode_q8(q8, on_invalid="ignore")
    with pytest.raises(ValueError, match="exceeds the 10 iterations"):
        dec.decode_q8(q8, T=11)
    with pytest.raises(ValueError, match="word_flags is an output of hard_last"):
        dec.decode_q8(q8, word_flags=True)
    with pytest.raises(ValueError, match="not iter_wrong"):
        dec.decode_q8(q8, hard_last=True, iter_wrong=True)
    with pytest.raises(ValueError, match="q8 must be int8"):
        dec.decode_q8(q8.astype(np.float32))
    with pytest.raises(ValueError, match="q8 has 11 bits per codeword"):
        dec.decode_q8(np.zeros((2, 11), np.int8))
    with pytest.raises(ValueError, match="awgn_q8 covers"):
        shell(monkeypatch, q_bit=6)[0].awgn_q8(4, 0.5, 1)
    assert not fell and not dec._ext.calls
