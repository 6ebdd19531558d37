"""Argument handling of ``decode(early_stop=True, hard_last=...)`` and ``decode_awgn`` (DESIGN.md
3.9) on an NMSDecoder shell without a device: the combination reaches the early-stop word decode
instead of being refused, the exports neither mode serves stay refused with the early-stop mode's
message, and ``decode_awgn(hard_last=True)`` without ``early_stop`` still raises."""
import pytest

from ldpc_error_floor_amd.decoder import NMSDecoder


class _Llr:
    shape = (5, 96)


@pytest.fixture()
def shell(monkeypatch):
    import torch
    dec = object.__new__(NMSDecoder)
    dec._torch = torch
    dec.T, dec.target_bits, dec.n_vars = 10, 48, 96
    dec.punct, dec.short = (1, 8), (0, 0)
    calls = []
    monkeypatch.setattr(NMSDecoder, "_as_llr", lambda self, llr: llr)
    monkeypatch.setattr(NMSDecoder, "_decode_es_word", lambda self, *a, **kw: calls.append((a, kw)) or "res")
    return dec, calls


def test_decode_accepts_early_stop_with_hard_last(shell):
    dec, calls = shell
    llr = _Llr()
    assert dec.decode(llr, early_stop=True, hard_last=True, word_flags=True, n_iter=True, iter_hist=True,
                      counters=True, flags=True, on_off_grid="mark") == "res"
    (a, kw), = calls
    assert a[0] is llr and a[1] == 5 and a[2] == 10 and a[3] == 48      # llr, B, T, target bits
    assert a[4] is True and a[5] is True                                # hard_last, word_flags
    assert a[-1] == "mark" and not kw


@pytest.mark.parametrize("export", ["app", "hard", "synd", "iter_wrong"])
def test_other_exports_stay_refused(shell, export):
    dec, calls = shell
    with pytest.raises(ValueError, match="early_stop serves counters, flags, n_iter and iter_hist only"):
        dec.decode(_Llr(), early_stop=True, hard_last=True, **{export: True})
    with pytest.raises(ValueError, match="hard_last serves word_flags, counters and flags only"):
        dec.decode(_Llr(), hard_last=True, **{export: True})
    assert not calls


def test_decode_awgn(shell):
    dec, calls = shell
    with pytest.raises(ValueError, match="decode_awgn does not serve hard_last"):
        dec.decode_awgn(8, 0.5, 1, hard_last=True)
    with pytest.raises(ValueError, match="word_flags is an output of hard_last"):
        dec.decode_awgn(8, 0.5, 1, early_stop=True, word_flags=True)
    with pytest.raises(ValueError, match="early_stop serves"):
        dec.decode_awgn(8, 0.5, 1, early_stop=True, hard_last=True, app=True)
    assert not calls
    assert dec.decode_awgn(8, 0.5, 3, offset=7, early_stop=True, hard_last=True, word_flags=True) == "res"
    (a, kw), = calls
    assert a[0] is None and a[1] == 8 and a[2] == 10 and a[3] == 48
    assert kw == {"channel": (0.5, 3, 7, (1, 8), (0, 0))}
