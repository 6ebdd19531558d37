"""Argument handling of ``decode(events=...)`` and ``decode_awgn(events=...)`` on an
NMSDecoder shell without a device: ``events`` reaches the events decode with the frame base (the
channel's offset for ``decode_awgn``), the outputs it does not serve raise ``ValueError``, and
``decode_awgn`` without ``early_stop`` raises as ``hard_last`` does there."""
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
    monkeypatch.setattr(NMSDecoder, "_decode_events", lambda self, *a, **kw: calls.append((a, kw)) or "res")
    return dec, calls


BUF = object()


@pytest.mark.parametrize("early_stop", [False, True])
def test_decode_reaches_the_events_decode(shell, early_stop):
    dec, calls = shell
    llr = _Llr()
    kw = dict(n_iter=True, iter_hist=True) if early_stop else {}
    assert dec.decode(llr, events=BUF, frame_base=1000, early_stop=early_stop, counters=True, flags=True,
                      on_off_grid="mark", **kw) == "res"
    (a, k), = calls
    assert a[0] is llr and a[1:4] == (5, 10, 48)                 # llr, B, T, target bits
    assert a[4] is BUF and a[5] == 1000 and a[6] is early_stop   # buffer, frame base, mode
    assert a[-1] == "mark" and not k


@pytest.mark.parametrize("export", ["hard_last", "app", "hard", "synd", "iter_wrong", "word_flags"])
@pytest.mark.parametrize("early_stop", [False, True])
def test_other_outputs_raise_with_events(shell, export, early_stop):
    dec, calls = shell
    with pytest.raises(ValueError, match="events serves counters and flags"):
        dec.decode(_Llr(), events=BUF, early_stop=early_stop, **{export: True})
    assert not calls


@pytest.mark.parametrize("export", ["n_iter", "iter_hist"])
def test_early_stop_outputs_need_early_stop(shell, export):
    dec, calls = shell
    with pytest.raises(ValueError, match="events serves counters and flags"):
        dec.decode(_Llr(), events=BUF, **{export: True})
    assert not calls


def test_decode_awgn(shell):
    dec, calls = shell
    with pytest.raises(ValueError, match="decode_awgn does not serve events without early_stop"):
        dec.decode_awgn(8, 0.5, 1, events=BUF)
    for export in ("hard_last", "app", "iter_wrong", "word_flags"):
        with pytest.raises(ValueError, match="events serves counters and flags"):
            dec.decode_awgn(8, 0.5, 1, early_stop=True, events=BUF, **{export: True})
    with pytest.raises(ValueError, match="exceeds"):
        dec.decode_awgn(8, 0.5, 1, early_stop=True, events=BUF, T=11)
    assert not calls
    assert dec.decode_awgn(8, 0.5, 3, offset=7, early_stop=True, events=BUF, n_iter=True) == "res"
    (a, kw), = calls
    assert a[0] is None and a[1:4] == (8, 10, 48) and a[4] is BUF and a[6] is True
    assert kw == {"channel": (0.5, 3, 7, (1, 8), (0, 0))}
