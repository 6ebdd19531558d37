"""The test-only reference of the early-stop decoded word (tests/_es_word_ref.py) on hand-made
per-iteration arrays: T = 4, five variables, two checks.  Frame 0 stops at t = 0; frame 1 stops at
t = 1, its syndrome reopens at t = 2 and its later hard decisions differ; frame 2 never stops;
frame 3's only zero syndrome is at T - 1."""
import numpy as np

from _es_word_ref import es_word_reference, pack_bits

T, NV, NC = 4, 5, 2


def _arrays():
    hard = np.zeros((T, 4, NV), np.uint8)
    synd = np.zeros((T, 4, NC), np.uint8)
    # frame 0: zero syndrome at once; later iterations hold other bits (never returned)
    hard[0, 0] = [1, 0, 1, 0, 0]
    hard[1:, 0] = [0, 1, 0, 1, 1]
    # frame 1: open, closed at t = 1, reopens at t = 2, closed again at t = 3
    hard[0, 1] = [1, 1, 1, 1, 1]
    hard[1, 1] = [0, 1, 0, 0, 1]
    hard[2, 1] = [1, 0, 0, 0, 0]
    hard[3, 1] = [0, 0, 0, 0, 0]
    synd[0, 1] = [1, 0]
    synd[2, 1] = [0, 1]
    # frame 2: never a zero syndrome
    hard[:, 2] = [[1, 0, 0, 0, 0], [1, 1, 0, 0, 0], [1, 1, 1, 0, 0], [0, 0, 0, 1, 1]]
    synd[:, 2] = [[1, 1], [1, 0], [0, 1], [1, 0]]
    # frame 3: the only zero syndrome is the last iteration's
    hard[:, 3] = [[0, 0, 0, 0, 1], [0, 0, 0, 1, 0], [0, 0, 1, 0, 0], [0, 1, 0, 0, 1]]
    synd[:3, 3] = [[0, 1], [1, 1], [1, 0]]
    return hard, synd


def test_stop_rule_and_word():
    hard, synd = _arrays()
    ref = es_word_reference(hard, synd, 3)
    assert ref["stop"].tolist() == [0, 1, 3, 3]
    assert ref["n_iter"].tolist() == [1, 2, 4, 4]
    assert ref["hd_stop"].tolist() == [[1, 0, 1, 0, 0], [0, 1, 0, 0, 1], [0, 0, 0, 1, 1], [0, 1, 0, 0, 1]]
    # bit v of word 0; bits 5 .. 31 zero
    assert ref["hard_stop"].tolist() == [[0b00101], [0b10010], [0b11000], [0b10010]]
    assert ref["hard_stop"].dtype == np.uint32
    # only the frame that never stops is not a codeword; T - 1's zero syndrome clears frame 3's flag
    assert ref["word_flags"].tolist() == [0, 0, 1, 0]
    # the early-stop outputs are tests/_es_ref.py's (target bits 0 .. 2)
    assert ref["iter_hist"].tolist() == [1, 1, 0, 2]
    assert ref["counters"].tolist() == [2 + 1 + 0 + 1, 3, 2, 0]
    assert ref["flags"].tolist() == [3, 3, 0, 2]


def test_frozen_at_stop_whatever_follows():
    """Changing what follows a frame's stop iteration changes nothing of its outputs."""
    hard, synd = _arrays()
    ref = es_word_reference(hard, synd, 3)
    hard[1:, 0] ^= 1
    synd[1:, 0] = 1
    hard[2:, 1] ^= 1
    synd[2:, 1] = 1
    again = es_word_reference(hard, synd, 3)
    for k in ("stop", "hd_stop", "hard_stop", "word_flags", "n_iter", "flags", "counters", "iter_hist"):
        assert np.array_equal(ref[k], again[k]), k


def test_pack_bits_layout():
    bits = np.zeros((2, 70), np.uint8)
    bits[0, [0, 31, 32, 69]] = 1
    bits[1, 33] = 1
    w = pack_bits(bits)
    assert w.shape == (2, 3) and w.dtype == np.uint32
    assert w.tolist() == [[0x80000001, 1, 1 << 5], [0, 2, 0]]
