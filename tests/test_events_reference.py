"""The events mode's test-only reference (tests/_events_ref.py) on a hand-built
example, and the host table ``events.FloorEvents`` (numpy only).  CPU only.

The code: proto [[0, 1, 0]], z = 2 -- check 0 = x0 + x3 + x4, check 1 = x1 + x2 + x5.
x = 100100 is a codeword (a = 2, b = 0); y = 100001 opens both checks (a = 2, b = 2).
Two frames, T = 2:
  frame 0: y at t = 0, x at t = 1 -- never at a zero word; the syndrome closes at t = 1, where the
           frame stops on the wrong codeword x: an undetected error, in both modes;
  frame 1: the zero word at t = 0, y at t = 1 -- early stop freezes it at t = 0 (no event, n_iter 1);
           the full-T decode ends on y."""
import numpy as np
import pytest

from _events_ref import as_tuples, events_of_words, events_reference
from ldpc_error_floor_amd.events import FloorEvents
from oracle import nms_oracle

PROTO, Z = np.array([[0, 1, 0]]), 2
X = np.array([1, 0, 0, 1, 0, 0], np.uint8)
Y = np.array([1, 0, 0, 0, 0, 1], np.uint8)
O = np.zeros(6, np.uint8)


def _example():
    hard = np.array([[Y, O], [X, Y]], np.uint8)                 # [T, B, 6]
    synd = nms_oracle.syndromes(hard, nms_oracle.lifted_edges(PROTO, Z))
    assert synd.tolist() == [[[1, 1], [0, 0]], [[0, 0], [1, 1]]]
    return hard, synd


def test_early_stop_events_of_the_example():
    hard, synd = _example()
    ev, ref = events_reference(hard, synd, target_bits=2, early_stop=True, frame_base=100)
    assert ref["n_iter"].tolist() == [2, 1]
    assert as_tuples(ev) == [(100, 2, 2, 0)]                     # (frame, n_iter, a, b): frame 0 alone
    assert ev["a_target"].tolist() == [1]
    assert ev["words"].tolist() == [[0b001001]]
    assert int(ev["a_target"].sum()) == ref["counters"][0] and int((ev["a_target"] > 0).sum()) == ref["counters"][1]


def test_full_t_events_of_the_example():
    hard, synd = _example()
    ev, ref = events_reference(hard, synd, target_bits=2, early_stop=False)
    assert as_tuples(ev) == [(0, 2, 2, 0), (1, 2, 2, 2)]
    assert ev["a_target"].tolist() == [1, 1] and ref["counters"].tolist() == [2, 2]
    assert ev["words"].tolist() == [[0b001001], [0b100001]]


def test_a_target_counts_the_first_bits_only():
    ev = events_of_words(np.array([Y, O, X]), np.array([[1, 1], [0, 0], [0, 0]]), [3, 1, 2], target_bits=4, frame_base=7)
    assert as_tuples(ev) == [(7, 3, 2, 2), (9, 2, 2, 0)]
    assert ev["a_target"].tolist() == [1, 2]


def _table(frames, n_vars=40, seed=0):
    rs = np.random.RandomState(seed)
    n = len(frames)
    bits = rs.randint(0, 2, (n, n_vars)).astype(np.uint8)
    bits[:, 0] = 1
    pad = np.concatenate([bits, np.zeros((n, 64 - n_vars), np.uint8)], axis=1)
    words = np.packbits(pad, axis=1, bitorder="little").view(np.uint32)
    return FloorEvents(np.array(frames), rs.randint(1, 20, n), bits.sum(axis=1), bits[:, :8].sum(axis=1),
                       rs.randint(0, 3, n), words, n_vars), bits


def test_floor_events_sorts_by_frame_and_keeps_rows_together():
    t, bits = _table([50, 3, 17, 4])
    order = [1, 3, 2, 0]
    assert t.frame.tolist() == [3, 4, 17, 50] and len(t) == 4
    assert t.a.tolist() == bits.sum(axis=1)[order].tolist()
    for i, o in enumerate(order):
        assert np.array_equal(t.bits(i), bits[o]) and t.bits(i).shape == (40,)
    assert t.frame.dtype == np.int64 and t.a.dtype == np.int32 and t.words.dtype == np.uint32


def test_concat_is_sorted_and_equals_the_whole():
    whole, _ = _table([1, 2, 30, 31, 32, 70])
    pick = lambda idx: FloorEvents(whole.frame[idx], whole.n_iter[idx], whole.a[idx], whole.a_target[idx],  # noqa: E731
                                   whole.b[idx], whole.words[idx], whole.n_vars)
    parts = [pick([4, 5]), pick([0, 1, 2, 3])]                   # given out of order
    assert FloorEvents.concat(parts) == whole
    assert FloorEvents.concat([whole, FloorEvents.empty(40)]) == whole
    assert len(FloorEvents.concat([])) == 0
    with pytest.raises(ValueError, match="word lengths"):
        FloorEvents.concat([whole, FloorEvents.empty(41)])
    nowords = FloorEvents(whole.frame, whole.n_iter, whole.a, whole.a_target, whole.b, None, 40)
    assert FloorEvents.concat([nowords, FloorEvents.empty(40)]).words is None
    assert nowords != whole
    with pytest.raises(ValueError, match="no words"):
        nowords.bits(0)


def test_ab_histogram_and_undetected():
    z = np.zeros(5, np.int32)
    t = FloorEvents([5, 1, 2, 9, 7], z + 3, [1, 1, 12, 4, 1], z, [1, 1, 0, 6, 2])
    assert t.ab_histogram() == {(1, 1): 2, (1, 2): 1, (4, 6): 1, (12, 0): 1}
    assert t.frame[t.undetected()].tolist() == [2]
    assert "undetected" in t.format() and "5 events" in t.format()


def test_npz_round_trip(tmp_path):
    t, _ = _table([9, 8, 1 << 40])
    p = tmp_path / "ev.npz"
    t.save(p)
    assert FloorEvents.load(p) == t
    assert FloorEvents.load(p).frame[-1] == 1 << 40
    nw = FloorEvents(t.frame, t.n_iter, t.a, t.a_target, t.b, None, 40)
    nw.save(tmp_path / "bare")
    back = FloorEvents.load(tmp_path / "bare")
    assert back == nw and back.words is None
    e = FloorEvents.empty(40)
    e.save(p)
    assert FloorEvents.load(p) == e and FloorEvents.load(p).words.shape == (0, 2)


def test_mismatched_columns_are_refused():
    with pytest.raises(ValueError, match="entries"):
        FloorEvents([1, 2], [1], [1, 1], [1, 1], [1, 1])
    with pytest.raises(ValueError, match="words"):
        FloorEvents([1, 2], [1, 1], [1, 1], [1, 1], [1, 1], np.zeros((3, 2), np.uint32), 40)
