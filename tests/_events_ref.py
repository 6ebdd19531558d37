"""Test-only reference of the events mode (include/ldpc_nms.h: ldpc_decode_events):
the events of a batch -- the frames whose decoded word is nonzero anywhere over the N*z variables --
with ``a`` (ones of the word), ``a_target`` (ones among the first target bits), ``b`` (ones of its
syndrome) and the packed rows, from the per-iteration hard decisions and syndromes of
``nms_oracle.decode``: at each frame's stop iteration (``es_word_reference``) for the early-stop
decode, at iteration T - 1 for the full-T one.  Never used by the product.
"""
import numpy as np

from _es_word_ref import es_word_reference, pack_bits


def events_of_words(hd, synd, n_iter, target_bits, frame_base=0):
    """``hd`` [B, N*z], ``synd`` [B, M*z] (0/1), ``n_iter`` [B] -> dict of the events in frame
    order: ``frame`` int64 [n] (``frame_base`` + batch index), ``n_iter``, ``a``, ``a_target``,
    ``b`` int32 [n], ``words`` uint32 [n, ceil(N*z/32)]."""
    hd = np.asarray(hd).astype(np.uint8)
    synd = np.asarray(synd).astype(np.uint8)
    idx = np.nonzero(hd.any(axis=1))[0]
    assert not synd[np.setdiff1d(np.arange(hd.shape[0]), idx)].any()      # zero word -> zero syndrome
    w = hd[idx]
    return {"frame": idx.astype(np.int64) + int(frame_base),
            "n_iter": np.asarray(n_iter)[idx].astype(np.int32),
            "a": w.sum(axis=1).astype(np.int32),
            "a_target": w[:, :target_bits].sum(axis=1).astype(np.int32),
            "b": synd[idx].sum(axis=1).astype(np.int32),
            "words": pack_bits(w).reshape(idx.size, -1)}


def events_reference(hard, synd, target_bits, early_stop, frame_base=0):
    """``hard`` [T, B, N*z], ``synd`` [T, B, M*z] of ``nms_oracle.decode`` -> ``(events,
    decode)``: ``events_of_words`` of each frame's word at its stop iteration (``early_stop``) or
    at iteration T - 1, and the decode's own reference outputs (``es_word_reference``'s dict, or
    ``counters`` [bit errors, frame errors] of iteration T - 1)."""
    hard = np.asarray(hard).astype(bool)
    synd = np.asarray(synd).astype(bool)
    T, B = hard.shape[0], hard.shape[1]
    if early_stop:
        ref = es_word_reference(hard, synd, target_bits)
        b = np.arange(B)
        return events_of_words(ref["hd_stop"], synd[ref["stop"], b], ref["n_iter"], target_bits, frame_base), ref
    last = hard[T - 1]
    ref = {"counters": np.array([last[:, :target_bits].sum(), last[:, :target_bits].any(axis=1).sum()], np.int64)}
    return events_of_words(last, synd[T - 1], np.full(B, T), target_bits, frame_base), ref


def as_tuples(ev):
    """[(frame, n_iter, a, b)] of an events dict or a ``FloorEvents``."""
    g = (lambda k: ev[k]) if isinstance(ev, dict) else (lambda k: getattr(ev, k))
    return list(zip(g("frame").tolist(), g("n_iter").tolist(), g("a").tolist(), g("b").tolist()))
