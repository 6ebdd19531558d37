"""Test-only reference of the early-stop mode's decoded word (include/ldpc_nms.h:
ldpc_decode_es_word): ``hard_stop`` and ``word_flags`` derived from the per-iteration hard decisions
and syndromes of ``nms_oracle.decode``, with the stop rule of ``tests/_es_ref.py``.  Never used by
the product.

Per codeword b: stop(b) = the smallest t with syndrome s_t == 0, else T - 1; hard_stop[b] =
hard[stop(b), b] over all N*z variables, whatever later iterations hold; word_flags[b] = [the
syndrome of hard_stop[b] is nonzero] = synd[stop(b), b].any().
"""
import numpy as np

from _es_ref import es_reference


def pack_bits(bits):
    """[..., n] 0/1 -> [..., ceil(n/32)] uint32, bit v % 32 of word v // 32, the bits past n zero."""
    bits = np.asarray(bits).astype(np.uint8)
    pad = (-bits.shape[-1]) % 32
    if pad:
        bits = np.concatenate([bits, np.zeros(bits.shape[:-1] + (pad,), np.uint8)], axis=-1)
    return np.ascontiguousarray(np.packbits(bits, axis=-1, bitorder="little")).view(np.uint32)


def es_word_reference(hard, synd, target_bits):
    """``hard`` [T, B, N*z], ``synd`` [T, B, M*z] (0/1) -> ``es_reference``'s dict and ``stop`` int
    [B], ``hd_stop`` uint8 [B, N*z], ``hard_stop`` uint32 [B, ceil(N*z/32)] (packed) and
    ``word_flags`` uint8 [B]."""
    hard = np.asarray(hard).astype(bool)
    synd = np.asarray(synd).astype(bool)
    ref = es_reference(hard, synd, target_bits)
    stop = ref["n_iter"].astype(int) - 1
    b = np.arange(hard.shape[1])
    hd_stop = hard[stop, b, :].astype(np.uint8)
    ref.update(stop=stop, hd_stop=hd_stop, hard_stop=pack_bits(hd_stop),
               word_flags=synd[stop, b, :].any(axis=1).astype(np.uint8))
    return ref
