"""Test-only reference of the early-stop mode (include/ldpc_nms.h): the mode's
outputs derived from the per-iteration hard decisions and syndromes of ``nms_oracle.decode``.
Never used by the product.

Per codeword b (all-zero codeword): stop(b) = the smallest t with syndrome s_t == 0, else T - 1;
n_iter = stop + 1; every output is taken at stop(b), whatever the syndrome does afterwards.
"""
import numpy as np

from oracle import nms_oracle


def es_reference(hard, synd, target_bits):
    """``hard`` [T, B, N*z], ``synd`` [T, B, M*z] (0/1) -> dict with ``n_iter`` uint8 [B],
    ``flags`` uint8 [B] (bit 0 wrong at every t <= stop, bit 1 wrong at stop), ``counters``
    int64 [4] ({bit errors at stop, frames wrong at stop, frames wrong at every t <= stop, 0}) and
    ``iter_hist`` int64 [T]."""
    hard = np.asarray(hard).astype(bool)
    synd = np.asarray(synd).astype(bool)
    T, B = hard.shape[0], hard.shape[1]
    zero = ~synd.any(axis=2)                                 # [T, B]: s_t == 0
    stop = np.where(zero.any(axis=0), zero.argmax(axis=0), T - 1)
    wrong = hard[:, :, :target_bits].any(axis=2)             # [T, B]
    b = np.arange(B)
    hd_stop = hard[stop, b, :target_bits]                    # [B, target_bits]
    wrong_stop = wrong[stop, b]
    upto = np.arange(T)[:, None] <= stop[None, :]            # [T, B]: t <= stop(b)
    wrong_all = (wrong | ~upto).all(axis=0)
    n_iter = (stop + 1).astype(np.uint8)
    return {"n_iter": n_iter,
            "flags": wrong_all.astype(np.uint8) | (wrong_stop.astype(np.uint8) << 1),
            "counters": np.array([hd_stop.sum(), wrong_stop.sum(), wrong_all.sum(), 0], np.int64),
            "iter_hist": np.bincount(stop, minlength=T).astype(np.int64)}


def es_oracle(llr, proto, z, W, T, q_bit, target_bits, graph=None):
    """The reference on the oracle's decode of ``llr`` [B, N*z] (QMS, decoding_type 2)."""
    out = nms_oracle.decode(np.asarray(llr, np.float32), proto, z, W.alpha, W.alpha_ucn, W.beta, T, 2,
                            q_bit, graph=graph)
    return es_reference(out["hard"], out["synd"], target_bits)
