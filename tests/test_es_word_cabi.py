"""The early-stop decoded-word entry points of the C ABI (include/ldpc_nms.h: ldpc_decode_es_word,
ldpc_decode_awgn_es_word, ldpc_es_word_supported; CPU only -- no compute calls):
exported, the outputs struct checked before anything else is read, and the ABI version unchanged
(the mode adds entry points and a size-declared struct of its own; ldpc_es_outputs keeps its size,
which tests/test_es_cabi.py pins)."""
import ctypes
import os

import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "ldpc_error_floor_amd", "libldpc_nms.so")
ERR_ARG = -1


class Params(ctypes.Structure):
    _fields_ = [("T", ctypes.c_int32), ("decoding_type", ctypes.c_int32), ("q_bit", ctypes.c_int32),
                ("target_bits", ctypes.c_int32), ("clip_llr", ctypes.c_float), ("kernel", ctypes.c_int32),
                ("outputs_size", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class Channel(ctypes.Structure):
    _fields_ = [("sigma", ctypes.c_double), ("seed", ctypes.c_uint64), ("offset", ctypes.c_int64),
                ("punct_start", ctypes.c_int32), ("punct_end", ctypes.c_int32),
                ("short_start", ctypes.c_int32), ("short_end", ctypes.c_int32),
                ("reserved", ctypes.c_int32 * 4)]


class EsWordOutputs(ctypes.Structure):
    _fields_ = [("size", ctypes.c_int32), ("reserved", ctypes.c_int32), ("hard_stop", ctypes.c_void_p),
                ("word_flags", ctypes.c_void_p), ("counters", ctypes.c_void_p),
                ("frame_flags", ctypes.c_void_p), ("n_iter", ctypes.c_void_p),
                ("iter_hist", ctypes.c_void_p), ("reserved1", ctypes.c_uint64)]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.fail(f"{LIB} not built: run python -m ldpc_error_floor_amd.build")
    L = ctypes.CDLL(LIB)
    L.ldpc_decode_es_word.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                      ctypes.c_void_p, ctypes.c_void_p]
    L.ldpc_decode_awgn_es_word.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_void_p]
    L.ldpc_es_word_supported.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    return L


def test_symbols_exported(lib):
    for f in ("ldpc_decode_es_word", "ldpc_decode_awgn_es_word", "ldpc_es_word_supported"):
        assert hasattr(lib, f), f


def test_abi_version_unchanged(lib):
    assert lib.ldpc_abi_version() == 3


def test_struct_size():
    assert ctypes.sizeof(EsWordOutputs) == 64


def test_null_arguments_without_gpu(lib):
    p = Params(T=4, decoding_type=2, q_bit=5, target_bits=8, clip_llr=20.0)
    ch = Channel(sigma=0.5, seed=1)
    dummy = ctypes.create_string_buffer(64)
    d = ctypes.addressof(dummy)
    o = EsWordOutputs(size=ctypes.sizeof(EsWordOutputs), hard_stop=d)
    pp, po, pc = ctypes.addressof(p), ctypes.addressof(o), ctypes.addressof(ch)
    assert lib.ldpc_decode_es_word(None, None, 1, None, None, None) == ERR_ARG
    assert lib.ldpc_decode_es_word(None, d, 1, pp, po, None) == ERR_ARG        # null context
    assert lib.ldpc_decode_es_word(d, None, 1, pp, po, None) == ERR_ARG        # null LLRs
    assert lib.ldpc_decode_es_word(d, d, 1, None, po, None) == ERR_ARG
    assert lib.ldpc_decode_es_word(d, d, 1, pp, None, None) == ERR_ARG
    assert lib.ldpc_decode_awgn_es_word(None, 1, pp, pc, po, None) == ERR_ARG
    assert lib.ldpc_decode_awgn_es_word(d, 1, None, pc, po, None) == ERR_ARG
    assert lib.ldpc_decode_awgn_es_word(d, 1, pp, None, po, None) == ERR_ARG
    assert lib.ldpc_decode_awgn_es_word(d, 1, pp, pc, None, None) == ERR_ARG
    assert lib.ldpc_es_word_supported(None, None) == ERR_ARG
    assert lib.ldpc_es_word_supported(None, pp) == ERR_ARG
    assert lib.ldpc_es_word_supported(d, None) == ERR_ARG


def test_bad_size_and_null_hard_stop_are_refused_before_the_context_is_read(lib):
    """``size`` other than sizeof(ldpc_es_word_outputs) (56 would be the struct without its padding
    word), or a null ``hard_stop`` -> LDPC_ERR_ARG.  The context and LLR pointers here are never
    dereferenced: the outputs are checked first."""
    p = Params(T=4, decoding_type=2, q_bit=5, target_bits=8, clip_llr=20.0)
    ch = Channel(sigma=0.5, seed=1)
    dummy = ctypes.create_string_buffer(64)
    d = ctypes.addressof(dummy)
    pp, pc = ctypes.addressof(p), ctypes.addressof(ch)
    for size in (0, 8, 56, 72):
        o = EsWordOutputs(size=size, hard_stop=d)
        assert lib.ldpc_decode_es_word(d, d, 1, pp, ctypes.addressof(o), None) == ERR_ARG, size
        assert lib.ldpc_decode_awgn_es_word(d, 1, pp, pc, ctypes.addressof(o), None) == ERR_ARG, size
    o = EsWordOutputs(size=ctypes.sizeof(EsWordOutputs), hard_stop=None, word_flags=d)
    assert lib.ldpc_decode_es_word(d, d, 1, pp, ctypes.addressof(o), None) == ERR_ARG
    assert lib.ldpc_decode_awgn_es_word(d, 1, pp, pc, ctypes.addressof(o), None) == ERR_ARG
