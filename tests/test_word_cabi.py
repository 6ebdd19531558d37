"""The decoded-word entry points of the C ABI (include/ldpc_nms.h: ldpc_decode_word,
ldpc_word_supported; CPU only -- no compute calls): exported, arguments validated before anything
touches a GPU, and the ABI version unchanged (the mode adds entry points and a size-declared struct
of its own; no existing struct changes)."""
import ctypes
import os

import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "ldpc_error_floor_amd", "libldpc_nms.so")


class Params(ctypes.Structure):
    _fields_ = [("T", ctypes.c_int32), ("decoding_type", ctypes.c_int32), ("q_bit", ctypes.c_int32),
                ("target_bits", ctypes.c_int32), ("clip_llr", ctypes.c_float), ("kernel", ctypes.c_int32),
                ("outputs_size", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class WordOutputs(ctypes.Structure):
    _fields_ = [("size", ctypes.c_int32), ("reserved", ctypes.c_int32), ("hard_last", ctypes.c_void_p),
                ("word_flags", ctypes.c_void_p), ("counters", ctypes.c_void_p),
                ("frame_flags", ctypes.c_void_p)]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.fail(f"{LIB} not built: run python -m ldpc_error_floor_amd.build")
    L = ctypes.CDLL(LIB)
    L.ldpc_decode_word.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                   ctypes.c_void_p, ctypes.c_void_p]
    L.ldpc_word_supported.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    return L


def test_symbols_exported(lib):
    for f in ("ldpc_decode_word", "ldpc_word_supported"):
        assert hasattr(lib, f), f


def test_abi_version_unchanged(lib):
    assert lib.ldpc_abi_version() == 3


def test_struct_size():
    assert ctypes.sizeof(WordOutputs) == 40


def test_null_arguments_without_gpu(lib):
    p = Params(T=4, decoding_type=2, q_bit=5, target_bits=8, clip_llr=20.0)
    dummy = ctypes.create_string_buffer(64)
    d = ctypes.addressof(dummy)
    o = WordOutputs(size=ctypes.sizeof(WordOutputs), hard_last=d)
    pp, po = ctypes.addressof(p), ctypes.addressof(o)
    assert lib.ldpc_decode_word(None, None, 1, None, None, None) == -1
    assert lib.ldpc_decode_word(None, d, 1, pp, po, None) == -1          # null context
    assert lib.ldpc_decode_word(d, None, 1, pp, po, None) == -1          # null LLRs
    assert lib.ldpc_decode_word(d, d, 1, None, po, None) == -1
    assert lib.ldpc_decode_word(d, d, 1, pp, None, None) == -1
    assert lib.ldpc_word_supported(None, None) == -1
    assert lib.ldpc_word_supported(None, pp) == -1
    assert lib.ldpc_word_supported(d, None) == -1


def test_bad_size_and_null_hard_last_are_refused_before_the_context_is_read(lib):
    """``size`` other than sizeof(ldpc_word_outputs), or a null ``hard_last`` -> LDPC_ERR_ARG.  The
    context and LLR pointers here are never dereferenced: the outputs are checked first."""
    p = Params(T=4, decoding_type=2, q_bit=5, target_bits=8, clip_llr=20.0)
    dummy = ctypes.create_string_buffer(64)
    d = ctypes.addressof(dummy)
    for size in (0, 8, 32, 48):
        o = WordOutputs(size=size, hard_last=d)
        assert lib.ldpc_decode_word(d, d, 1, ctypes.addressof(p), ctypes.addressof(o), None) == -1
    o = WordOutputs(size=ctypes.sizeof(WordOutputs), hard_last=None, word_flags=d)
    assert lib.ldpc_decode_word(d, d, 1, ctypes.addressof(p), ctypes.addressof(o), None) == -1
