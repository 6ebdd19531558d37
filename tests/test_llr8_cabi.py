"""The int8-LLR entry points of the C ABI (include/ldpc_nms.h: ldpc_decode_q8, ldpc_decode_q8_word,
ldpc_q8_supported, ldpc_channel_awgn_q8, ldpc_llr_to_q8; CPU only -- no compute
calls): exported, and a NULL input, a wrong struct size or an export pointer the mode does not serve
is LDPC_ERR_ARG before anything reads the context or touches a GPU.  The ABI version is unchanged:
the mode adds entry points and reuses ldpc_decode_outputs / ldpc_word_outputs."""
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


class Outputs(ctypes.Structure):
    _fields_ = [("app_all", ctypes.c_void_p), ("hard_bits", ctypes.c_void_p), ("synd_bits", ctypes.c_void_p),
                ("counters", ctypes.c_void_p), ("frame_flags", ctypes.c_void_p), ("iter_wrong", ctypes.c_void_p)]


class WordOutputs(ctypes.Structure):
    _fields_ = [("size", ctypes.c_int32), ("reserved", ctypes.c_int32), ("hard_last", ctypes.c_void_p),
                ("word_flags", ctypes.c_void_p), ("counters", ctypes.c_void_p),
                ("frame_flags", ctypes.c_void_p)]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.fail(f"{LIB} not built: run python -m ldpc_error_floor_amd.build")
    L = ctypes.CDLL(LIB)
    six = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.ldpc_decode_q8.argtypes = six
    L.ldpc_decode_q8_word.argtypes = six
    L.ldpc_q8_supported.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32]
    L.ldpc_llr_to_q8.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_float, ctypes.c_void_p,
                                 ctypes.c_void_p, ctypes.c_void_p]
    return L


def test_symbols_exported(lib):
    for f in ("ldpc_decode_q8", "ldpc_decode_q8_word", "ldpc_q8_supported", "ldpc_channel_awgn_q8",
              "ldpc_llr_to_q8"):
        assert hasattr(lib, f), f


def test_abi_version_and_struct_sizes_unchanged(lib):
    assert lib.ldpc_abi_version() == 3
    assert ctypes.sizeof(Outputs) == 48 and ctypes.sizeof(WordOutputs) == 40


def test_null_arguments_without_gpu(lib):
    p = Params(T=4, decoding_type=2, q_bit=5, target_bits=8, clip_llr=20.0)
    dummy = ctypes.create_string_buffer(64)
    d = ctypes.addressof(dummy)
    o = Outputs()
    w = WordOutputs(size=ctypes.sizeof(WordOutputs), hard_last=d)
    pp, po, pw = ctypes.addressof(p), ctypes.addressof(o), ctypes.addressof(w)
    assert lib.ldpc_decode_q8(None, None, 1, None, None, None) == ERR_ARG
    assert lib.ldpc_decode_q8(d, None, 1, pp, po, None) == ERR_ARG           # null q8
    assert lib.ldpc_decode_q8(None, d, 1, pp, po, None) == ERR_ARG           # null context
    assert lib.ldpc_decode_q8(d, d, 1, None, po, None) == ERR_ARG            # null params
    assert lib.ldpc_decode_q8_word(None, None, 1, None, None, None) == ERR_ARG
    assert lib.ldpc_decode_q8_word(d, None, 1, pp, pw, None) == ERR_ARG
    assert lib.ldpc_decode_q8_word(None, d, 1, pp, pw, None) == ERR_ARG
    assert lib.ldpc_decode_q8_word(d, d, 1, None, pw, None) == ERR_ARG
    assert lib.ldpc_decode_q8_word(d, d, 1, pp, None, None) == ERR_ARG
    assert lib.ldpc_q8_supported(None, None, 0, 0) == ERR_ARG
    assert lib.ldpc_q8_supported(None, pp, 0, 0) == ERR_ARG
    assert lib.ldpc_q8_supported(d, None, 1, 1) == ERR_ARG
    assert lib.ldpc_llr_to_q8(None, 4, 5, 20.0, d, None, None) == ERR_ARG
    assert lib.ldpc_llr_to_q8(d, 4, 5, 20.0, None, None, None) == ERR_ARG
    assert lib.ldpc_llr_to_q8(d, -1, 5, 20.0, d, None, None) == ERR_ARG


def test_wrong_size_is_refused_before_the_context_is_read(lib):
    """The context and q8 pointers here are 64 zero bytes and are never dereferenced: the sizes
    are checked first."""
    dummy = ctypes.create_string_buffer(64)
    d = ctypes.addressof(dummy)
    o = Outputs()
    for size in (8, 40, 56):
        p = Params(T=4, decoding_type=2, q_bit=5, target_bits=8, clip_llr=20.0, outputs_size=size)
        assert lib.ldpc_decode_q8(d, d, 1, ctypes.addressof(p), ctypes.addressof(o), None) == ERR_ARG
    p = Params(T=4, decoding_type=2, q_bit=5, target_bits=8, clip_llr=20.0)
    for size in (0, 8, 32, 48):
        w = WordOutputs(size=size, hard_last=d)
        assert lib.ldpc_decode_q8_word(d, d, 1, ctypes.addressof(p), ctypes.addressof(w), None) == ERR_ARG
    w = WordOutputs(size=ctypes.sizeof(WordOutputs), hard_last=None, word_flags=d)
    assert lib.ldpc_decode_q8_word(d, d, 1, ctypes.addressof(p), ctypes.addressof(w), None) == ERR_ARG


@pytest.mark.parametrize("export", ["app_all", "hard_bits", "synd_bits"])
@pytest.mark.parametrize("size", [0, 48])
def test_unserved_export_pointer_is_refused_before_the_context_is_read(lib, export, size):
    dummy = ctypes.create_string_buffer(64)
    d = ctypes.addressof(dummy)
    p = Params(T=4, decoding_type=2, q_bit=5, target_bits=8, clip_llr=20.0, outputs_size=size)
    o = Outputs(counters=d, **{export: d})
    assert lib.ldpc_decode_q8(d, d, 1, ctypes.addressof(p), ctypes.addressof(o), None) == ERR_ARG
