"""The early-stop entry points of the C ABI (include/ldpc_nms.h: ldpc_decode_es,
ldpc_decode_awgn_es, ldpc_es_supported; CPU only -- no compute calls): exported, arguments
validated before anything touches a GPU, and the ABI version unchanged (the mode adds entry points
and a size-declared struct of its own; no existing struct changes)."""
import ctypes
import os

import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "ldpc_error_floor_amd", "libldpc_nms.so")


class Params(ctypes.Structure):
    _fields_ = [("T", ctypes.c_int32), ("decoding_type", ctypes.c_int32), ("q_bit", ctypes.c_int32),
                ("target_bits", ctypes.c_int32), ("clip_llr", ctypes.c_float), ("kernel", ctypes.c_int32),
                ("outputs_size", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class Channel(ctypes.Structure):
    _fields_ = [("sigma", ctypes.c_double), ("seed", ctypes.c_uint64), ("offset", ctypes.c_int64),
                ("ranges", ctypes.c_int32 * 4), ("reserved", ctypes.c_int32 * 4)]


class EsOutputs(ctypes.Structure):
    _fields_ = [("size", ctypes.c_int32), ("reserved", ctypes.c_int32), ("counters", ctypes.c_void_p),
                ("frame_flags", ctypes.c_void_p), ("n_iter", ctypes.c_void_p), ("iter_hist", ctypes.c_void_p)]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.fail(f"{LIB} not built: run python -m ldpc_error_floor_amd.build")
    L = ctypes.CDLL(LIB)
    L.ldpc_decode_es.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                 ctypes.c_void_p, ctypes.c_void_p]
    L.ldpc_decode_awgn_es.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.c_void_p, ctypes.c_void_p]
    L.ldpc_es_supported.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    return L


def test_symbols_exported(lib):
    for f in ("ldpc_decode_es", "ldpc_decode_awgn_es", "ldpc_es_supported"):
        assert hasattr(lib, f), f


def test_abi_version_unchanged(lib):
    assert lib.ldpc_abi_version() == 3


def test_null_arguments_without_gpu(lib):
    p = Params(T=4, decoding_type=2, q_bit=5, target_bits=8, clip_llr=20.0)
    o = EsOutputs(size=ctypes.sizeof(EsOutputs))
    ch = Channel(sigma=0.5)
    pp, po, pc = ctypes.addressof(p), ctypes.addressof(o), ctypes.addressof(ch)
    assert lib.ldpc_decode_es(None, None, 1, None, None, None) == -1
    assert lib.ldpc_decode_es(None, None, 1, pp, po, None) == -1
    assert lib.ldpc_decode_awgn_es(None, 1, None, None, None, None) == -1
    assert lib.ldpc_decode_awgn_es(None, 1, pp, pc, po, None) == -1
    assert lib.ldpc_es_supported(None, None) == -1
    assert lib.ldpc_es_supported(None, pp) == -1


def test_bad_size_is_refused_before_the_context_is_read(lib):
    """``size`` other than sizeof(ldpc_es_outputs) -> LDPC_ERR_ARG.  The context and LLR pointers
    here are never dereferenced: the outputs' size is checked first."""
    p = Params(T=4, decoding_type=2, q_bit=5, target_bits=8, clip_llr=20.0)
    ch = Channel(sigma=0.5)
    dummy = ctypes.create_string_buffer(64)
    d = ctypes.addressof(dummy)
    for size in (0, 8, ctypes.sizeof(EsOutputs) - 8, ctypes.sizeof(EsOutputs) + 8):
        o = EsOutputs(size=size)
        assert lib.ldpc_decode_es(d, d, 1, ctypes.addressof(p), ctypes.addressof(o), None) == -1
        assert lib.ldpc_decode_awgn_es(d, 1, ctypes.addressof(p), ctypes.addressof(ch),
                                       ctypes.addressof(o), None) == -1
    assert ctypes.sizeof(EsOutputs) == 40
