"""The int8-LLR entry points of the early-stop, stop-iteration-word and events modes in the C ABI
(include/ldpc_nms.h: ldpc_decode_q8_es, ldpc_decode_q8_es_word, ldpc_decode_q8_events,
ldpc_q8_es_supported; CPU only -- no compute calls): exported, and a NULL input, a
wrong struct size or a missing required pointer is LDPC_ERR_ARG before anything reads the context or
touches a GPU.  The ABI version is unchanged: the modes add entry points and reuse ldpc_es_outputs,
ldpc_es_word_outputs and ldpc_event_outputs."""
import ctypes
import os

import pytest

from conftest import ROOT
from test_es_cabi import EsOutputs
from test_es_word_cabi import EsWordOutputs, Params
from test_events_cabi import EventOutputs
from test_llr8_cabi import Outputs, WordOutputs

LIB = os.path.join(ROOT, "ldpc_error_floor_amd", "libldpc_nms.so")
ERR_ARG = -1
DECODES = ("ldpc_decode_q8_es", "ldpc_decode_q8_es_word", "ldpc_decode_q8_events")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.fail(f"{LIB} not built: run python -m ldpc_error_floor_amd.build")
    L = ctypes.CDLL(LIB)
    vp = ctypes.c_void_p
    for f in DECODES:
        getattr(L, f).argtypes = [vp, vp, ctypes.c_int64, vp, vp, vp]
    L.ldpc_q8_es_supported.argtypes = [vp, vp, ctypes.c_int32]
    return L


def _args():
    p = Params(T=4, decoding_type=2, q_bit=5, target_bits=8, clip_llr=20.0)
    dummy = ctypes.create_string_buffer(128)
    return p, dummy, ctypes.addressof(dummy)


def _good(d):
    """A valid outputs struct of each decode, every required pointer set."""
    return {"ldpc_decode_q8_es": EsOutputs(size=ctypes.sizeof(EsOutputs), counters=d),
            "ldpc_decode_q8_es_word": EsWordOutputs(size=ctypes.sizeof(EsWordOutputs), hard_stop=d),
            "ldpc_decode_q8_events": EventOutputs(size=ctypes.sizeof(EventOutputs), early_stop=1, cap=4, ev_count=d,
                                                  ev_frame=d, ev_info=d)}


def test_symbols_exported(lib):
    for f in DECODES + ("ldpc_q8_es_supported",):
        assert hasattr(lib, f), f


def test_abi_version_and_struct_sizes_unchanged(lib):
    assert lib.ldpc_abi_version() == 3
    assert ctypes.sizeof(EsOutputs) == 40 and ctypes.sizeof(EsWordOutputs) == 64 and ctypes.sizeof(EventOutputs) == 96
    assert ctypes.sizeof(Outputs) == 48 and ctypes.sizeof(WordOutputs) == 40 and ctypes.sizeof(Params) == 32


def test_null_arguments_without_gpu(lib):
    p, dummy, d = _args()
    pp = ctypes.addressof(p)
    for f, o in _good(d).items():
        fn, po = getattr(lib, f), ctypes.addressof(o)
        assert fn(None, None, 1, None, None, None) == ERR_ARG, f
        assert fn(d, None, 1, pp, po, None) == ERR_ARG, f            # null q8
        assert fn(None, d, 1, pp, po, None) == ERR_ARG, f            # null context
        assert fn(d, d, 1, None, po, None) == ERR_ARG, f             # null params
        assert fn(d, d, 1, pp, None, None) == ERR_ARG, f             # null outputs
    assert lib.ldpc_q8_es_supported(None, None, 0) == ERR_ARG
    assert lib.ldpc_q8_es_supported(None, pp, 0) == ERR_ARG
    assert lib.ldpc_q8_es_supported(d, None, 1) == ERR_ARG
    assert not any(dummy.raw)


def test_wrong_size_or_missing_pointer_is_refused_before_the_context_is_read(lib):
    """The context and q8 pointers here are 128 zero bytes and are never dereferenced: the outputs
    are checked first (with an all-zero context a read of it would dereference its null graph)."""
    p, dummy, d = _args()
    pp = ctypes.addressof(p)
    bad = []
    for size in (0, 8, 32, 48, 64):
        bad.append(("ldpc_decode_q8_es", EsOutputs(size=size, counters=d)))
    for size in (0, 8, 40, 56, 72):
        bad.append(("ldpc_decode_q8_es_word", EsWordOutputs(size=size, hard_stop=d)))
    bad.append(("ldpc_decode_q8_es_word", EsWordOutputs(size=ctypes.sizeof(EsWordOutputs), hard_stop=None, word_flags=d)))
    ev = dict(size=ctypes.sizeof(EventOutputs), cap=4, ev_count=d, ev_frame=d, ev_info=d)
    for early_stop in (0, 1):
        for size in (0, 8, 64, 88, 104):
            bad.append(("ldpc_decode_q8_events", EventOutputs(**{**ev, "size": size, "early_stop": early_stop})))
        for k in ("ev_count", "ev_frame", "ev_info"):
            bad.append(("ldpc_decode_q8_events", EventOutputs(**{**ev, k: None, "early_stop": early_stop})))
        for cap in (-1, -(1 << 40)):
            bad.append(("ldpc_decode_q8_events", EventOutputs(**{**ev, "cap": cap, "early_stop": early_stop})))
    for f, o in bad:
        assert getattr(lib, f)(d, d, 1, pp, ctypes.addressof(o), None) == ERR_ARG, (f, o.size)
    assert not any(dummy.raw)
