"""The events entry points of the C ABI (include/ldpc_nms.h: ldpc_decode_events,
ldpc_decode_awgn_events, ldpc_events_supported; the test hook ldpc_debug_events_out of
ldpc_nms_debug.h; CPU only -- no compute calls): exported, the outputs struct
checked before anything else is read, and the ABI version and the sizes of the existing
size-declared structs unchanged."""
import ctypes
import os

import pytest

from conftest import ROOT
from test_es_word_cabi import Channel, EsWordOutputs, Params

LIB = os.path.join(ROOT, "ldpc_error_floor_amd", "libldpc_nms.so")
ERR_ARG = -1


class EventOutputs(ctypes.Structure):
    _fields_ = [("size", ctypes.c_int32), ("early_stop", ctypes.c_int32), ("frame_base", ctypes.c_int64),
                ("cap", ctypes.c_int64), ("ev_count", ctypes.c_void_p), ("ev_frame", ctypes.c_void_p),
                ("ev_info", ctypes.c_void_p), ("ev_word", ctypes.c_void_p), ("counters", ctypes.c_void_p),
                ("frame_flags", ctypes.c_void_p), ("n_iter", ctypes.c_void_p), ("iter_hist", ctypes.c_void_p),
                ("reserved1", ctypes.c_uint64)]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.fail(f"{LIB} not built: run python -m ldpc_error_floor_amd.build")
    L = ctypes.CDLL(LIB)
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    L.ldpc_decode_events.argtypes = [vp, vp, i64, vp, vp, vp]
    L.ldpc_decode_awgn_events.argtypes = [vp, i64, vp, vp, vp, vp]
    L.ldpc_events_supported.argtypes = [vp, vp, i32]
    L.ldpc_debug_events_out.argtypes = [vp, vp, vp, i64, i32, vp, i32, vp, vp]
    return L


def test_symbols_exported(lib):
    for f in ("ldpc_decode_events", "ldpc_decode_awgn_events", "ldpc_events_supported", "ldpc_debug_events_out"):
        assert hasattr(lib, f), f


def test_abi_version_and_struct_sizes(lib):
    assert lib.ldpc_abi_version() == 3
    assert ctypes.sizeof(EventOutputs) == 96
    assert ctypes.sizeof(EsWordOutputs) == 64


def _args():
    p = Params(T=4, decoding_type=2, q_bit=5, target_bits=8, clip_llr=20.0)
    ch = Channel(sigma=0.5, seed=1)
    dummy = ctypes.create_string_buffer(128)
    return p, ch, dummy, ctypes.addressof(dummy)


def _good(d, **kw):
    f = dict(size=ctypes.sizeof(EventOutputs), early_stop=1, cap=4, ev_count=d, ev_frame=d, ev_info=d)
    f.update(kw)
    return EventOutputs(**f)


def test_null_arguments_without_gpu(lib):
    p, ch, dummy, d = _args()
    o = _good(d)
    pp, po, pc = ctypes.addressof(p), ctypes.addressof(o), ctypes.addressof(ch)
    assert lib.ldpc_decode_events(None, None, 1, None, None, None) == ERR_ARG
    assert lib.ldpc_decode_events(None, d, 1, pp, po, None) == ERR_ARG         # null context
    assert lib.ldpc_decode_events(d, None, 1, pp, po, None) == ERR_ARG         # null LLRs
    assert lib.ldpc_decode_events(d, d, 1, None, po, None) == ERR_ARG
    assert lib.ldpc_decode_events(d, d, 1, pp, None, None) == ERR_ARG
    assert lib.ldpc_decode_awgn_events(None, 1, pp, pc, po, None) == ERR_ARG
    assert lib.ldpc_decode_awgn_events(d, 1, None, pc, po, None) == ERR_ARG
    assert lib.ldpc_decode_awgn_events(d, 1, pp, None, po, None) == ERR_ARG
    assert lib.ldpc_decode_awgn_events(d, 1, pp, pc, None, None) == ERR_ARG
    assert lib.ldpc_events_supported(None, None, 1) == ERR_ARG
    assert lib.ldpc_events_supported(None, pp, 0) == ERR_ARG
    assert lib.ldpc_events_supported(d, None, 1) == ERR_ARG
    assert lib.ldpc_debug_events_out(None, d, d, 32, 8, None, 4, po, None) == ERR_ARG
    assert lib.ldpc_debug_events_out(d, d, d, 32, 8, None, 4, None, None) == ERR_ARG


def test_bad_outputs_are_refused_before_the_context_is_read(lib):
    """``size`` other than sizeof(ldpc_event_outputs) (88 would be the struct without its padding
    word), a null ``ev_count`` / ``ev_frame`` / ``ev_info`` or a negative ``cap`` -> LDPC_ERR_ARG.  The
    context and LLR pointers here are never dereferenced: the outputs are checked first."""
    p, ch, dummy, d = _args()
    pp, pc = ctypes.addressof(p), ctypes.addressof(ch)
    bad = [_good(d, size=s) for s in (0, 8, 64, 88, 104)]
    bad += [_good(d, **{k: None}) for k in ("ev_count", "ev_frame", "ev_info")]
    bad += [_good(d, cap=-1), _good(d, cap=-(1 << 40))]
    for early_stop in (0, 1):
        for o in bad:
            o.early_stop = early_stop
            po = ctypes.addressof(o)
            assert lib.ldpc_decode_events(d, d, 1, pp, po, None) == ERR_ARG
            assert lib.ldpc_decode_awgn_events(d, 1, pp, pc, po, None) == ERR_ARG
            assert lib.ldpc_debug_events_out(d, d, d, 32, 8, None, 4, po, None) == ERR_ARG
    assert not any(dummy.raw)
