"""The event collector on synthetic planes (``ldpc_debug_events_out`` of include/ldpc_nms_debug.h:
csrc/ldpc_events.hip's kernel on caller-supplied plane words and off-grid marks).
No decode here ends on a wrong codeword, and (a, 0) is the class the mode exists to separate, so the
words are built by hand on the wman graph and the records compared with numpy:
  pack 0  frame 3 a nonzero codeword x (GF(2) null space of the lifted H): (a, b) = (|x|, 0);
          frame 9 one flipped bit: (1, the column's degree); the other frames zero;
  pack 1  marked bad, garbage planes: no event, frame flags 0x80;
  pack 2  all 32 frames nonzero (1 to 5 random bits each);
  pack 3  ragged, 6 valid frames: frame 1 holds two bits, the 26 frames past B hold garbage."""
import functools

import numpy as np
import pytest

from _events_ref import events_of_words
from oracle import nms_oracle
from test_gpu_early_stop import _wman
from test_gpu_word import null_vector

pytestmark = pytest.mark.gpu
B, T, TARGET, BASE = 102, 20, 432, 5000


@functools.lru_cache(maxsize=None)
def _setup(device):
    dec, _ = _wman(device)
    nv = dec.n_vars
    rs = np.random.RandomState(8)
    bits = np.zeros((128, nv), np.uint8)
    x = null_vector(dec.graph.proto, dec.z, (0, 0))
    bits[3] = x
    bits[9, 100] = 1
    bits[32:64] = rs.randint(0, 2, (32, nv))
    for f in range(64, 96):
        bits[f, rs.choice(nv, rs.randint(1, 6), replace=False)] = 1
    bits[97, [0, nv - 1]] = 1
    bits[102:] = rs.randint(0, 2, (26, nv))
    bad = np.array([0, 1, 0, 0], np.uint32)
    planes = (bits.reshape(4, 32, nv).astype(np.uint32) << np.arange(32, dtype=np.uint32)[None, :, None]).sum(
        axis=1, dtype=np.uint32)
    n_iter = rs.randint(1, T + 1, B).astype(np.uint8)
    valid = bits[:B].copy()
    valid[32:64] = 0                                     # the bad pack is not an event
    synd = nms_oracle.syndromes(valid, nms_oracle.lifted_edges(dec.graph.proto, dec.z))
    return dec, x, planes, bad, n_iter, valid, synd


def _run(dec, planes, bad, n, n_iter, cap=64, words=True):
    import torch
    dev = dec.device
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    nw = (dec.n_vars + 31) // 32
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    frame = torch.full((cap,), -77, dtype=torch.int64, device=dev)
    info = torch.full((cap, 4), -78, dtype=torch.int32, device=dev)
    word = torch.full((cap, nw), 0x5A5A5A5A, dtype=torch.int32, device=dev) if words else None
    flags = torch.full((n,), 0x55, dtype=torch.uint8, device=dev)
    p, b = t(planes.view(np.int32)), t(bad.view(np.int32))
    ni = None if n_iter is None else t(n_iter)
    ctx = dec._ensure_ctx(1, T)
    dec._ext.debug_events_out(ctx, p.data_ptr(), b.data_ptr(), n, TARGET, 0 if ni is None else ni.data_ptr(), T,
                              BASE, cap, count.data_ptr(), frame.data_ptr(), info.data_ptr(),
                              0 if word is None else word.data_ptr(), flags.data_ptr(),
                              torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    k = int(count.item())
    order = np.argsort(frame[:k].cpu().numpy())
    return {"count": k, "frame": frame[:k].cpu().numpy()[order], "info": info[:k].cpu().numpy()[order],
            "words": None if word is None else word[:k].cpu().numpy().view(np.uint32)[order],
            "flags": flags.cpu().numpy(), "rest": (frame[k:], info[k:], None if word is None else word[k:])}


@pytest.mark.parametrize("with_n_iter", [True, False])
def test_synthetic_planes(cuda_device, with_n_iter):
    dec, x, planes, bad, n_iter, valid, synd = _setup(cuda_device)
    ev = events_of_words(valid, synd, n_iter if with_n_iter else np.full(B, T), TARGET, BASE)
    by = dict(zip((ev["frame"] - BASE).tolist(), zip(ev["a"].tolist(), ev["b"].tolist())))
    # the numpy side holds what the case is there for
    deg = int((dec.graph.proto[:, 100 // dec.z] >= 0).sum())
    assert by[3] == (int(x.sum()), 0) and x.sum() > 0                        # a wrong codeword: (a, 0)
    assert by[9] == (1, deg) and deg >= 2
    assert set(by) == {3, 9, 97} | set(range(64, 96)) and by[97][0] == 2     # no bad pack, no frame past B
    got = _run(dec, planes, bad, B, n_iter if with_n_iter else None)
    assert got["count"] == len(by)
    assert got["frame"].tolist() == ev["frame"].tolist()
    for i, k in enumerate(("n_iter", "a", "a_target", "b")):
        assert np.array_equal(got["info"][:, i], ev[k]), k
    assert np.array_equal(got["words"], ev["words"])
    assert (ev["a_target"] < ev["a"]).any()
    assert (got["flags"][32:64] == 0x80).all() and (got["flags"][np.r_[0:32, 64:B]] == 0x55).all()
    fr, info, word = got["rest"]
    assert (fr == -77).all() and (info == -78).all() and (word == 0x5A5A5A5A).all()


def test_only_invalid_frames_set_is_no_event(cuda_device):
    """A ragged pack whose only set bits belong to frames past B: nothing is counted or written."""
    dec, x, planes, bad, n_iter, valid, synd = _setup(cuda_device)
    p = planes[3:4] & np.uint32(0xFFFFFFC0)               # frames 6 .. 31 of the ragged pack alone
    assert p.any()
    got = _run(dec, p, np.zeros(1, np.uint32), 6, None, cap=4)
    assert got["count"] == 0 and (got["flags"] == 0x55).all()
    fr, info, word = got["rest"]
    assert (fr == -77).all() and (info == -78).all() and (word == 0x5A5A5A5A).all()


def test_full_pack_overflowing_the_buffer(cuda_device):
    """The 32-event pack into 5 slots, without words: 35 counted, 5 distinct records written whole."""
    dec, x, planes, bad, n_iter, valid, synd = _setup(cuda_device)
    ev = events_of_words(valid, synd, n_iter, TARGET, BASE)
    got = _run(dec, planes, bad, B, n_iter, cap=5, words=False)
    assert got["count"] == 35 and got["words"] is None
    assert got["frame"].size == 5 and len(set(got["frame"].tolist())) == 5
    for i, f in enumerate(got["frame"].tolist()):
        j = ev["frame"].tolist().index(f)
        assert got["info"][i].tolist() == [ev[k][j] for k in ("n_iter", "a", "a_target", "b")]
