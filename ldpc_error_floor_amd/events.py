"""Floor events (``ldpc_decode_events``): the failing frames of a decode -- every
frame whose decoded word is nonzero -- collected on the GPU with the two weights error-floor work
classifies an event by: ``a``, the wrong bits of the word, and ``b``, its unsatisfied checks (the
(a, b) signature of a trapping set; ``b == 0`` with ``a > 0`` is an undetected error).

``EventBuffer`` owns the device buffers a decode appends to (``NMSDecoder.decode(events=buf)``,
``decode_awgn(early_stop=True, events=buf)``), ``FloorEvents`` is the host table (numpy only), and
``floor_events`` runs a range of one SNR point's Philox stream into such a table.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Iterable, Optional, Tuple

import numpy as np

__all__ = ["EventBuffer", "FloorEvents", "floor_events"]


def _unpack(words, n_bits: int) -> np.ndarray:
    w = np.ascontiguousarray(np.asarray(words).astype(np.uint32))
    b = np.unpackbits(w.view(np.uint8).reshape(w.shape + (4,)), axis=-1, bitorder="little")
    return b.reshape(w.shape[:-1] + (w.shape[-1] * 32,))[..., :n_bits]


@dataclass(eq=False)
class FloorEvents:
    """The events of a run, sorted by frame index.  ``frame`` int64 [n]; ``n_iter``, ``a``,
    ``a_target``, ``b`` int32 [n] (iterations run; ones of the word over all N*z variables, over
    the first target bits, and of its syndrome); ``words`` uint32 [n, ceil(n_vars/32)] (bit v % 32
    of word v // 32) or None when the buffer kept none; ``n_vars`` the word length in bits."""
    frame: np.ndarray
    n_iter: np.ndarray
    a: np.ndarray
    a_target: np.ndarray
    b: np.ndarray
    words: Optional[np.ndarray] = None
    n_vars: int = 0

    def __post_init__(self):
        self.frame = np.asarray(self.frame, np.int64).reshape(-1)
        n = self.frame.size
        for k in ("n_iter", "a", "a_target", "b"):
            v = np.asarray(getattr(self, k), np.int32).reshape(-1)
            if v.size != n:
                raise ValueError(f"{k} has {v.size} entries for {n} frames")
            setattr(self, k, v)
        if self.words is not None:
            w = np.asarray(self.words)
            w = w.view(np.uint32) if w.dtype == np.int32 else w.astype(np.uint32)
            if w.ndim != 2 or w.shape[0] != n:
                raise ValueError(f"words must be [{n}, nw]")
            self.words = w
        self.n_vars = int(self.n_vars)
        order = np.argsort(self.frame, kind="stable")
        if not np.array_equal(order, np.arange(n)):
            self.frame = self.frame[order]
            for k in ("n_iter", "a", "a_target", "b"):
                setattr(self, k, getattr(self, k)[order])
            if self.words is not None:
                self.words = self.words[order]

    def __len__(self) -> int:
        return int(self.frame.size)

    @classmethod
    def empty(cls, n_vars: int = 0, words: bool = True) -> "FloorEvents":
        z = np.zeros(0, np.int32)
        w = np.zeros((0, (int(n_vars) + 31) // 32), np.uint32) if words else None
        return cls(np.zeros(0, np.int64), z, z, z, z, w, n_vars)

    def ab_histogram(self) -> Dict[Tuple[int, int], int]:
        """``{(a, b): number of events}``."""
        out: Dict[Tuple[int, int], int] = {}
        for a, b in zip(self.a.tolist(), self.b.tolist()):
            out[(a, b)] = out.get((a, b), 0) + 1
        return dict(sorted(out.items()))

    def undetected(self) -> np.ndarray:
        """The events that are wrong codewords: ``a > 0`` and ``b == 0`` (bool [n])."""
        return (self.a > 0) & (self.b == 0)

    def bits(self, i: int) -> np.ndarray:
        """The word of event ``i`` unpacked: uint8 [n_vars]."""
        if self.words is None:
            raise ValueError("this table holds no words (EventBuffer(words=False))")
        return _unpack(self.words[i], self.n_vars)

    def save(self, path) -> None:
        d = dict(frame=self.frame, n_iter=self.n_iter, a=self.a, a_target=self.a_target, b=self.b,
                 n_vars=np.int64(self.n_vars))
        if self.words is not None:
            d["words"] = self.words
        with open(path, "wb") as f:                 # (np.savez would append ".npz" to a bare name)
            np.savez_compressed(f, **d)

    @classmethod
    def load(cls, path) -> "FloorEvents":
        with np.load(path) as d:
            return cls(d["frame"], d["n_iter"], d["a"], d["a_target"], d["b"],
                       d["words"] if "words" in d.files else None, int(d["n_vars"]))

    @classmethod
    def concat(cls, tables: Iterable["FloorEvents"]) -> "FloorEvents":
        """The tables joined and sorted by frame.  ``words`` are kept when every table has them."""
        ts = list(tables)
        if not ts:
            return cls.empty()
        nvs = {t.n_vars for t in ts}
        if len(nvs) != 1:
            raise ValueError(f"tables of different word lengths: {sorted(nvs)}")
        words = None
        if all(t.words is not None for t in ts):
            words = np.concatenate([t.words for t in ts], axis=0)
        cat = lambda k: np.concatenate([getattr(t, k) for t in ts])   # noqa: E731
        return cls(cat("frame"), cat("n_iter"), cat("a"), cat("a_target"), cat("b"), words, ts[0].n_vars)

    def __eq__(self, other):
        if not isinstance(other, FloorEvents):
            return NotImplemented
        if (self.words is None) != (other.words is None) or self.n_vars != other.n_vars:
            return False
        return (all(np.array_equal(getattr(self, k), getattr(other, k))
                    for k in ("frame", "n_iter", "a", "a_target", "b")) and
                (self.words is None or np.array_equal(self.words, other.words)))

    def format(self) -> str:
        """The (a, b) table as text: one line per class, undetected errors marked."""
        lines = [f"{len(self)} events, {int(self.undetected().sum())} undetected (b = 0)",
                 f"{'a':>6} {'b':>6} {'events':>8}"]
        for (a, b), n in self.ab_histogram().items():
            lines.append(f"{a:>6} {b:>6} {n:>8}" + ("   undetected" if b == 0 else ""))
        return "\n".join(lines)


class EventBuffer:
    """Device buffers for up to ``cap`` events of ``decoder`` (``words=False``: without the decoded
    words): the count (accumulated by every decode given this buffer; it may exceed ``cap``, the
    records past ``cap`` are then lost), the frame indices, ``{n_iter, a, a_target, b}`` and the
    packed words.  Decodes append asynchronously; ``count`` and ``table`` synchronise."""

    def __init__(self, decoder, cap: int, words: bool = True):
        torch = decoder._torch
        cap = int(cap)
        if cap < 0:
            raise ValueError("cap must be >= 0")
        self.cap = cap
        self.n_vars = int(decoder.n_vars)
        self.nw = (self.n_vars + 31) // 32
        self.device = decoder.device
        dev = decoder.device
        self.ev_count = torch.zeros(1, dtype=torch.int64, device=dev)
        self.ev_frame = torch.zeros(max(cap, 1), dtype=torch.int64, device=dev)
        self.ev_info = torch.zeros((max(cap, 1), 4), dtype=torch.int32, device=dev)
        self.ev_word = torch.zeros((max(cap, 1), self.nw), dtype=torch.int32, device=dev) if words else None

    def count(self) -> int:
        """The events seen since the last ``reset`` (the written ones are the first ``cap``)."""
        return int(self.ev_count.item())

    def reset(self) -> None:
        self.ev_count.zero_()

    def table(self, allow_overflow: bool = False) -> FloorEvents:
        """The collected events on the host, sorted by frame.  Raises ``OverflowError`` when more
        than ``cap`` events were seen, unless ``allow_overflow`` (the table then holds ``cap``)."""
        n = self.count()
        if n > self.cap and not allow_overflow:
            raise OverflowError(f"{n} events for a buffer of {self.cap}: records were lost "
                                "(a larger cap, or table(allow_overflow=True))")
        n = min(n, self.cap)
        info = self.ev_info[:n].cpu().numpy()
        words = None if self.ev_word is None else self.ev_word[:n].cpu().numpy().view(np.uint32)
        return FloorEvents(self.ev_frame[:n].cpu().numpy(), info[:, 0], info[:, 1], info[:, 2], info[:, 3],
                           words, self.n_vars)


def floor_events(decoder, sigma: float, n_codewords: int, batch: int, seed: int, early_stop: bool = True,
                 begin: Optional[int] = None, end: Optional[int] = None, cap: int = 1 << 16, T=None,
                 words: bool = True, kernel=None):
    """The events of codewords ``[begin, end)`` (default all ``n_codewords``) of one SNR point's
    Philox stream (``decode_awgn``'s ``seed`` and global codeword offset, as ``fer_sweep`` walks
    it), decoded ``batch`` at a time: ``(Counters, FloorEvents)``.  Frame indices are global, so
    the tables of any partition of a range concatenate (``FloorEvents.concat``) to the table of
    the whole range.  One synchronisation, at the end.

    ``early_stop=True`` takes each frame's word at its stop iteration with the channel generated
    inside the kernel where the decoder serves that; ``early_stop=False`` the last iteration's,
    composing ``awgn()`` and ``decode()`` (the in-kernel channel has no full-T word build).
    Raises ``OverflowError`` when the range holds more than ``cap`` events."""
    import torch
    from .metrics import Counters
    begin = 0 if begin is None else int(begin)
    end = int(n_codewords) if end is None else int(end)
    if not 0 <= begin <= end <= int(n_codewords):
        raise ValueError("need 0 <= begin <= end <= n_codewords")
    batch = int(batch)
    if batch <= 0:
        raise ValueError("batch must be positive")
    T = decoder.T if T is None else int(T)
    if not decoder.supports_events(T=T, kernel=kernel, early_stop=early_stop):
        raise ValueError("this decoder does not serve events" + (" with early_stop" if early_stop else "") +
                         " (NMSDecoder.supports_events)")
    buf = EventBuffer(decoder, cap, words=words)
    dev = decoder.device
    counters = torch.zeros(4, dtype=torch.int64, device=dev)
    hist = torch.zeros(T, dtype=torch.int64, device=dev) if early_stop else None
    llr = None
    pos = begin
    while pos < end:
        b = min(batch, end - pos)
        if early_stop:
            decoder.decode_awgn(b, float(sigma), int(seed), offset=pos, T=T, counters=counters, kernel=kernel,
                                early_stop=True, iter_hist=hist, events=buf)
        else:
            if llr is None:
                llr = torch.empty((min(batch, end - begin), decoder.n_vars), dtype=torch.float32, device=dev)
            decoder.awgn(b, float(sigma), int(seed), offset=pos, out=llr[:b])
            # (the library's channel is always on the grid: no per-batch check, no synchronisation)
            decoder.decode(llr[:b], T=T, counters=counters, kernel=kernel, events=buf, frame_base=pos,
                           on_off_grid="mark")
        pos += b
    table = buf.table()
    c = Counters.from_array(counters.cpu().numpy(), end - begin, decoder.n_vars)
    if hist is not None:
        c.iter_hist = hist.cpu().numpy().astype(np.int64)
    return c, table
