"""``NMSDecoder``: the HIP decoder over torch device tensors.

This is the build's replacement for the T-iteration graph that ``build_neural_network``
unrolls (``Main_Functions.py:157-385``) and ``compute_results`` runs through ``sess.run``
(``Print_Functions.py:147-151``).  Inputs are LLRs ``[B, N*z]`` (or ``[B, N, z]``, the
``xa`` placeholder shape) in the reference's log(p1/p0) convention; outputs are
``ya_output_all`` (``[T*B, Nt*z]`` float32), per-iteration hard bits / syndromes, and
on-device FER/BER counters.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _native
from .code import TannerGraph
from .config import DECODING_MS, DECODING_MS_NONUDGE, DECODING_QMS, DECODING_SP, VALID_Q_BITS
from .weights import DecoderWeights

__all__ = ["NMSDecoder", "Decoder", "DecodeResult", "KERNELS"]

KERNELS = {"auto": 0, "flood": 1, "fused": 2}
# the q8 format's grids: q_bit -> (step, qmax); a byte is LLR / step
Q8_GRIDS = {5: (0.5, 15), -5: (1.0, 15), 4: (1.0, 7), 3: (2.0, 3)}


@dataclass
class DecodeResult:
    app: Optional["object"] = None          # torch f32 [T, B, Nt*z]
    hard: Optional["object"] = None         # torch int32 [T, B, ceil(N*z/32)] (bit words)
    synd: Optional["object"] = None         # torch int32 [T, B, ceil(M*z/32)]
    counters: Optional["object"] = None     # torch int64 [4]
    flags: Optional["object"] = None        # torch uint8 [B]
    iter_wrong: Optional["object"] = None   # torch int32 [T, ceil(B/32)]: bit b%32 of word
                                            # (t, b//32) = frame b wrong at iteration t
    n_iter: Optional["object"] = None       # early stop: torch uint8 [B], iterations run (0: the
                                            # frame's pack held an off-grid LLR and was not decoded)
    iter_hist: Optional["object"] = None    # early stop: torch int64 [T], frames with n_iter == t+1
    hard_last: Optional["object"] = None    # word mode: torch int32 [B, ceil(N*z/32)], the last
                                            # iteration's hard decisions (``unpack_bits`` unpacks them);
                                            # with early_stop, each frame's at its stop iteration
    word_flags: Optional["object"] = None   # word mode: torch uint8 [B], bit 0 = syndrome nonzero,
                                            # 0x80 = the frame's pack held an off-grid LLR (not decoded)

    def frame_errors(self, B: int) -> np.ndarray:
        """``iter_wrong`` unpacked on the host: bool [T, B] (calc_ber_fer's per-iteration frame
        error, ``Print_Functions.py:100-118``)."""
        return unpack_bits(self.iter_wrong.cpu().numpy(), B).astype(bool)

    def ya_output_all(self):
        """``ya_output_all`` layout: iterations stacked on axis 0 -> [T*B, Nt*z]."""
        T, B, n = self.app.shape
        return self.app.reshape(T * B, n)


def unpack_bits(words, n_bits: int) -> np.ndarray:
    """[..., W] uint32 words (bit k of word w = bit 32w+k) -> [..., n_bits] uint8."""
    w = np.ascontiguousarray(np.asarray(words).astype(np.uint32))
    b = np.unpackbits(w.view(np.uint8).reshape(w.shape + (4,)), axis=-1, bitorder="little")
    return b.reshape(w.shape[:-1] + (w.shape[-1] * 32,))[..., :n_bits]


class NMSDecoder:
    def __init__(self, proto, z: int, weights: DecoderWeights, decoding_type: int = DECODING_QMS,
                 q_bit: int = 5, target_node: int = 0, clip_LLR: float = 20.0, device=None,
                 kernel: str = "auto", B_max: int = 0):
        import torch
        self._torch = torch
        if decoding_type not in (DECODING_SP, DECODING_MS, DECODING_QMS, DECODING_MS_NONUDGE):
            raise ValueError(f"decoding_type {decoding_type} not supported")
        if decoding_type == DECODING_QMS and q_bit not in VALID_Q_BITS:
            raise ValueError(f"q_bit {q_bit} not in {VALID_Q_BITS}")
        if kernel not in KERNELS:
            raise ValueError(f"kernel must be one of {list(KERNELS)}")
        self.graph = TannerGraph(np.asarray(proto), int(z))
        self.z = int(z)
        self.N, self.M = self.graph.N, self.graph.M
        self.n_vars = self.N * self.z
        self.n_checks = self.M * self.z
        self.target_node = int(target_node) if target_node and target_node > 0 else self.N
        self.target_bits = self.target_node * self.z
        self.decoding_type = int(decoding_type)
        self.q_bit = int(q_bit)
        self.clip = float(clip_LLR)
        self.kernel = kernel
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("NMSDecoder runs on a ROCm GPU device only (no CPU fallback)")
        self._ext = _native.load()
        self._g = self._ext.Graph(self.graph.proto.astype(np.int32), self.z,
                                  self.device.index or 0)
        self.set_weights(weights)
        self._ctx = None
        self._ctx_B = 0
        self._ctx_T = 0
        if B_max:
            self._ensure_ctx(B_max, self.T)

    # ------------------------------------------------------------------------------
    def set_weights(self, weights: DecoderWeights):
        W = weights
        if W.alpha.shape[1] != self.graph.E or W.beta.shape[1] != self.N:
            raise ValueError("weight tables do not match the graph")
        self.weights = W
        self.T = W.T
        self._g.set_weights(np.ascontiguousarray(W.alpha, np.float32),
                            None if W.alpha_ucn is None else np.ascontiguousarray(W.alpha_ucn, np.float32),
                            np.ascontiguousarray(W.beta, np.float32))

    def _ensure_ctx(self, B: int, T: int):
        if self._ctx is None or B > self._ctx_B or T > self._ctx_T:
            Bm = max(B, self._ctx_B)
            Tm = max(T, self._ctx_T, self.T)
            self._ctx = None
            self._ctx = self._ext.Ctx(self._g, int(Bm), int(Tm))
            self._ctx_B, self._ctx_T = Bm, Tm
        return self._ctx

    def kernel_info(self, T=None, kernel=None):
        T = self.T if T is None else T
        ctx = self._ensure_ctx(1, T)
        return self._ext.kernel_info(ctx, T, self.decoding_type, self.q_bit, self.target_bits,
                                     KERNELS[kernel or self.kernel], self.clip)

    def supports(self, kernel: str, T=None) -> bool:
        try:
            self.kernel_info(T, kernel)
            return True
        except RuntimeError:
            return False

    def _as_llr(self, llr):
        torch = self._torch
        if not isinstance(llr, torch.Tensor):
            llr = torch.from_numpy(np.ascontiguousarray(np.asarray(llr, np.float32)))
        llr = llr.to(device=self.device, dtype=torch.float32)
        B = llr.shape[0]
        if B == 0:
            return llr.reshape(0, self.n_vars)
        llr = llr.reshape(B, -1).contiguous()
        if llr.shape[1] != self.n_vars:
            raise ValueError(f"llr has {llr.shape[1]} bits per codeword, graph has {self.n_vars}")
        return llr

    def supports_early_stop(self, T=None, kernel=None) -> bool:
        """Whether ``decode(..., early_stop=True)`` is served for this decoder
        (``ldpc_es_supported``): a QMS grid with q in {5, -5, 4, 3}, no per-edge check weights, kernel
        auto or fused, and a graph that an early-stop instance of the bit-sliced kernel fits (wman,
        802.11n) or, with channel weights that are all 1, the compressed kernel's early-stop build
        (5G BG1 n2112)."""
        T = self.T if T is None else int(T)
        if T > self.T:
            return False
        ctx = self._ensure_ctx(1, T)
        return bool(self._ext.es_supported(ctx, T, self.decoding_type, self.q_bit, self.target_bits,
                                           KERNELS[kernel or self.kernel], self.clip))

    def supports_hard_last(self, T=None, kernel=None, early_stop: bool = False) -> bool:
        """Whether ``decode(..., hard_last=True)`` is served for this decoder
        (``ldpc_word_supported``): what the bit-sliced kernels decode -- a QMS grid with q in
        {5, -5, 4, 3}, no per-edge check weights, kernel auto or fused, and a graph the bit-sliced
        kernel or the compressed one fits.  ``early_stop=True``: whether
        ``decode(..., early_stop=True, hard_last=True)`` is (``ldpc_es_word_supported``): exactly
        where ``supports_early_stop`` holds."""
        T = self.T if T is None else int(T)
        if T > self.T:
            return False
        ctx = self._ensure_ctx(1, T)
        if early_stop:
            return bool(self._ext.es_word_supported(ctx, T, self.decoding_type, self.q_bit, self.target_bits,
                                                    KERNELS[kernel or self.kernel], self.clip))
        return bool(self._ext.word_supported(ctx, T, self.decoding_type, self.q_bit, self.target_bits,
                                             KERNELS[kernel or self.kernel], self.clip))

    def supports_events(self, T=None, kernel=None, early_stop: bool = False) -> bool:
        """Whether ``decode(..., events=buf)`` (``early_stop=True``: with ``early_stop=True``, and
        ``decode_awgn(..., early_stop=True, events=buf)``) is served for this decoder
        (``ldpc_events_supported``): exactly where ``supports_hard_last`` with the same
        ``early_stop`` holds."""
        T = self.T if T is None else int(T)
        if T > self.T:
            return False
        ctx = self._ensure_ctx(1, T)
        return bool(self._ext.events_supported(ctx, T, self.decoding_type, self.q_bit, self.target_bits,
                                               KERNELS[kernel or self.kernel], self.clip, bool(early_stop)))

    def _decode_events(self, llr, B, T, nt, events, frame_base, early_stop, counters, flags, n_iter, iter_hist,
                       kernel, stream, on_off_grid, channel=None):
        """``decode(events=...)`` and, with ``channel`` (sigma, seed, offset, punct, short) instead of
        ``llr``, ``decode_awgn``'s: the batch's events appended to the ``EventBuffer`` beside the
        outputs of the early-stop decode, or of the word mode without ``early_stop``."""
        torch = self._torch
        if on_off_grid not in ("raise", "mark"):
            raise ValueError("on_off_grid must be 'raise' or 'mark'")
        if events.device != self.device or events.n_vars != self.n_vars:
            raise ValueError("events must be an EventBuffer of this decoder")
        res = DecodeResult()
        # (the generated channel is always on the grid)
        check = on_off_grid == "raise" and channel is None
        asked = flags is not None and flags is not False
        self._es_outputs(res, B, T, counters, flags if asked else check, n_iter if early_stop else False,
                         iter_hist if early_stop else None)
        if B == 0:
            return res
        ctx = self._ensure_ctx(B, T)
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        ptr = lambda t: 0 if t is None else t.data_ptr()   # noqa: E731
        outs = (bool(early_stop),) + (() if channel is not None else (int(frame_base),)) + (
            events.cap, events.ev_count.data_ptr(), events.ev_frame.data_ptr(), events.ev_info.data_ptr(),
            ptr(events.ev_word), ptr(res.counters), ptr(res.flags), ptr(res.n_iter), ptr(res.iter_hist),
            stream.cuda_stream)
        if channel is not None:
            sigma, seed, offset, punct, short = channel
            self._ext.decode_awgn_events(ctx, B, T, self.decoding_type, self.q_bit, nt, self.clip,
                                         KERNELS[kernel or self.kernel], float(sigma), int(seed), int(offset),
                                         int(punct[0]), int(punct[1]), int(short[0]), int(short[1]), *outs)
            return res
        self._ext.decode_events(ctx, llr.data_ptr(), B, T, self.decoding_type, self.q_bit, nt, self.clip,
                                KERNELS[kernel or self.kernel], *outs)
        if check:
            stream.synchronize()
            nbad = int((res.flags[:B] == 0x80).sum().item())
            if nbad:
                raise ValueError(f"events: {nbad} frames are in packs with LLRs off the quantizer "
                                 "grid and were not decoded (on_off_grid='mark' returns them marked)")
            if not asked:
                res.flags = None
        return res

    def _decode_word(self, llr, T, nt, hard_last, word_flags, counters, flags, kernel, stream, on_off_grid):
        """``decode(hard_last=...)``: the decoded words of the last iteration."""
        torch = self._torch
        dev = self.device
        if on_off_grid not in ("raise", "mark"):
            raise ValueError("on_off_grid must be 'raise' or 'mark'")
        llr = self._as_llr(llr)
        B = int(llr.shape[0])
        res = self._word_result(B, hard_last)
        want_wf = word_flags or on_off_grid == "raise"
        if want_wf:
            res.word_flags = torch.empty(B, dtype=torch.uint8, device=dev)
        self._es_outputs(res, B, T, counters, flags, False, None)
        if B == 0:
            return res
        ctx = self._ensure_ctx(B, T)
        if stream is None:
            stream = torch.cuda.current_stream(dev)
        ptr = lambda t: 0 if t is None else t.data_ptr()   # noqa: E731
        self._ext.decode_word(ctx, llr.data_ptr(), B, T, self.decoding_type, self.q_bit, nt, self.clip,
                              KERNELS[kernel or self.kernel], res.hard_last.data_ptr(), ptr(res.word_flags),
                              ptr(res.counters), ptr(res.flags), stream.cuda_stream)
        if on_off_grid == "raise":
            self._raise_off_grid(res, stream, "hard_last", word_flags)
        return res

    def _word_result(self, B, hard_last):
        """A result with the word modes' rows: ``hard_last`` itself when it is a caller-owned
        contiguous int32 [>= B, ceil(n_vars / 32)] tensor (checked), else B new rows."""
        torch = self._torch
        dev = self.device
        nw = (self.n_vars + 31) // 32
        res = DecodeResult()
        if isinstance(hard_last, torch.Tensor):
            if (hard_last.dtype != torch.int32 or hard_last.device != dev or hard_last.dim() != 2 or
                    hard_last.shape[0] < B or hard_last.shape[1] != nw or not hard_last.is_contiguous()):
                raise ValueError(f"hard_last must be a contiguous int32 [>= B, {nw}] tensor on the decoder's device")
            res.hard_last = hard_last
        else:
            res.hard_last = torch.empty((B, nw), dtype=torch.int32, device=dev)
        return res

    @staticmethod
    def _raise_off_grid(res, stream, what, keep_word_flags):
        """``on_off_grid="raise"`` of the word modes: wait for the decode, raise when
        ``res.word_flags`` marks frames of a pack off the grid, and drop the flags if unasked."""
        stream.synchronize()
        nbad = int((res.word_flags == 0x80).sum().item())
        if nbad:
            raise ValueError(f"{what}: {nbad} frames are in packs with LLRs off the quantizer "
                             "grid and were not decoded (on_off_grid='mark' returns them marked)")
        if not keep_word_flags:
            res.word_flags = None

    def _decode_es_word(self, llr, B, T, nt, hard_last, word_flags, counters, flags, n_iter, iter_hist,
                        kernel, stream, on_off_grid, channel=None):
        """``decode(early_stop=True, hard_last=...)`` and, with ``channel`` (sigma, seed, offset,
        punct, short) instead of ``llr``, ``decode_awgn``'s: each frame's decoded word at its stop
        iteration beside the early-stop outputs."""
        torch = self._torch
        dev = self.device
        if on_off_grid not in ("raise", "mark"):
            raise ValueError("on_off_grid must be 'raise' or 'mark'")
        res = self._word_result(B, hard_last)
        # (the generated channel is always on the grid)
        want_wf = word_flags or (on_off_grid == "raise" and channel is None)
        if want_wf:
            res.word_flags = torch.empty(B, dtype=torch.uint8, device=dev)
        self._es_outputs(res, B, T, counters, flags, n_iter, iter_hist)
        if B == 0:
            return res
        ctx = self._ensure_ctx(B, T)
        if stream is None:
            stream = torch.cuda.current_stream(dev)
        ptr = lambda t: 0 if t is None else t.data_ptr()   # noqa: E731
        outs = (res.hard_last.data_ptr(), ptr(res.word_flags), ptr(res.counters), ptr(res.flags),
                ptr(res.n_iter), ptr(res.iter_hist), stream.cuda_stream)
        if channel is not None:
            sigma, seed, offset, punct, short = channel
            self._ext.decode_awgn_es_word(ctx, B, T, self.decoding_type, self.q_bit, nt, self.clip,
                                          KERNELS[kernel or self.kernel], float(sigma), int(seed), int(offset),
                                          int(punct[0]), int(punct[1]), int(short[0]), int(short[1]), *outs)
            return res
        self._ext.decode_es_word(ctx, llr.data_ptr(), B, T, self.decoding_type, self.q_bit, nt, self.clip,
                                 KERNELS[kernel or self.kernel], *outs)
        if on_off_grid == "raise":
            self._raise_off_grid(res, stream, "early_stop", word_flags)
        return res

    def _es_outputs(self, res, B, T, counters, flags, n_iter, iter_hist):
        """The output tensors of an early-stop or word decode into ``res`` (caller-owned ones
        checked; the word mode has no ``n_iter`` / ``iter_hist``)."""
        torch = self._torch
        dev = self.device
        if counters is True:
            counters = torch.zeros(4, dtype=torch.int64, device=dev)
        if counters is not None:
            if counters.dtype != torch.int64 or counters.numel() < 4 or counters.device != dev:
                raise ValueError("counters must be an int64[4] tensor on the decoder's device")
            res.counters = counters
        if isinstance(flags, torch.Tensor):
            if flags.dtype != torch.uint8 or flags.device != dev or flags.numel() < B:
                raise ValueError("flags tensor must be uint8 on the decoder's device, >= B long")
            res.flags = flags
        elif flags:
            res.flags = torch.empty(B, dtype=torch.uint8, device=dev)
        if n_iter:
            res.n_iter = torch.empty(B, dtype=torch.uint8, device=dev)
        if iter_hist is True:
            iter_hist = torch.zeros(T, dtype=torch.int64, device=dev)
        if iter_hist is not None and iter_hist is not False:
            if (not isinstance(iter_hist, torch.Tensor) or iter_hist.dtype != torch.int64 or
                    iter_hist.numel() < T or iter_hist.device != dev or not iter_hist.is_contiguous()):
                raise ValueError("iter_hist must be a contiguous int64[T] tensor on the decoder's device")
            res.iter_hist = iter_hist
        return res

    @staticmethod
    def _es_check_exports(**exports):
        bad = [k for k, v in exports.items() if v]
        if bad:
            raise ValueError("early_stop serves counters, flags, n_iter and iter_hist only, not " +
                             ", ".join(bad))

    def decode(self, llr, T: Optional[int] = None, app: Optional[bool] = None, hard: bool = False,
               synd: bool = False, counters=None, flags: bool = False, kernel: Optional[str] = None,
               stream=None, target_bits: Optional[int] = None, iter_wrong: bool = False,
               early_stop: bool = False, n_iter: bool = False, iter_hist=None,
               on_off_grid: str = "raise", hard_last=False, word_flags: bool = False,
               events=None, frame_base: int = 0) -> DecodeResult:
        """Decode a batch.  ``counters`` may be a caller-owned int64[4] device tensor that is
        accumulated into (``+=``); pass ``True`` to get a fresh one.  ``target_bits``
        overrides the output / FER bit range (default Nt*z).  ``iter_wrong``: the per-iteration
        frame-error words (every kernel, the counters-only ones included).  ``app`` defaults to
        True, and to False with ``early_stop``.

        ``early_stop`` (opt-in, no counterpart in the reference): each frame stops at
        the first iteration whose hard decisions have a zero syndrome and its outputs are frozen
        there.  ``counters[0..2]`` and ``flags`` then describe the frames at their own stop
        iteration (``counters[3]`` is left untouched), ``n_iter=True`` returns the iterations run
        per frame (uint8 [B]) and ``iter_hist`` (``True`` or a caller-owned int64[T] tensor that is
        accumulated into) their histogram.  ``app`` / ``hard`` / ``synd`` / ``iter_wrong`` are not
        served and raise ``ValueError``.  The LLRs must lie on the quantizer grid: a pack of 32
        frames holding an off-grid value is not decoded (``n_iter`` 0, ``flags`` 0x80, not
        counted); ``on_off_grid="raise"`` synchronises and raises ``ValueError`` when there is one,
        ``"mark"`` returns the result as it is.

        ``hard_last`` (``True``, or a caller-owned contiguous int32 tensor with at least B rows of
        ceil(N*z/32) words): the decoded words -- the last iteration's hard decisions
        over all N*z variables, packed as ``hard[T-1]`` is -- from the bit-sliced kernels' own
        launch, with ``counters`` / ``flags`` as a plain decode gives them and, with
        ``word_flags=True``, a uint8 [B] whose bit 0 says the word's syndrome is nonzero.  ``app``
        defaults to False; ``app`` / ``hard`` / ``synd`` / ``iter_wrong`` are not served with it and
        raise ``ValueError``.  The LLRs must lie on the quantizer grid, as for ``early_stop``: a
        pack of 32 frames holding an off-grid value is not decoded (zero rows, ``word_flags`` and
        ``flags`` 0x80, not counted); ``on_off_grid`` as above.

        ``early_stop=True`` with ``hard_last``: ``res.hard_last`` then holds each
        frame's word at the iteration it stopped at, ``hd_stop`` -- what a practical decoder
        returns -- not the last iteration's: frozen at the frame's first zero-syndrome iteration,
        iteration T - 1's for a frame that never stops.  ``word_flags`` bit 0 is then 0 for every
        frame with ``n_iter < T``; ``counters`` / ``flags`` / ``n_iter`` / ``iter_hist`` are those of
        ``early_stop=True`` alone.

        ``events`` (an ``events.EventBuffer`` of this decoder): instead of a row per
        frame, the batch's events -- the frames whose decoded word (the last iteration's, or with
        ``early_stop=True`` the stop iteration's) is nonzero anywhere -- are found on the device and
        appended to the buffer: frame index ``frame_base + b``, iterations run, ``a`` (wrong bits),
        ``a_target`` (those among the target bits) and ``b`` (unsatisfied checks), and the word.
        ``counters`` / ``flags`` (and ``n_iter`` / ``iter_hist`` with ``early_stop``) are those of
        the mode without ``events``; ``hard_last`` / ``app`` / ``hard`` / ``synd`` / ``iter_wrong``
        are not served with it and raise ``ValueError``.  Off-grid packs as above: no event."""
        torch = self._torch
        T = self.T if T is None else int(T)
        nt = self.target_bits if target_bits is None else int(target_bits)
        if T > self.T:
            raise ValueError(f"T={T} exceeds the {self.T} iterations the weights cover")
        if events is not None:
            bad = [k for k, v in dict(hard_last=hard_last is not False and hard_last is not None, app=app, hard=hard,
                                      synd=synd, iter_wrong=iter_wrong, word_flags=word_flags).items() if v]
            if not early_stop:
                bad += [k for k, v in dict(n_iter=n_iter, iter_hist=iter_hist is not None and iter_hist is not False).items() if v]
            if bad:
                raise ValueError("events serves counters and flags (with early_stop: n_iter and iter_hist) only, "
                                 "not " + ", ".join(bad))
            llr = self._as_llr(llr)
            return self._decode_events(llr, int(llr.shape[0]), T, nt, events, frame_base, early_stop, counters,
                                       flags, n_iter, iter_hist, kernel, stream, on_off_grid)
        if hard_last is not False and hard_last is not None and early_stop:
            self._es_check_exports(app=app, hard=hard, synd=synd, iter_wrong=iter_wrong)
            llr = self._as_llr(llr)
            return self._decode_es_word(llr, int(llr.shape[0]), T, nt, hard_last, word_flags, counters, flags,
                                        n_iter, iter_hist, kernel, stream, on_off_grid)
        if hard_last is not False and hard_last is not None:
            bad = [k for k, v in dict(app=app, hard=hard, synd=synd, iter_wrong=iter_wrong,
                                      n_iter=n_iter, iter_hist=iter_hist is not None and iter_hist is not False).items() if v]
            if bad:
                raise ValueError("hard_last serves word_flags, counters and flags only, not " + ", ".join(bad))
            return self._decode_word(llr, T, nt, hard_last, word_flags, counters, flags, kernel, stream, on_off_grid)
        if word_flags:
            raise ValueError("word_flags is an output of hard_last=True")
        if early_stop:
            self._es_check_exports(app=app, hard=hard, synd=synd, iter_wrong=iter_wrong)
            if on_off_grid not in ("raise", "mark"):
                raise ValueError("on_off_grid must be 'raise' or 'mark'")
            llr = self._as_llr(llr)
            B = int(llr.shape[0])
            res = DecodeResult()
            if B == 0:
                return self._es_outputs(res, 0, T, counters, flags, n_iter, iter_hist)
            ctx = self._ensure_ctx(B, T)
            want_n = n_iter or on_off_grid == "raise"
            self._es_outputs(res, B, T, counters, flags, want_n, iter_hist)
            if stream is None:
                stream = torch.cuda.current_stream(self.device)
            ptr = lambda t: 0 if t is None else t.data_ptr()   # noqa: E731
            self._ext.decode_es(ctx, llr.data_ptr(), B, T, self.decoding_type, self.q_bit, nt, self.clip,
                                KERNELS[kernel or self.kernel], ptr(res.counters), ptr(res.flags),
                                ptr(res.n_iter), ptr(res.iter_hist), stream.cuda_stream)
            if on_off_grid == "raise":
                stream.synchronize()
                nbad = int((res.n_iter == 0).sum().item())
                if nbad:
                    raise ValueError(f"early_stop: {nbad} frames are in packs with LLRs off the quantizer "
                                     "grid and were not decoded (on_off_grid='mark' returns them marked)")
                if not n_iter:
                    res.n_iter = None
            return res
        if n_iter or (iter_hist is not None and iter_hist is not False):
            raise ValueError("n_iter and iter_hist are outputs of early_stop=True")
        app = True if app is None else app
        llr = self._as_llr(llr)
        B = int(llr.shape[0])
        if B == 0:
            return self._empty_result(T, nt, hard, synd, counters, flags, app, iter_wrong)
        ctx = self._ensure_ctx(B, T)
        res = DecodeResult()
        dev = self.device
        if app:
            res.app = torch.empty((T, B, nt), dtype=torch.float32, device=dev)
        if hard:
            res.hard = torch.empty((T, B, (self.n_vars + 31) // 32), dtype=torch.int32, device=dev)
        if synd:
            res.synd = torch.empty((T, B, (self.n_checks + 31) // 32), dtype=torch.int32, device=dev)
        if counters is True:
            counters = torch.zeros(4, dtype=torch.int64, device=dev)
        if counters is not None:
            if counters.dtype != torch.int64 or counters.numel() < 4 or counters.device != dev:
                raise ValueError("counters must be an int64[4] tensor on the decoder's device")
            res.counters = counters
        if isinstance(flags, torch.Tensor):                 # caller-owned uint8 [>= B]
            if flags.dtype != torch.uint8 or flags.device != dev or flags.numel() < B:
                raise ValueError("flags tensor must be uint8 on the decoder's device, >= B long")
            res.flags = flags
        elif flags:
            res.flags = torch.empty(B, dtype=torch.uint8, device=dev)
        if iter_wrong:
            res.iter_wrong = torch.empty((T, (B + 31) // 32), dtype=torch.int32, device=dev)
        if stream is None:
            stream = torch.cuda.current_stream(dev)
        ptr = lambda t: 0 if t is None else t.data_ptr()   # noqa: E731
        self._ext.decode(ctx, llr.data_ptr(), B, T, self.decoding_type, self.q_bit,
                         nt, self.clip, KERNELS[kernel or self.kernel],
                         ptr(res.app), ptr(res.hard), ptr(res.synd), ptr(res.counters),
                         ptr(res.flags), stream.cuda_stream, ptr(res.iter_wrong))
        return res

    # ---- int8 quantized LLRs ----------------------------------------------------
    def _q8_grid(self):
        """(step, qmax) of the bytes this decoder takes: its quantizer grid (``Q8_GRIDS``).  The
        float modes and q = 6 have no such grid and no int8 kernel; for them, which only
        ``decode_q8``'s dequantizing fallback serves, a byte is the LLR itself (step 1, |g| <= 126)."""
        if self.decoding_type == DECODING_QMS and self.q_bit in Q8_GRIDS:
            return Q8_GRIDS[self.q_bit]
        return (1.0, 126)

    def supports_q8(self, has_short: bool = False, word: bool = False, T=None, kernel=None,
                    early_stop: bool = False) -> bool:
        """Whether ``decode_q8`` runs the bit-sliced kernels' int8 builds for this decoder
        (``ldpc_q8_supported``) -- exactly where they serve the float decode of the same kind
        (counters / flags / iter_wrong, or with ``word`` the ``hard_last`` mode) -- and, with
        ``has_short``, decodes the +-clip markers of shortened bits.  Where it is false (q = 6, the
        float modes, flood, per-edge weights, other graphs) ``decode_q8`` dequantizes and calls
        ``decode``.  ``early_stop=True``: whether ``decode_q8(early_stop=True)``, with or without
        ``hard_last`` or ``events``, runs the int8 builds of the early-stop kernels
        (``ldpc_q8_es_supported``); ``events`` without ``early_stop`` is the
        ``word`` case."""
        T = self.T if T is None else int(T)
        if T > self.T or self.decoding_type != DECODING_QMS or self.q_bit not in Q8_GRIDS:
            return False
        ctx = self._ensure_ctx(1, T)
        if early_stop:
            return bool(self._ext.q8_es_supported(ctx, T, self.decoding_type, self.q_bit, self.target_bits,
                                                  KERNELS[kernel or self.kernel], self.clip, bool(has_short)))
        return bool(self._ext.q8_supported(ctx, T, self.decoding_type, self.q_bit, self.target_bits,
                                           KERNELS[kernel or self.kernel], self.clip, bool(has_short), bool(word)))

    def quantize_q8(self, llr, strict: bool = True):
        """Float LLRs -> the q8 bytes (int8, same shape): ``rint(llr / step)`` where the value is on
        the grid and within +-qmax, -128 / +127 for -clip / +clip.  Any other value has no byte:
        ``strict=True`` raises ``ValueError``, ``strict=False`` stores it saturated to +-qmax.  A
        tensor on the decoder's device is converted there (``ldpc_llr_to_q8``), anything else on
        the host."""
        torch = self._torch
        step, qmax = self._q8_grid()
        native = self.decoding_type == DECODING_QMS and self.q_bit in Q8_GRIDS
        if native and isinstance(llr, torch.Tensor) and llr.device.type == "cuda":
            x = llr.to(dtype=torch.float32).contiguous()
            out = torch.empty(x.shape, dtype=torch.int8, device=x.device)
            bad = torch.zeros(1, dtype=torch.int64, device=x.device)
            if x.numel():
                with torch.cuda.device(x.device):
                    self._ext.llr_to_q8(x.data_ptr(), x.numel(), self.q_bit, self.clip, out.data_ptr(), bad.data_ptr(),
                                        torch.cuda.current_stream(x.device).cuda_stream)
            nbad = int(bad.item()) if strict else 0
        else:
            x = np.asarray(llr.cpu().numpy() if isinstance(llr, torch.Tensor) else llr, dtype=np.float32)
            g = x * np.float32(1.0 / step)
            q = np.clip(np.rint(np.nan_to_num(g, nan=0.0)), -qmax, qmax)
            lo, hi = x == np.float32(-self.clip), x == np.float32(self.clip)
            ok = q == g
            q = np.where(~ok & lo, -128, np.where(~ok & hi, 127, q)).astype(np.int8)
            nbad = int((~(ok | lo | hi)).sum())
            out = torch.from_numpy(q)
        if strict and nbad:
            raise ValueError(f"quantize_q8: {nbad} values are neither on the q_bit={self.q_bit} grid "
                             f"(multiples of {step} within +-{qmax * step}) nor +-clip_LLR")
        return out

    def dequantize_q8(self, q8):
        """The float LLRs q8 bytes stand for (float32, same shape, on the input's device):
        ``g * step``, -128 / +127 -> -clip / +clip.  (An invalid byte maps to ``g * step``, off the
        range of the grid.)"""
        torch = self._torch
        step, _ = self._q8_grid()
        q = q8 if isinstance(q8, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(q8, np.int8)))
        if q.dtype != torch.int8:
            raise ValueError("q8 must be int8")
        x = q.to(torch.float32) * step
        x = torch.where(q == -128, torch.full_like(x, -self.clip), x)
        return torch.where(q == 127, torch.full_like(x, self.clip), x)

    def _as_q8(self, q8):
        torch = self._torch
        if not isinstance(q8, torch.Tensor):
            a = np.asarray(q8)
            if a.dtype != np.int8:
                raise ValueError("q8 must be int8")
            q8 = torch.from_numpy(np.ascontiguousarray(a))
        if q8.dtype != torch.int8:
            raise ValueError("q8 must be int8 (decode() takes LLRs of any other dtype)")
        q8 = q8.to(device=self.device)
        B = q8.shape[0]
        q8 = q8.reshape(B, -1) if B else q8.reshape(0, self.n_vars)
        if q8.shape[1] != self.n_vars:
            raise ValueError(f"q8 has {q8.shape[1]} bits per codeword, graph has {self.n_vars}")
        # (rows of n_vars bytes back to back; any start address: the kernels load single bytes)
        return q8 if q8.is_contiguous() else q8.contiguous()

    def _q8_invalid_rows(self, q8):
        """bool [B]: the rows of a q8 tensor that hold an invalid byte (markers taken as valid)."""
        _, qmax = self._q8_grid()
        ok = ((q8 >= -qmax) & (q8 <= qmax)) | (q8 == -128) | (q8 == 127)
        return ~ok.all(dim=1)

    def decode_q8(self, q8, T: Optional[int] = None, counters=None, flags=False, iter_wrong: bool = False,
                  hard_last=False, word_flags: bool = False, kernel: Optional[str] = None, stream=None,
                  on_invalid: str = "raise", app: bool = False, hard: bool = False, synd: bool = False,
                  target_bits: Optional[int] = None, early_stop: bool = False, n_iter: bool = False,
                  iter_hist=None, events=None, frame_base: int = 0) -> DecodeResult:
        """Decode int8 quantized LLRs: ``q8`` is int8 ``[B, N*z]``, the LLR in grid
        units ``g = LLR / step`` with ``-qmax <= g <= qmax``, -128 / +127 for a shortened bit's
        -clip / +clip (``quantize_q8`` makes it, ``awgn_q8`` generates it).  Every output equals,
        bit for bit, ``decode`` of ``dequantize_q8(q8)``: ``counters``, ``flags``, ``iter_wrong``,
        and with ``hard_last`` (``True`` or a caller-owned tensor) the decoded words and
        ``word_flags``.  The bit-sliced kernels read the bytes directly (a quarter of the float
        input), with no fixup launch.

        Any other byte is invalid, and so is a marker where ``supports_q8(has_short=True)`` is
        false.  A pack of 32 frames holding one is not decoded: ``flags`` (and ``word_flags``) 0x80,
        zero rows, nothing in the counters or ``iter_wrong``.  ``on_invalid="raise"`` synchronises
        and raises ``ValueError`` naming the first such frame; ``"mark"`` returns the result as it
        is.

        ``early_stop`` / ``n_iter`` / ``iter_hist`` / ``events`` / ``frame_base``
        mean what they mean in ``decode``, with ``hard_last`` the stop-iteration words, and are
        refused as there: ``iter_wrong`` (and ``app`` / ``hard`` / ``synd``) not with
        ``early_stop``, ``n_iter`` / ``iter_hist`` only with it, ``events`` without ``hard_last`` /
        ``word_flags``.  The int8 builds of the early-stop kernels decode them (``events`` without
        ``early_stop``: the int8 word build), each output bit for bit ``decode``'s of
        ``dequantize_q8(q8)`` in the same mode.  A marked pack has ``n_iter`` 0 and no event, and
        enters neither the counters nor ``iter_hist``.

        Where ``supports_q8`` is false, or ``app`` / ``hard`` / ``synd`` is asked for, the bytes are
        dequantized and ``decode`` runs with the same mode arguments (``last_kernel()`` tells);
        invalid bytes are then checked on the device for ``"raise"`` and decoded as ``decode``
        decodes off-grid LLRs for ``"mark"``."""
        torch = self._torch
        if on_invalid not in ("raise", "mark"):
            raise ValueError("on_invalid must be 'raise' or 'mark'")
        T = self.T if T is None else int(T)
        nt = self.target_bits if target_bits is None else int(target_bits)
        if T > self.T:
            raise ValueError(f"T={T} exceeds the {self.T} iterations the weights cover")
        word = hard_last is not False and hard_last is not None
        if word_flags and not word:
            raise ValueError("word_flags is an output of hard_last=True")
        if word and iter_wrong:
            raise ValueError("hard_last serves word_flags, counters and flags only, not iter_wrong")
        want_hist = iter_hist is not None and iter_hist is not False
        if events is not None:
            bad = [k for k, v in dict(hard_last=word, app=app, hard=hard, synd=synd, iter_wrong=iter_wrong,
                                      word_flags=word_flags).items() if v]
            if not early_stop:
                bad += [k for k, v in dict(n_iter=n_iter, iter_hist=want_hist).items() if v]
            if bad:
                raise ValueError("events serves counters and flags (with early_stop: n_iter and iter_hist) only, "
                                 "not " + ", ".join(bad))
        elif early_stop:
            self._es_check_exports(app=app, hard=hard, synd=synd, iter_wrong=iter_wrong)
        elif n_iter or want_hist:
            raise ValueError("n_iter and iter_hist are outputs of early_stop=True")
        q8 = self._as_q8(q8)
        B = int(q8.shape[0])
        mode = early_stop or events is not None
        # (the mode arguments reach decode only where one is asked for: the plain call is unchanged)
        mode_kw = dict(early_stop=early_stop, n_iter=n_iter, iter_hist=iter_hist, events=events,
                       frame_base=frame_base) if mode else {}
        if early_stop:
            served = self.supports_q8(T=T, kernel=kernel, early_stop=True)
        else:
            served = self.supports_q8(word=word or events is not None, T=T, kernel=kernel)
        if app or hard or synd or not served:
            if on_invalid == "raise" and B:
                badrows = self._q8_invalid_rows(q8)
                if bool(badrows.any().item()):
                    first = int(badrows.nonzero()[0].item())
                    raise ValueError(f"decode_q8: frame {first} holds a byte that is no q8 value "
                                     "(on_invalid='mark' decodes it as an off-grid LLR)")
            return self.decode(self.dequantize_q8(q8), T=T, app=bool(app), hard=hard, synd=synd, counters=counters,
                               flags=flags, kernel=kernel, stream=stream, target_bits=target_bits,
                               iter_wrong=iter_wrong, hard_last=hard_last, word_flags=word_flags,
                               on_off_grid="mark", **mode_kw)
        if mode:
            return self._decode_q8_mode(q8, B, T, nt, early_stop, hard_last if word else None, word_flags, events,
                                        frame_base, counters, flags, n_iter, iter_hist, kernel, stream,
                                        on_invalid == "raise")
        dev = self.device
        res = self._word_result(B, hard_last) if word else DecodeResult()
        asked = flags is not None and flags is not False
        check = on_invalid == "raise"
        self._es_outputs(res, B, T, counters, flags if asked else check, False, None)
        if word and word_flags:
            res.word_flags = torch.empty(B, dtype=torch.uint8, device=dev)
        if iter_wrong:
            res.iter_wrong = torch.empty((T, (B + 31) // 32), dtype=torch.int32, device=dev)
        if B == 0:
            return res
        ctx = self._ensure_ctx(B, T)
        if stream is None:
            stream = torch.cuda.current_stream(dev)
        ptr = lambda t: 0 if t is None else t.data_ptr()   # noqa: E731
        if word:
            self._ext.decode_q8_word(ctx, q8.data_ptr(), B, T, self.decoding_type, self.q_bit, nt, self.clip,
                                     KERNELS[kernel or self.kernel], res.hard_last.data_ptr(), ptr(res.word_flags),
                                     ptr(res.counters), ptr(res.flags), stream.cuda_stream)
        else:
            self._ext.decode_q8(ctx, q8.data_ptr(), B, T, self.decoding_type, self.q_bit, nt, self.clip,
                                KERNELS[kernel or self.kernel], ptr(res.counters), ptr(res.flags),
                                ptr(res.iter_wrong), stream.cuda_stream)
        if check:
            stream.synchronize()
            marked = (res.flags[:B] == 0x80).nonzero()
            if marked.numel():
                raise ValueError(f"decode_q8: frame {int(marked[0].item())} is the first of {int(marked.numel())} "
                                 "frames in packs holding a byte that is no q8 value; they were not decoded "
                                 "(on_invalid='mark' returns them marked)")
            if not asked:
                res.flags = None
        return res

    def _decode_q8_mode(self, q8, B, T, nt, early_stop, hard_last, word_flags, events, frame_base, counters,
                        flags, n_iter, iter_hist, kernel, stream, check):
        """``decode_q8``'s early-stop, stop-iteration-word and events decodes on the int8 builds
        (DESIGN.md 3.12): the outputs of ``decode`` in the same mode; ``check``: wait and raise on a
        marked pack (``frame_flags`` 0x80)."""
        torch = self._torch
        dev = self.device
        if events is not None and (events.device != dev or events.n_vars != self.n_vars):
            raise ValueError("events must be an EventBuffer of this decoder")
        res = self._word_result(B, hard_last) if hard_last is not None else DecodeResult()
        asked = flags is not None and flags is not False
        self._es_outputs(res, B, T, counters, flags if asked else check, n_iter if early_stop else False,
                         iter_hist if early_stop else None)
        if hard_last is not None and word_flags:
            res.word_flags = torch.empty(B, dtype=torch.uint8, device=dev)
        if B == 0:
            return res
        ctx = self._ensure_ctx(B, T)
        if stream is None:
            stream = torch.cuda.current_stream(dev)
        ptr = lambda t: 0 if t is None else t.data_ptr()   # noqa: E731
        head = (ctx, q8.data_ptr(), B, T, self.decoding_type, self.q_bit, nt, self.clip, KERNELS[kernel or self.kernel])
        tail = (ptr(res.counters), ptr(res.flags), ptr(res.n_iter), ptr(res.iter_hist), stream.cuda_stream)
        if events is not None:
            self._ext.decode_q8_events(*head, bool(early_stop), int(frame_base), events.cap, events.ev_count.data_ptr(),
                                       events.ev_frame.data_ptr(), events.ev_info.data_ptr(), ptr(events.ev_word),
                                       *tail)
        elif hard_last is not None:
            self._ext.decode_q8_es_word(*head, res.hard_last.data_ptr(), ptr(res.word_flags), *tail)
        else:
            self._ext.decode_q8_es(*head, *tail)
        if check:
            stream.synchronize()
            marked = (res.flags[:B] == 0x80).nonzero()
            if marked.numel():
                raise ValueError(f"decode_q8: frame {int(marked[0].item())} is the first of {int(marked.numel())} "
                                 "frames in packs holding a byte that is no q8 value; they were not decoded "
                                 "(on_invalid='mark' returns them marked)")
            if not asked:
                res.flags = None
        return res

    def awgn_q8(self, B: int, sigma: float, seed: int, offset: int = 0, punct=None, short=None,
                out=None, stream=None):
        """``awgn`` as q8 bytes (int8 [B, N*z]; ``ldpc_channel_awgn_q8``): the same Philox stream
        and level sampler, so it equals ``quantize_q8(awgn(...))``; punctured bits 0, shortened
        bits -128."""
        torch = self._torch
        if self.decoding_type != DECODING_QMS or self.q_bit not in Q8_GRIDS:
            raise ValueError("awgn_q8 covers the QMS grids q_bit 5, -5, 4 and 3 only")
        punct = getattr(self, "punct", (0, 0)) if punct is None else punct
        short = getattr(self, "short", (0, 0)) if short is None else short
        if out is None:
            out = torch.empty((B, self.n_vars), dtype=torch.int8, device=self.device)
        elif (out.dtype != torch.int8 or out.device != self.device or not out.is_contiguous() or
              out.numel() < B * self.n_vars):
            raise ValueError("out must be a contiguous int8 [B, N*z] tensor on the decoder's device")
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        self._ext.channel_awgn_q8(out.data_ptr(), int(B), self.n_vars, float(sigma), int(seed), int(offset),
                                  self.q_bit, int(punct[0]), int(punct[1]), int(short[0]), int(short[1]),
                                  stream.cuda_stream)
        return out

    def generates_channel_in_kernel(self, T=None, kernel=None, app: bool = False) -> bool:
        """Whether a counters-only ``decode_awgn`` (``app``: one with an APP export) generates
        the LLRs inside the decoding kernel (the prologue of the fused v5 kernel, and of the
        bit-sliced kernels for QMS counters-only decodes); otherwise ``ldpc_decode_awgn`` runs
        the channel kernel into HBM and then the decoder (flood, ffl).  The C ABI's own decision
        (``ldpc_awgn_in_kernel``), with this decoder's shortened range."""
        T = self.T if T is None else T
        ctx = self._ensure_ctx(1, T)
        short = getattr(self, "short", (0, 0)) or (0, 0)
        return bool(self._ext.awgn_in_kernel(ctx, T, self.decoding_type, self.q_bit, self.target_bits,
                                             KERNELS[kernel or self.kernel], self.clip,
                                             has_short=short[0] > 0, app=app))

    def last_kernel(self) -> str:
        """The kernel that served this decoder's last decode (``ldpc_ctx_last_kernel``)."""
        return "" if self._ctx is None else self._ext.last_kernel(self._ctx)

    def last_frozen(self) -> bool:
        """Whether this decoder's last decode ran a geometry-frozen build of the bit-sliced kernel
        (``ldpc_ctx_last_frozen``; ``LDPC_BS_FROZEN=0`` forces the generic build)."""
        return False if self._ctx is None else bool(self._ext.last_frozen(self._ctx))

    def last_afix(self) -> bool:
        """Whether this decoder's last decode weighed the check minima of its bit-sliced kernel
        through the fixed-set immediate tables (``ldpc_ctx_last_afix``; ``LDPC_BS_AFIX=0`` forces
        the tables in LDS)."""
        return False if self._ctx is None else bool(self._ext.last_afix(self._ctx))

    def last_wf(self) -> bool:
        """Whether this decoder's last decode ran a bit-sliced build with the weights frozen in
        kind (``ldpc_ctx_last_wf``; ``LDPC_BS_WF=0`` forces the other builds)."""
        return False if self._ctx is None else bool(self._ext.last_wf(self._ctx))

    def _empty_result(self, T, nt, hard, synd, counters, flags, app, iter_wrong=False):
        """An empty batch decodes to empty outputs; a caller's counters are left unchanged."""
        torch = self._torch
        dev = self.device
        res = DecodeResult()
        if app:
            res.app = torch.empty((T, 0, nt), dtype=torch.float32, device=dev)
        if hard:
            res.hard = torch.empty((T, 0, (self.n_vars + 31) // 32), dtype=torch.int32, device=dev)
        if synd:
            res.synd = torch.empty((T, 0, (self.n_checks + 31) // 32), dtype=torch.int32, device=dev)
        if counters is True:
            counters = torch.zeros(4, dtype=torch.int64, device=dev)
        res.counters = counters if counters is not None else None
        if isinstance(flags, torch.Tensor):
            res.flags = flags[:0]
        elif flags:
            res.flags = torch.empty(0, dtype=torch.uint8, device=dev)
        if iter_wrong:
            res.iter_wrong = torch.empty((T, 0), dtype=torch.int32, device=dev)
        return res

    def decode_awgn(self, B: int, sigma: float, seed: int, offset: int = 0, punct=None, short=None,
                    T: Optional[int] = None, app: bool = False, counters=None, flags=None,
                    kernel: Optional[str] = None, stream=None, iter_wrong: bool = False,
                    early_stop: bool = False, n_iter: bool = False, iter_hist=None,
                    hard_last=False, word_flags: bool = False, events=None) -> DecodeResult:
        """Decode B codewords whose LLRs come from the on-GPU AWGN channel, generated inside
        the decoder (``ldpc_decode_awgn``): identical to ``decode(awgn(...))`` without the
        LLRs ever being written to HBM.  ``counters`` / ``flags`` as in ``decode``;
        ``early_stop`` / ``n_iter`` / ``iter_hist`` as in ``decode`` (the generated channel is
        always on the grid).  ``hard_last`` / ``word_flags`` are served with ``early_stop=True``
        (each frame's word at its stop iteration, as ``decode(early_stop=True, hard_last=...)``;
        DESIGN.md 3.9).  Without ``early_stop``, ``hard_last`` is not served here (the kernels'
        in-prologue channel has no export build) and raises ``ValueError``: compose ``awgn()`` and
        ``decode()``.  ``events`` (an ``EventBuffer``) likewise needs
        ``early_stop=True``: the batch's events are appended with the frame index ``offset + b``,
        the codeword's global index in the channel's stream."""
        want_word = hard_last is not False and hard_last is not None
        if events is not None:
            if not early_stop:
                raise ValueError("decode_awgn does not serve events without early_stop: use "
                                 "decode(awgn(...), events=buf, frame_base=offset)")
            bad = [k for k, v in dict(hard_last=want_word, app=app, iter_wrong=iter_wrong, word_flags=word_flags).items() if v]
            if bad:
                raise ValueError("events serves counters and flags (with early_stop: n_iter and iter_hist) only, "
                                 "not " + ", ".join(bad))
            T = self.T if T is None else int(T)
            if T > self.T:
                raise ValueError(f"T={T} exceeds the {self.T} iterations the weights cover")
            punct = getattr(self, "punct", (0, 0)) if punct is None else punct
            short = getattr(self, "short", (0, 0)) if short is None else short
            return self._decode_events(None, int(B), T, self.target_bits, events, 0, True, counters, flags, n_iter,
                                       iter_hist, kernel, stream, "mark",
                                       channel=(sigma, seed, offset, punct, short))
        if want_word and not early_stop:
            raise ValueError("decode_awgn does not serve hard_last: use decode(awgn(...), hard_last=True)")
        if word_flags and not want_word:
            raise ValueError("word_flags is an output of hard_last=True")
        torch = self._torch
        T = self.T if T is None else int(T)
        punct = getattr(self, "punct", (0, 0)) if punct is None else punct
        short = getattr(self, "short", (0, 0)) if short is None else short
        if early_stop:
            self._es_check_exports(app=app, iter_wrong=iter_wrong)
            if T > self.T:
                raise ValueError(f"T={T} exceeds the {self.T} iterations the weights cover")
            B = int(B)
            if want_word:
                return self._decode_es_word(None, B, T, self.target_bits, hard_last, word_flags, counters, flags,
                                            n_iter, iter_hist, kernel, stream, "mark",
                                            channel=(sigma, seed, offset, punct, short))
            res = DecodeResult()
            if B == 0:
                return self._es_outputs(res, 0, T, counters, flags, n_iter, iter_hist)
            ctx = self._ensure_ctx(B, T)
            self._es_outputs(res, B, T, counters, flags, n_iter, iter_hist)
            if stream is None:
                stream = torch.cuda.current_stream(self.device)
            ptr = lambda t: 0 if t is None else t.data_ptr()   # noqa: E731
            self._ext.decode_awgn_es(ctx, B, T, self.decoding_type, self.q_bit, self.target_bits,
                                     self.clip, KERNELS[kernel or self.kernel], float(sigma), int(seed),
                                     int(offset), int(punct[0]), int(punct[1]), int(short[0]),
                                     int(short[1]), ptr(res.counters), ptr(res.flags), ptr(res.n_iter),
                                     ptr(res.iter_hist), stream.cuda_stream)
            return res
        if n_iter or (iter_hist is not None and iter_hist is not False):
            raise ValueError("n_iter and iter_hist are outputs of early_stop=True")
        if int(B) == 0:
            return self._empty_result(T, self.target_bits, False, False, counters, flags, app, iter_wrong)
        ctx = self._ensure_ctx(int(B), T)
        dev = self.device
        res = DecodeResult()
        if app:
            res.app = torch.empty((T, B, self.target_bits), dtype=torch.float32, device=dev)
        if counters is True:
            counters = torch.zeros(4, dtype=torch.int64, device=dev)
        if counters is not None:
            if counters.dtype != torch.int64 or counters.numel() < 4 or counters.device != dev:
                raise ValueError("counters must be an int64[4] tensor on the decoder's device")
            res.counters = counters
        if isinstance(flags, torch.Tensor):
            if flags.dtype != torch.uint8 or flags.device != dev or flags.numel() < B:
                raise ValueError("flags tensor must be uint8 on the decoder's device, >= B long")
            res.flags = flags
        elif flags:
            res.flags = torch.empty(B, dtype=torch.uint8, device=dev)
        if iter_wrong:
            res.iter_wrong = torch.empty((T, (int(B) + 31) // 32), dtype=torch.int32, device=dev)
        if stream is None:
            stream = torch.cuda.current_stream(dev)
        ptr = lambda t: 0 if t is None else t.data_ptr()   # noqa: E731
        self._ext.decode_awgn(ctx, int(B), T, self.decoding_type, self.q_bit, self.target_bits,
                              self.clip, KERNELS[kernel or self.kernel], float(sigma), int(seed),
                              int(offset), int(punct[0]), int(punct[1]), int(short[0]),
                              int(short[1]), ptr(res.app), ptr(res.counters), ptr(res.flags),
                              stream.cuda_stream, ptr(res.iter_wrong))
        return res

    def _uncorrected_index(self, flags, stream):
        """Batch indices (sorted, on the device) of the frames wrong at every iteration."""
        torch = self._torch
        B = int(flags.shape[0])
        idx = torch.empty(max(B, 1), dtype=torch.int64, device=self.device)
        cnt = torch.empty(1, dtype=torch.int64, device=self.device)
        self._ext.collect_frames(flags.data_ptr(), B, 1, 1, idx.data_ptr(), B, cnt.data_ptr(),
                                 stream.cuda_stream)
        stream.synchronize()
        n = int(cnt.item())
        return torch.sort(idx[:n]).values.contiguous()     # batch order, as the reference writes

    def collect_uncorrected(self, flags, llr, stream=None):
        """LLR rows (host float32 [n, N*z], batch order) of the frames wrong at every iteration
        (``frame_flags`` bit 0 = the reference's ``uncor_flag``), compacted on the GPU by
        ``ldpc_collect_frames`` + ``ldpc_gather_rows``; only the n rows cross PCIe."""
        torch = self._torch
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        sel = self._uncorrected_index(flags, stream)
        n = int(sel.numel())
        if n == 0:
            return np.zeros((0, self.n_vars), np.float32)
        llr = llr.reshape(llr.shape[0], -1)
        rows = torch.empty((n, self.n_vars), dtype=torch.float32, device=self.device)
        for s0 in range(0, n, 65535):
            s1 = min(n, s0 + 65535)
            self._ext.gather_rows(llr.data_ptr(), self.n_vars, sel[s0:].data_ptr(), s1 - s0,
                                  rows[s0:].data_ptr(), stream.cuda_stream)
        return rows.cpu().numpy()

    def collect_uncorrected_awgn(self, flags, sigma: float, seed: int, offset: int = 0,
                                 punct=None, short=None, stream=None):
        """``collect_uncorrected`` after ``decode_awgn``: the failing frames' LLR rows
        regenerated from the channel (``ldpc_channel_awgn_rows``, the same values ``awgn`` would
        have written), so the sweep keeps the in-kernel channel while collecting."""
        torch = self._torch
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        punct = getattr(self, "punct", (0, 0)) if punct is None else punct
        short = getattr(self, "short", (0, 0)) if short is None else short
        with torch.cuda.stream(stream):          # (allocations and the copy on `stream`)
            sel = self._uncorrected_index(flags, stream)
            n = int(sel.numel())
            if n == 0:
                return np.zeros((0, self.n_vars), np.float32)
            rows = torch.empty((n, self.n_vars), dtype=torch.float32, device=self.device)
            self._ext.channel_awgn_rows(rows.data_ptr(), sel.data_ptr(), n, self.n_vars, float(sigma),
                                        int(seed), int(offset), self.decoding_type, self.q_bit,
                                        int(punct[0]), int(punct[1]), int(short[0]), int(short[1]),
                                        self.clip, stream.cuda_stream)
            return rows.cpu().numpy()

    def format_uncor_rows(self, rows):
        """``write_uncor_file``'s text for float32 LLR rows [n, N*z] as bytes, formatted by the
        native ``ldpc_format_uncor_rows`` (byte-identical to np.savetxt with "%.1f")."""
        return self._ext.format_uncor_rows(rows)

    def awgn(self, B: int, sigma: float, seed: int, offset: int = 0, punct=None, short=None,
             out=None, stream=None):
        """On-GPU AWGN LLRs [B, N*z] for the all-zero word (Philox, see ldpc_channel.hip).
        ``punct`` / ``short`` default to the ranges the decoder was built with (``Decoder``)."""
        torch = self._torch
        punct = getattr(self, "punct", (0, 0)) if punct is None else punct
        short = getattr(self, "short", (0, 0)) if short is None else short
        if out is None:
            out = torch.empty((B, self.n_vars), dtype=torch.float32, device=self.device)
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        self._ext.channel_awgn(out.data_ptr(), int(B), self.n_vars, float(sigma), int(seed),
                               int(offset), self.decoding_type, self.q_bit, int(punct[0]),
                               int(punct[1]), int(short[0]), int(short[1]), self.clip,
                               stream.cuda_stream)
        return out


def Decoder(graph_txt: str, z: int, punct=(0, 0), short=(0, 0), sharing=(3, 0, 3),
            decoding_type: int = DECODING_QMS, q_bit: int = 5, weights_txt: Optional[str] = None,
            T: Optional[int] = None, target_node: int = 0, fixed_iter: int = 0,
            clip_LLR: float = 20.0, device=None, kernel: str = "auto", B_max: int = 0) -> NMSDecoder:
    """File-level constructor (SURVEY §8 b): a base-graph text file (``BaseGraph/*.txt``, read
    like ``init_parameter``, ``Main_Functions.py:8-38``) and a weights file
    (``Weights/*.txt``, ``Main_Functions.py:387-439``) -> an ``NMSDecoder``.

    ``punct`` / ``short`` are the 1-based inclusive ranges of ``create_mix_epoch``
    (``Print_Functions.py:29-72``); they belong to the channel, so they only become the
    defaults of ``awgn``.  ``T`` defaults to the number of iterations the weight file holds;
    without a weight file the decoder uses flat weights (alpha 1, beta 1) for ``T`` iterations.
    """
    from .code import load_base_graph
    from .weights import expand_weights, read_weight_file, flat_weights
    proto = load_base_graph(graph_txt)
    g = TannerGraph(proto, int(z))
    if weights_txt is not None:
        wf = read_weight_file(weights_txt)
        if T is None:
            T = max(int(b.shape[0]) for b in wf.blocks.values()) if wf.blocks else 1
        W = expand_weights(tuple(sharing), wf.blocks, int(T), g, fixed_iter)
    else:
        if T is None:
            raise ValueError("T is required without a weights file")
        W = flat_weights(g, int(T))
    dec = NMSDecoder(proto, z, W, decoding_type, q_bit, target_node, clip_LLR, device=device,
                     kernel=kernel, B_max=B_max)
    dec.punct = (int(punct[0]), int(punct[1]))
    dec.short = (int(short[0]), int(short[1]))
    return dec
