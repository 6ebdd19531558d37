/*
 * ldpc_nms.h — C ABI of the MI355X neural min-sum (NMS / quantized NMS) LDPC decoder.
 *
 * The reference (ghy1228/LDPC_Error_Floor) has no FFI: its decoder is a TF1 graph built by
 * build_neural_network (Main_Functions.py:157-385) and executed through
 *     sess.run(fetches=net_dict["ya_output_all"] [, net_dict["lossa"]],
 *              feed_dict={xa: X[B,N,z], ya: Y, etha: e, learn_rate: 0})
 * (Print_Functions.py:147-151).  Each entry point below replaces one piece of that:
 *
 *   ldpc_graph_create   <- init_parameter + init_connecting_matrix (Main_Functions.py:8-150)
 *   ldpc_weights_set    <- weight_init's var_{i}_{t} (Main_Functions.py:387-439), already
 *                          expanded per iteration by the sharing rules (:167-174, :266-304)
 *   ldpc_ctx_create     <- the placeholders' fixed batch size (main_Base.py:122-127)
 *   ldpc_decode         <- sess.run of the T unrolled iterations; app_all == ya_output_all,
 *                          counters == calc_ber_fer (Print_Functions.py:100-118) on device
 *
 * Conventions: LLRs are log(p1/p0) (Print_Functions.py:45-46), bit index j*z+g, proto edges
 * in row-major order E(C).  All device pointers are owned by the caller (e.g. torch
 * tensors); the library owns graph tables, weights and per-context scratch.  Every call
 * returns LDPC_OK (0) or a negative status; no exception crosses the boundary.  A context
 * must be used by one host thread / stream at a time; there is no global mutable state.
 */
#ifndef LDPC_NMS_H
#define LDPC_NMS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LDPC_NMS_ABI_VERSION 3     /* 2: ldpc_decode_outputs.iter_wrong, ldpc_ctx_last_kernel;
                                      3: ldpc_decode_params.outputs_size */

typedef struct ldpc_graph ldpc_graph;
typedef struct ldpc_ctx ldpc_ctx;

enum ldpc_status {
    LDPC_OK = 0,
    LDPC_ERR_ARG = -1,          /* bad argument (null pointer, size, unsupported mode) */
    LDPC_ERR_HIP = -2,          /* a HIP runtime call or kernel launch failed */
    LDPC_ERR_OOM = -3,          /* device allocation failed */
    LDPC_ERR_STATE = -4,        /* weights not set / B or T above the context limits */
    LDPC_ERR_UNSUPPORTED = -5   /* valid request this build cannot serve */
};

enum ldpc_decoding_type {       /* decoding_type of main_Base.py:27 */
    LDPC_DEC_SP = 0,            /* sum-product: tanh / atanh check update (flood kernel) */
    LDPC_DEC_MS = 1,            /* min-sum fp32, messages clipped to +-clip_llr */
    LDPC_DEC_QMS = 2,           /* quantized min-sum on the q_bit grid */
    LDPC_DEC_MS_NONUDGE = 3     /* min-sum without the 0 -> 1e-4 nudge */
};

enum ldpc_kernel {
    LDPC_KERNEL_AUTO = 0,       /* fused when supported, else flooding */
    LDPC_KERNEL_FLOOD = 1,      /* two edge-parallel kernels per iteration, state in HBM */
    LDPC_KERNEL_FUSED = 2       /* all T iterations in one launch, state in LDS/registers */
};

typedef struct ldpc_decode_params {
    int32_t T;                  /* iterations (training_iter_end), 1 <= T <= T_max */
    int32_t decoding_type;      /* ldpc_decoding_type */
    int32_t q_bit;              /* 6, 5, -5, 4 or 3 (QMS only) */
    int32_t target_bits;        /* Nt*z: width of app_all and of the FER/BER bit range */
    float clip_llr;             /* clip_LLR (20.0 in the reference) */
    int32_t kernel;             /* ldpc_kernel */
    int32_t outputs_size;       /* sizeof(ldpc_decode_outputs) the caller was built with: 0 = the
                                   ABI-1 struct (five pointers, no iter_wrong; ABI-1 callers zeroed
                                   this word as reserved), sizeof(ldpc_decode_outputs) = this
                                   header's struct; any other value -> LDPC_ERR_ARG.  The library
                                   never reads past the size the caller declares.  An ABI-2
                                   binary (iter_wrong set, this word zeroed as reserved[0]) is
                                   read as ABI 1 and gets no iter_wrong: ABI-2 callers must be
                                   rebuilt against this header, and a caller relying on
                                   iter_wrong checks ldpc_abi_version() >= 3 first. */
    int32_t reserved;
} ldpc_decode_params;

typedef struct ldpc_decode_outputs {
    float* app_all;             /* [T][B][target_bits] f32 (== ya_output_all) or NULL */
    uint32_t* hard_bits;        /* [T][B][ceil(N*z/32)] bit v%32 of word v/32, or NULL */
    uint32_t* synd_bits;        /* [T][B][ceil(M*z/32)] syndrome of hard_bits[t], or NULL */
    int64_t* counters;          /* [4] += {bit errors @T-1, frames wrong @T-1,
                                   frames wrong at every t, 2*loss (loss_type 2, etha 0)}
                                   for the all-zero codeword; or NULL */
    uint8_t* frame_flags;       /* [B] bit0 wrong at every t (uncor), bit1 wrong @T-1; or NULL */
    uint32_t* iter_wrong;       /* [T][ceil(B/32)]: bit b%32 of word (t, b/32) = frame b has a hard
                                   decision 1 among the target bits at iteration t (the per-iteration
                                   frame error of calc_ber_fer, Print_Functions.py:100-118; the
                                   all-zero codeword), bits past B zero; or NULL.  Every kernel
                                   serves it, the counters-only ones included.  Read only when
                                   ldpc_decode_params.outputs_size declares it (ABI 3). */
} ldpc_decode_outputs;

int ldpc_abi_version(void);
const char* ldpc_status_string(int status);

/* proto: host [M][N] row-major, -1 = no edge, else cyclic shift (taken mod z). */
int ldpc_graph_create(const int32_t* proto, int32_t M, int32_t N, int32_t z, int32_t device,
                      ldpc_graph** out);
int ldpc_graph_destroy(ldpc_graph* g);
/* dims[8] = {M, N, z, E, n_checks, n_vars, n_edges, max_check_degree} */
int ldpc_graph_query(const ldpc_graph* g, int32_t* dims);

/* Host tables, copied to the device: alpha [T][E] (E(C) order), alpha_ucn [T][E] or NULL
   (UCN weighting off), beta [T][N]. */
int ldpc_weights_set(ldpc_graph* g, int32_t T, const float* alpha, const float* alpha_ucn,
                     const float* beta);

int ldpc_ctx_create(ldpc_graph* g, int64_t B_max, int32_t T_max, ldpc_ctx** out);
int ldpc_ctx_destroy(ldpc_ctx* c);

/* llr_dev: device [B][N*z] f32 (natural bit order, log p1/p0).  stream: hipStream_t (NULL =
   default stream).  Asynchronous: returns after enqueueing on the stream. */
int ldpc_decode(ldpc_ctx* c, const float* llr_dev, int64_t B, const ldpc_decode_params* p,
                const ldpc_decode_outputs* o, void* stream);

/* Bytes of HBM traffic per codeword the selected kernel is designed to move (for the
   roofline report), and a short kernel name.  Returns 0 if unsupported. */
int ldpc_kernel_info(const ldpc_ctx* c, const ldpc_decode_params* p, int64_t* bytes_per_cw,
                     char* name, int32_t name_len);

/* Name of the kernel that served the last successful ldpc_decode / ldpc_decode_awgn on this
   context (empty before the first).  Which kernel runs depends on the requested outputs: APP
   exports run v5 or flood, counters / frame flags / iter_wrong / hard_bits / synd_bits of the
   QMS grids the bit-sliced kernels ("bsl[...]", "bsc[...]"), whose hard-bit export is a
   separate build of the same kernel that also stores each iteration's hard decisions. */
int ldpc_ctx_last_kernel(const ldpc_ctx* c, char* name, int32_t name_len);

/* 1 when the last successful decode on this context ran a geometry-frozen build of its bit-sliced
   kernel (the graph's pack geometry as compile-time constants; same name, same results), 0 when it
   ran the generic build or another kernel; LDPC_ERR_ARG for a null context.  The environment
   variable LDPC_BS_FROZEN=0, read at every launch, forces the generic build. */
int ldpc_ctx_last_frozen(const ldpc_ctx* c);

/* 1 when the last successful decode on this context ran a bit-sliced kernel ("bsl[...]") that
   weighed its check minima through the fixed-set immediate tables (one alpha per iteration, q = 5
   or -5, every iteration's table in the set; same name, same results), 0 when it read the tables
   from LDS or another kernel ran; LDPC_ERR_ARG for a null context.  The environment variable
   LDPC_BS_AFIX=0, read at every launch, forces the LDS tables. */
int ldpc_ctx_last_afix(const ldpc_ctx* c);

/* 1 when the last successful decode on this context ran a bit-sliced kernel ("bsl[...]") in a build
   with the weights frozen in kind: a geometry-frozen build whose every check table and channel
   table is one of the fixed set (or the identity channel table) and which reads their ids from LDS
   (same name, same results); 0 when another build or kernel ran; LDPC_ERR_ARG for a null context.
   The environment variable LDPC_BS_WF=0, read at every launch, forces the other builds; so do
   LDPC_BS_AFIX=0, LDPC_BS_NOBFIX and LDPC_BS_FROZEN=0. */
int ldpc_ctx_last_wf(const ldpc_ctx* c);

/* On-GPU AWGN channel for the all-zero codeword (create_mix_epoch, Print_Functions.py:29-72):
   writes llr_dev [B][n_vars] f32 = Q(2(sigma*n - 1)/sigma^2) with punctured (1-based bits
   punct_start..punct_end, 0 = none) -> 0 and shortened -> -clip_llr.  Counter-based Philox
   streams indexed by (seed, offset + b, element): shards generated with their global codeword
   offset reproduce the single-GPU stream.  QMS: the quantized level is sampled exactly from
   its distribution (64-bit CDF thresholds computed in float64, one Philox per 4 codewords of a
   variable); float modes: Box-Muller with a 53-bit uniform under the logarithm (tails to ~8.6
   sigma).  See csrc/ldpc_awgn.h. */
int ldpc_channel_awgn(float* llr_dev, int64_t B, int32_t n_vars, double sigma, uint64_t seed,
                      int64_t offset, int32_t decoding_type, int32_t q_bit, int32_t punct_start,
                      int32_t punct_end, int32_t short_start, int32_t short_end, float clip_llr,
                      void* stream);

/* In-decoder channel for throughput sweeps (SURVEY §8 f rank 1): the LLRs of the B codewords
   come from the same generator as ldpc_channel_awgn (same seed, global codeword offset,
   puncture/shorten) and never cross HBM as floats: APP exports generate them in the fused v5
   kernel's prologue; counters-only QMS decodes of the bit-sliced kernels take a byte channel
   (one byte per LLR, already in the layout their prologue packs into bit planes); flood and the
   float-mode kernel generate float LLRs into a context buffer first.  The result is identical to
   ldpc_channel_awgn followed by ldpc_decode.  Replaces create_mix_epoch + sess.run in the
   compute_results loop (Print_Functions.py:29-72, :130-165). */
typedef struct ldpc_channel_params {
    double sigma;                 /* noise standard deviation (SNR -> sigma: init_parameter) */
    uint64_t seed;
    int64_t offset;               /* global index of the batch's first codeword */
    int32_t punct_start, punct_end, short_start, short_end;   /* 1-based, 0 = none */
    int32_t reserved[4];
} ldpc_channel_params;

int ldpc_decode_awgn(ldpc_ctx* ctx, int64_t B, const ldpc_decode_params* params,
                     const ldpc_channel_params* channel, const ldpc_decode_outputs* outputs,
                     void* stream);

/* Whether ldpc_decode_awgn with these parameters generates the channel inside the decoding
   kernel (the v5 prologue for APP exports, the bit-sliced kernels' prologue for counters-only QMS
   decodes): 1, else 0 (the channel kernel writes float LLRs to the context's buffer first), or a
   negative status.  has_short: the channel has shortened bits; app: an APP export is asked for.
   The decision ldpc_decode_awgn itself takes; a decode it served in-kernel also reports its
   kernel through ldpc_ctx_last_kernel with the suffix "+gen". */
int ldpc_awgn_in_kernel(const ldpc_ctx* ctx, const ldpc_decode_params* params, int32_t has_short,
                        int32_t app);

/* Syndrome-based early termination (opt-in).  These entry points have NO
   counterpart in the reference, whose unrolled graph always runs T iterations: their results are
   defined here and are not compute_results' numbers.  Per codeword b, for the all-zero codeword,
   with hd_t = (APP_t >= 0) and s_t the syndrome of hd_t over all M*z checks and N*z variables:
     stop(b)   = the smallest t in [0, T) with s_t == 0, else T - 1;
     n_iter(b) = stop(b) + 1, in [1, T] (at least one iteration always runs);
   the frame's outputs are frozen at stop(b), whatever s_t does later, and do not depend on which
   other codewords share its pack or batch.
     counters[0] += the ones among the first target_bits of hd_stop
     counters[1] += [hd_stop has a one among them]
     counters[2] += [the frame was wrong at every t <= stop(b)]
     counters[3]    is left untouched (the loss is a training quantity)
     frame_flags[b] bit 0 = wrong at every t <= stop, bit 1 = wrong at stop (as
                    ldpc_collect_frames reads them)
     n_iter[b]      uint8 [B], or NULL
     iter_hist[t]  += the frames with n_iter == t + 1; int64 [T], or NULL
   Input LLRs must lie on the quantizer grid (shortened bits at +-clip_llr allowed); the
   library's own channel produces such LLRs.  A pack of 32 codewords (b / 32) holding an off-grid
   value is not decoded: its frames get n_iter = 0 and frame_flags = 0x80 and enter neither the
   counters nor the histogram.
   Served: QMS with q_bit 5, -5, 4 or 3, no per-edge check weights, kernel AUTO or FUSED,
   T <= T_max, a graph one of the bit-sliced kernel's early-stop instances fits (one 32-codeword
   pack per workgroup: wman- and 802.11n-sized graphs), or, for a graph that only the compressed
   bit-sliced kernel serves (5G BG1 n2112), that kernel's early-stop build, which exists for
   channel weights that are all 1 (no UCN weights).  Anything else returns
   LDPC_ERR_UNSUPPORTED with nothing launched and no partial result.  ldpc_ctx_last_kernel
   reports "bsl[...,es]" or "bsc[...,es]" (and "+gen" when the channel was generated in the kernel).
   size: sizeof(ldpc_es_outputs) of the caller's header; any other value -> LDPC_ERR_ARG. */
typedef struct ldpc_es_outputs {
    int32_t size;
    int32_t reserved;
    int64_t* counters;          /* [4], elements 0..2 accumulated, or NULL */
    uint8_t* frame_flags;       /* [B] or NULL */
    uint8_t* n_iter;            /* [B] or NULL */
    int64_t* iter_hist;         /* [T] accumulated, or NULL */
} ldpc_es_outputs;

/* ldpc_decode with the early-stop rule above (no reference counterpart). */
int ldpc_decode_es(ldpc_ctx* ctx, const float* llr_dev, int64_t B, const ldpc_decode_params* params,
                   const ldpc_es_outputs* es_outputs, void* stream);
/* ldpc_decode_awgn with the early-stop rule above (no reference counterpart): identical to
   ldpc_channel_awgn followed by ldpc_decode_es. */
int ldpc_decode_awgn_es(ldpc_ctx* ctx, int64_t B, const ldpc_decode_params* params,
                        const ldpc_channel_params* channel, const ldpc_es_outputs* es_outputs,
                        void* stream);
/* Whether ldpc_decode_es serves these parameters on this context: 1, 0, or a negative status
   (no reference counterpart). */
int ldpc_es_supported(const ldpc_ctx* ctx, const ldpc_decode_params* params);

/* The decoded word: the hard decisions of the LAST iteration and a per-frame
   "is not a codeword" flag, from the same launch of the bit-sliced kernels that produces the
   counters.  No new arithmetic: for codeword b,
     hard_last[b]   = hd_{T-1} = (APP_{T-1} >= 0) over all N*z variables, packed as
                      hard_bits[T-1][b] is: ceil(N*z/32) words, bit v % 32 of word v / 32, the
                      bits past N*z zero; punctured and shortened bits included
     word_flags[b]    bit 0 = the syndrome of hard_last[b] over all M*z checks is nonzero
     counters, frame_flags  as ldpc_decode gives them (for the all-zero codeword)
   The only workspace is ceil(B_max/32) * N*z * 4 bytes (one word per 32 codewords and variable),
   allocated at the first call; nothing is proportional to T.
   Input LLRs must lie on the quantizer grid (shortened bits at +-clip_llr allowed), the rule of
   the early-stop mode.  A pack of 32 codewords (b / 32) holding an off-grid value is not decoded:
   word_flags = 0x80, frame_flags = 0x80, hard_last rows all zero, nothing in the counters.
   Served: what the bit-sliced kernels decode -- QMS with q_bit 5, -5, 4 or 3, no per-edge check
   weights, kernel AUTO or FUSED, a graph the bit-sliced kernel (bsl) or else the compressed one
   (bsc) fits, with or without UCN weights.  Anything else (the float modes, q_bit 6, flood, graphs
   only the v5 kernel serves) returns LDPC_ERR_UNSUPPORTED with nothing launched and nothing
   written.  ldpc_ctx_last_kernel reports the kernel's name with ",word" inside the brackets
   ("bsl[p32,w9,d15,v6,l4,word]").  params->outputs_size is not read.
   size: sizeof(ldpc_word_outputs) of the caller's header; any other value -> LDPC_ERR_ARG. */
typedef struct ldpc_word_outputs {
    int32_t size;
    int32_t reserved;
    uint32_t* hard_last;        /* [B][ceil(N*z/32)], required */
    uint8_t* word_flags;        /* [B] or NULL: bit 0 syndrome nonzero, 0x80 pack not decoded */
    int64_t* counters;          /* [4] accumulated as ldpc_decode does, or NULL */
    uint8_t* frame_flags;       /* [B] as ldpc_decode (0x80: pack not decoded), or NULL */
} ldpc_word_outputs;

int ldpc_decode_word(ldpc_ctx* ctx, const float* llr_dev, int64_t B, const ldpc_decode_params* params,
                     const ldpc_word_outputs* word_outputs, void* stream);
/* Whether ldpc_decode_word serves these parameters on this context: 1, 0, or a negative status. */
int ldpc_word_supported(const ldpc_ctx* ctx, const ldpc_decode_params* params);

/* The decoded word of the early-stop decode (no reference counterpart): what a
   practical decoder returns, the hard decisions of the iteration the frame stopped at.  With
   stop(b), n_iter(b) and hd_t as the early-stop mode above defines them, for codeword b
     hard_stop[b]   = hd_{stop(b)} = (APP_{stop(b)} >= 0) over all N*z variables, punctured and
                      shortened bits included, packed as hard_last / hard_bits[t][b] are:
                      ceil(N*z/32) words, bit v % 32 of word v / 32, the bits past N*z zero.
                      Frozen at stop(b), whatever later iterations do, and independent of which
                      frames share the pack or batch.
     word_flags[b]    bit 0 = the syndrome of hard_stop[b] over all M*z checks is nonzero: 0 for
                      every frame with n_iter < T (the stop rule), [s_{T-1} != 0] when n_iter == T
     counters[0..2], frame_flags, n_iter, iter_hist   exactly ldpc_decode_es's for the same input
   A pack of 32 codewords holding an off-grid value is not decoded: word_flags = 0x80,
   frame_flags = 0x80, n_iter = 0, hard_stop rows all zero, nothing in the counters or histogram.
   The only workspace is ldpc_decode_word's, ceil(B_max/32) * N*z * 4 bytes, shared with it.
   Served: exactly what ldpc_es_supported serves; ldpc_decode_awgn_es_word is identical to
   ldpc_channel_awgn followed by ldpc_decode_es_word and generates the channel inside the kernel
   where ldpc_decode_awgn_es does.  Anything else returns LDPC_ERR_UNSUPPORTED with nothing
   launched and nothing written.  ldpc_ctx_last_kernel reports "bsl[...,es,word]" or
   "bsc[...,es,word]" (and "+gen").  params->outputs_size is not read.
   size: sizeof(ldpc_es_word_outputs) of the caller's header; any other value -> LDPC_ERR_ARG, as
   is a NULL hard_stop; both are checked before the context is read. */
typedef struct ldpc_es_word_outputs {
    int32_t size;
    int32_t reserved;
    uint32_t* hard_stop;        /* [B][ceil(N*z/32)], required */
    uint8_t* word_flags;        /* [B] or NULL: bit 0 syndrome nonzero, 0x80 pack not decoded */
    int64_t* counters;          /* [4], elements 0..2 accumulated, or NULL */
    uint8_t* frame_flags;       /* [B] or NULL */
    uint8_t* n_iter;            /* [B] or NULL */
    int64_t* iter_hist;         /* [T] accumulated, or NULL */
    uint64_t reserved1;         /* not read; pads the struct to 64 bytes */
} ldpc_es_word_outputs;

int ldpc_decode_es_word(ldpc_ctx* ctx, const float* llr_dev, int64_t B, const ldpc_decode_params* params,
                        const ldpc_es_word_outputs* outputs, void* stream);
int ldpc_decode_awgn_es_word(ldpc_ctx* ctx, int64_t B, const ldpc_decode_params* params,
                             const ldpc_channel_params* channel, const ldpc_es_word_outputs* outputs,
                             void* stream);
/* Whether ldpc_decode_es_word serves these parameters on this context: 1, 0, or a negative
   status. */
int ldpc_es_word_supported(const ldpc_ctx* ctx, const ldpc_decode_params* params);

/* Floor events (no reference counterpart): the word modes' decode with, in place
   of a row per frame, one record per EVENT, collected on the device.  An event is a decoded frame
   whose word -- hard_last[b] (early_stop = 0) or hard_stop[b] (early_stop = 1), as defined above --
   is nonzero anywhere over the N*z variables, punctured and shortened bits included (a nonzero
   syndrome implies a nonzero word, so the one test covers both).  Each event of the batch takes
   one slot k of the caller's buffers, reserved at *ev_count:
     ev_frame[k]   = frame_base + b, the frame's index (ldpc_decode_awgn_events: the channel's
                     offset + b, its global codeword index; frame_base is not read there)
     ev_info[k]    = { n_iter(b) (early_stop = 0: T),
                       a        = the ones of the word over all N*z variables,
                       a_target = the ones among its first target_bits (the frame's share of
                                  counters[0]; a_target > 0 <=> the frame counts in counters[1]),
                       b        = the ones of its syndrome over all M*z checks }
                     -- the (a, b) signature of a trapping set; b = 0 with a > 0 is an undetected
                     error, a wrong codeword
     ev_word[k]    = the word, packed as a row of hard_last is: ceil(N*z/32) words, bit v % 32 of
                     word v / 32, the bits past N*z zero; not written when ev_word is NULL
   *ev_count accumulates over calls, as counters do, and is never zeroed by the library: it is the
   number of events seen, the next free slot while it is below cap.  Events that would take a
   slot >= cap are counted and not written; nothing past cap is touched.  The order of the
   records is unspecified (sort by ev_frame on the host); all of one 32-frame pack's are adjacent.
   counters[0..2], frame_flags, n_iter, iter_hist are exactly ldpc_decode_es's (early_stop = 1) or
   counters and frame_flags ldpc_decode_word's (early_stop = 0; n_iter and iter_hist are then not
   written) for the same input.  A pack of 32 codewords holding an off-grid value is not decoded
   and is no event: frame_flags = 0x80, n_iter = 0, nothing in the counters or histogram.
   The workspace is ldpc_decode_word's, shared with it, and B_max bytes when n_iter is NULL.
   Served: early_stop = 0 exactly what ldpc_word_supported serves, early_stop = 1 exactly what
   ldpc_es_word_supported serves; ldpc_decode_awgn_events serves early_stop = 1 alone, is identical
   to ldpc_channel_awgn followed by ldpc_decode_events with frame_base = the channel's offset, and
   generates the channel inside the kernel where ldpc_decode_awgn_es_word does.  Anything else
   returns LDPC_ERR_UNSUPPORTED with nothing launched and nothing written.  ldpc_ctx_last_kernel
   reports "bsl[...,events]", "bsl[...,es,events]" or "bsc[...,es,events]" (and "+gen").
   params->outputs_size is not read.
   size: sizeof(ldpc_event_outputs) of the caller's header; any other value -> LDPC_ERR_ARG, as are
   a NULL ev_count, ev_frame or ev_info and a negative cap; all checked before the context is read. */
typedef struct ldpc_event_outputs {
    int32_t size;
    int32_t early_stop;         /* 0: the last iteration's word, 1: the stop iteration's */
    int64_t frame_base;         /* index of the batch's first frame */
    int64_t cap;                /* slots of ev_frame / ev_info / ev_word, >= 0 */
    int64_t* ev_count;          /* [1] accumulated, required */
    int64_t* ev_frame;          /* [cap], required */
    int32_t* ev_info;           /* [cap][4] {n_iter, a, a_target, b}, required */
    uint32_t* ev_word;          /* [cap][ceil(N*z/32)] or NULL */
    int64_t* counters;          /* [4], elements 0..2 accumulated, or NULL */
    uint8_t* frame_flags;       /* [B] or NULL */
    uint8_t* n_iter;            /* [B] or NULL (early_stop = 1) */
    int64_t* iter_hist;         /* [T] accumulated, or NULL (early_stop = 1) */
    uint64_t reserved1;         /* not read; pads the struct to 96 bytes */
} ldpc_event_outputs;

int ldpc_decode_events(ldpc_ctx* ctx, const float* llr_dev, int64_t B, const ldpc_decode_params* params,
                       const ldpc_event_outputs* outputs, void* stream);
int ldpc_decode_awgn_events(ldpc_ctx* ctx, int64_t B, const ldpc_decode_params* params,
                            const ldpc_channel_params* channel, const ldpc_event_outputs* outputs,
                            void* stream);
/* Whether ldpc_decode_events with outputs->early_stop = early_stop serves these parameters on this
   context: 1, 0, or a negative status. */
int ldpc_events_supported(const ldpc_ctx* ctx, const ldpc_decode_params* params, int32_t early_stop);

/* int8 quantized LLRs (no reference counterpart): the decodes above of LLRs that
   are already on the quantizer grid, one byte per LLR instead of four.
     q8_dev   device int8 [B][N*z], row-major, any alignment: g = LLR / step in grid units,
              step 0.5 / 1 / 1 / 2 and qmax 15 / 15 / 7 / 3 for q_bit 5 / -5 / 4 / 3
              -qmax <= g <= qmax   LLR g * step
              -128 / +127          LLR -clip_llr / +clip_llr (a shortened bit), where the kernel
                                   decodes shortened bits (ldpc_q8_supported with has_short = 1)
              every other byte is invalid (so is a marker where has_short = 1 is not served)
   For valid input every output equals, bit for bit, that of ldpc_decode / ldpc_decode_word on the
   float LLRs the bytes stand for.  A pack of 32 codewords (b / 32) holding an invalid byte in one
   of its codewords is not decoded: frame_flags = 0x80 (word_flags = 0x80, hard_last rows zero),
   nothing in the counters or in iter_wrong; there is no fixup launch.
   ldpc_decode_q8: outputs->counters / frame_flags / iter_wrong (params->outputs_size as for
   ldpc_decode); app_all, hard_bits and synd_bits must be NULL.  ldpc_decode_q8_word:
   ldpc_decode_word's outputs.  A NULL q8_dev, a wrong struct size or such an export pointer is
   LDPC_ERR_ARG before the context is read.
   Served exactly where the bit-sliced kernels serve the float request of the same kind (the
   counters-only ldpc_decode, ldpc_decode_word) on the instances a plan takes by default; anything
   else is LDPC_ERR_UNSUPPORTED with nothing launched or written.  ldpc_ctx_last_kernel reports
   "bsl[...]+q8", "bsl[...,word]+q8" or "bsc[...]+q8". */
int ldpc_decode_q8(ldpc_ctx* ctx, const int8_t* q8_dev, int64_t B, const ldpc_decode_params* params,
                   const ldpc_decode_outputs* outputs, void* stream);
int ldpc_decode_q8_word(ldpc_ctx* ctx, const int8_t* q8_dev, int64_t B, const ldpc_decode_params* params,
                        const ldpc_word_outputs* word_outputs, void* stream);
/* Whether ldpc_decode_q8 (word = 0) or ldpc_decode_q8_word (word = 1) serves these parameters on
   this context, for input with (has_short = 1) or without the +-clip markers: 1, 0, or a negative
   status. */
int ldpc_q8_supported(const ldpc_ctx* ctx, const ldpc_decode_params* params, int32_t has_short,
                      int32_t word);
/* int8 LLRs in the early-stop, stop-iteration-word and events modes: q8_dev as
   above.  For every valid q8, every output equals, bit for bit, that of the float entry point of
   the same kind -- ldpc_decode_es, ldpc_decode_es_word, ldpc_decode_events -- on the float LLRs
   the bytes stand for.  A pack of 32 codewords holding an invalid byte in one of its codewords is
   not decoded, as in those modes a pack off the grid is not: frame_flags = 0x80, n_iter = 0
   (hard_stop rows zero, word_flags = 0x80, no event), nothing in the counters or in iter_hist.
   ldpc_decode_q8_events serves both values of outputs->early_stop: 1 decodes with the int8
   early-stop builds, 0 with the int8 word build of ldpc_decode_q8_word (served where
   ldpc_q8_supported with word = 1 is).
   A NULL q8_dev, a wrong struct size or a missing required pointer (hard_stop; ev_count, ev_frame,
   ev_info, cap < 0) is LDPC_ERR_ARG before the context is read.  Served where the float entry
   point is served and the plan's early-stop instance has the int8 builds (bsl: wman, 802.11n;
   bsc: the beta = 1 builds); anything else is LDPC_ERR_UNSUPPORTED with nothing launched or
   written.  ldpc_ctx_last_kernel reports the float mode's name and "+q8": "bsl[...,es]+q8",
   "bsl[...,es,word]+q8", "bsl[...,es,events]+q8", "bsl[...,events]+q8", the "bsc[...]" forms
   likewise. */
int ldpc_decode_q8_es(ldpc_ctx* ctx, const int8_t* q8_dev, int64_t B, const ldpc_decode_params* params,
                      const ldpc_es_outputs* es_outputs, void* stream);
int ldpc_decode_q8_es_word(ldpc_ctx* ctx, const int8_t* q8_dev, int64_t B, const ldpc_decode_params* params,
                           const ldpc_es_word_outputs* es_word_outputs, void* stream);
int ldpc_decode_q8_events(ldpc_ctx* ctx, const int8_t* q8_dev, int64_t B, const ldpc_decode_params* params,
                          const ldpc_event_outputs* outputs, void* stream);
/* Whether the early-stop entry points above (ldpc_decode_q8_es, ldpc_decode_q8_es_word,
   ldpc_decode_q8_events with early_stop = 1) serve these parameters on this context, for input
   with (has_short = 1) or without the +-clip markers: 1, 0, or a negative status. */
int ldpc_q8_es_supported(const ldpc_ctx* ctx, const ldpc_decode_params* params, int32_t has_short);
/* ldpc_channel_awgn's QMS channel as int8 rows (q8_dev [B][n_vars]): the same Philox stream and
   level sampler, so the bytes equal ldpc_llr_to_q8 of ldpc_channel_awgn's output; punctured bits
   0, shortened bits -128.  QMS with q_bit 5, -5, 4 or 3 only (else LDPC_ERR_UNSUPPORTED). */
int ldpc_channel_awgn_q8(int8_t* q8_dev, int64_t B, int32_t n_vars, double sigma, uint64_t seed,
                         int64_t offset, int32_t q_bit, int32_t punct_start, int32_t punct_end,
                         int32_t short_start, int32_t short_end, void* stream);
/* q8_dev[i] = the byte of llr_dev[i] on q_bit's grid for i < n: rint(llr / step) where that is
   exact and within +-qmax, -128 / +127 for -clip_llr / +clip_llr otherwise; any other value is
   stored saturated and counted in *n_invalid_dev (int64, zeroed by the call; may be NULL). */
int ldpc_llr_to_q8(const float* llr_dev, int64_t n, int32_t q_bit, float clip_llr, int8_t* q8_dev,
                   int64_t* n_invalid_dev, void* stream);

/* The LLR rows ldpc_channel_awgn(B, ..., offset) would write at batch rows idx_dev[0..n) (each
   index < B, any order), into rows_dev[n][n_vars]: the same values bit for bit, generated for
   those codewords only -- the uncorrected-word sweep regenerates the few failing frames' rows
   after a decode whose channel was generated inside the kernel (ldpc_decode_awgn). */
int ldpc_channel_awgn_rows(float* rows_dev, const int64_t* idx_dev, int64_t n, int32_t n_vars,
                           double sigma, uint64_t seed, int64_t offset, int32_t decoding_type,
                           int32_t q_bit, int32_t punct_start, int32_t punct_end,
                           int32_t short_start, int32_t short_end, float clip_llr, void* stream);

/* Uncorrected-frame collection for the on-device sweep (replaces the host selection in
   compute_results -> write_uncor_file, Print_Functions.py:155-156 and :120-126).
   Writes the indices b < B with (frame_flags[b] & mask) == want into idx_dev[0..cap) (order
   within the batch is not preserved: sort the few indices on the host) and the number of
   matches (which may exceed cap) into *count_dev (zeroed by the call).  With the decoder's
   frame_flags, mask = want = 1 selects the frames wrong at every iteration (uncor_flag). */
int ldpc_collect_frames(const uint8_t* flags_dev, int64_t B, uint32_t mask, uint32_t want,
                        int64_t* idx_dev, int64_t cap, int64_t* count_dev, void* stream);

/* dst[r][:] = src[idx[r]][:] for r < n (n <= 65535 per call): the LLR rows of the collected
   frames, on the device, before the copy to the host. */
int ldpc_gather_rows(const float* src_dev, int64_t n_cols, const int64_t* idx_dev, int64_t n,
                     float* dst_dev, void* stream);

/* Host: the text of write_uncor_file's rows (Print_Functions.py:120-126, np.savetxt with
   fmt "%.1f", tab-delimited) for n float32 LLR rows of n_cols values: "0.0\t0.0\t0.0\t" then
   the negated LLRs, byte-identical to np.savetxt's output.  cap must be at least
   n * LDPC_UNCOR_ROW_BOUND(n_cols); *len = the bytes written. */
#define LDPC_UNCOR_ROW_BOUND(n_cols) (13 + 48 * (int64_t)(n_cols))
int ldpc_format_uncor_rows(const float* rows, int64_t n, int64_t n_cols, char* out, int64_t cap,
                           int64_t* len);

#ifdef __cplusplus
}
#endif
#endif /* LDPC_NMS_H */
