/*
 * ldpc_nms_debug.h — test infrastructure exported by libldpc_nms.so (not part of the decoder
 * ABI in ldpc_nms.h; host only and touching no device, but for ldpc_debug_events_out).
 */
#ifndef LDPC_NMS_DEBUG_H
#define LDPC_NMS_DEBUG_H

#include <stdint.h>

#include "ldpc_nms.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host-side bounds check of the bit-sliced kernel's reads (csrc/ldpc_bs.hip bs_bounds_check):
 * for every kernel instance (kBsInst) and UCN setting whose plan serves the proto graph with
 * the given weight properties (alpha_uniform: one check weight per iteration; beta_uniform: one
 * channel weight per iteration), the launch's own planning and host tables are built and every
 * index the kernel reads -- global tables, LDS regions, the dynamic LDS size -- is checked
 * against the allocation.  mode: the internal QMS mode (1 = q 5, 2 = q -5, 3 = q 4, 4 = q 3).
 * flags bit 0 (LDPC_BOUNDS_PRE_GUARD): check the cn_hd read without the `ql < cn_lanes` guard
 * (the round-4 fault), so a test can see the check catch it.  flags bit 1
 * (LDPC_BOUNDS_BIG_TABLES): take the in-prologue channel's sampler tables to be 4 bytes longer
 * than the LDS region the plan lends them (the slot region; bsc: the SGN region), wherever the
 * plan passes the test that lets that build run; the check then reports "channel tables".
 * flags bit 2 (LDPC_BOUNDS_ES): also check the plans of the early-stop instances (ldpc_decode_es),
 * with their hard-decision / syndrome reads on and their syndrome words in LDS; without it the
 * plans checked, and the count returned, are those of the decodes without the mode.  flags bit 3
 * (LDPC_BOUNDS_ES_BSC = 8): also check the compressed kernel's early-stop plan where a decode in
 * the mode would take it (no bsl plan serves the graph, uniform beta = 1: 5G BG1) -- its syndrome
 * words inside the RED region and before the alpha table, the LDS size, and the chunk, position
 * and channel-table checks of the bsc plan; one more plan in the count.  flags bit 4
 * (LDPC_BOUNDS_UCN1 = 16): also check the plan of the one-chunk UCN instance that decodes without
 * early stop take when UCN weights are set and no earlier instance serves them (wman with
 * alpha' != alpha: the last kBsInst entry) -- with the UCN setting alone, as only such requests
 * are planned on it: its hard decisions, its cn_hd and hard-decision-address reads and its packed
 * alpha-table address; one more plan in the count where the graph fits it, and without the bit
 * the plans checked and the count are those of the other instances.  Only
 * the checks read the flags, no kernel or launch path does.  Returns the number of plans
 * checked (>= 0) or a negative status; *violations = out-of-bounds reads found, msg = the
 * first one ("" if none). */
int ldpc_debug_bs_bounds(const int32_t* proto, int32_t M, int32_t N, int32_t z, int32_t T,
                         int32_t mode, int32_t alpha_uniform, int32_t beta_uniform, float clip,
                         int32_t flags, int32_t* violations, char* msg, int32_t msg_len);

/* The dispatch of the geometry-frozen builds of the bit-sliced kernel (csrc/ldpc_bs_frozen.h) for a
 * request on a proto graph: kind 0 a plain decode, 1 early stop, 2 the export / word builds; ucn:
 * UCN weights set.  plan / frozen [n]: the frozen fields as the request's plan has them (-1 without
 * a bsl plan) and as the frozen builds fix them; names: the fields' names, comma-separated.
 * Returns 1 when a frozen build serves the request, 0 when not, or a negative status.  Honours
 * LDPC_BS_FROZEN=0 as a launch does. */
int ldpc_debug_bs_frozen(const int32_t* proto, int32_t M, int32_t N, int32_t z, int32_t T, int32_t mode,
                         int32_t alpha_uniform, int32_t beta_uniform, int32_t ucn, int32_t kind,
                         float clip, int32_t* plan, int32_t* frozen, int32_t n, char* names,
                         int32_t names_len);

/* The place in the fixed table set (csrc/ldpc_beta_tabs.h, kBetaTab) of the check table the
 * bit-sliced kernels build for one weight alpha: mode 1 (q = 5) or 2 (q = -5), the modes of
 * csrc/ldpc_host.h; host only.  *out_id = the index, or -1 when the table is not in the set or the
 * mode is another; table (16 bytes, or NULL) takes the set's row of that index (untouched at -1).
 * Returns a status of ldpc_nms.h. */
int ldpc_debug_alpha_tid(float alpha, int32_t mode, int32_t* out_id, uint8_t* table);

/* The check-table ids a weight set [T][E] (alpha_ucn [T][E] or NULL) gets on a proto graph
 * (host::analyze_weights, what ldpc_weights_set uploads): ids [T] takes them.  Returns 1 when the
 * ids are filled (alpha one value per iteration and no UCN weights), 0 when there are none (ids
 * untouched: the kernels' argument stays null), or a negative status.  Host only. */
int ldpc_debug_alpha_tids(const int32_t* proto, int32_t M, int32_t N, int32_t z, int32_t T,
                          const float* alpha, const float* alpha_ucn, int32_t* ids);

/* The dispatch of the bit-sliced builds with the weights frozen in kind (csrc/ldpc_bs_kernel.h, WF)
 * for a request of T iterations on a proto graph with a weight set of T_w >= T iterations (alpha,
 * alpha_ucn or NULL [T_w][E], beta [T_w][N]); kind as for ldpc_debug_bs_frozen.  aids / bids [T]
 * (or NULL) take the ids the launch hands its kernel: the check tables' and column 0 of the channel
 * tables', -1 where it hands none of that kind; *identity (or NULL) the mask of the iterations
 * whose channel table is the identity; alpha_tid_in [T_w] (or NULL) replaces the check ids the
 * analysis found.  Returns 1 when such a build serves the request, 0 when not, or a negative
 * status.  Honours LDPC_BS_WF, LDPC_BS_AFIX, LDPC_BS_NOBFIX and LDPC_BS_FROZEN as a launch does. */
int ldpc_debug_bs_wf(const int32_t* proto, int32_t M, int32_t N, int32_t z, int32_t T_w,
                     const float* alpha, const float* alpha_ucn, const float* beta, int32_t T,
                     int32_t mode, int32_t kind, float clip, int32_t* aids, int32_t* bids,
                     uint64_t* identity, const int32_t* alpha_tid_in);

/* The event collector of ldpc_decode_events (csrc/ldpc_events.hip, events_out) on caller-supplied
 * device buffers instead of a decode's: planes_dev [ceil(B/32)][N*z], bit r of word (pack, v) =
 * variable v of frame 32 pack + r (the bits of a ragged last pack's frames past B may hold
 * anything); bad_dev [ceil(B/32)], nonzero: the pack is skipped, whatever its planes hold;
 * n_iter_dev [B] or NULL (every record then takes T).  Of `outputs`, size, frame_base, cap and the
 * ev_* buffers are used as ldpc_decode_events uses them and frame_flags (or NULL) takes 0x80 for
 * the frames of skipped packs; the other fields are not read.  Launches the one kernel on
 * `stream` on the context's device: so a test can hand it words no decode here produces (a wrong
 * codeword: a > 0, b = 0).  Returns a status of ldpc_nms.h. */
int ldpc_debug_events_out(ldpc_ctx* ctx, const uint32_t* planes_dev, const uint32_t* bad_dev, int64_t B,
                          int32_t target_bits, const uint8_t* n_iter_dev, int32_t T,
                          const ldpc_event_outputs* outputs, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LDPC_NMS_DEBUG_H */
