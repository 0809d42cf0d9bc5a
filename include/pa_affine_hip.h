/*
 * pa_affine_hip.h -- batched gap-affine global alignment on the GPU (libastarpa_c_hip.so, MI355X / gfx950).
 *
 * What `NW::new(cm, false, false).align(a, b)` of pa-base-algos computes (the full-matrix AffineFront, nw/affine.rs) for many
 * independent pairs: the cost and, optionally, the CIGAR of every pair, over the cost models AffineCost<0> and AffineCost<2> can express
 * (pa-affine-types/src/cost_model.rs:112-190: lcs, unit, linear, linear_asymmetric, affine, linear_affine, affine_asymmetric).
 * Sequences are any bytes, compared for equality (AffineFront builds no BitProfile); empty sequences are valid.  a and b are never
 * swapped: I consumes b, D consumes a.
 *
 * CIGAR: the reference's backward walk from (|a|, |b|, main) to (0, 0, main), taking at every state the first parent in
 * EditGraph::iterate_parents order whose cost fits (main layer: diagonal, linear ins, linear del, close of the insert layer, close of
 * the delete layer; affine layers: open before extend), printed as AffineCigar::to_string() (= X I D, the count left out when 1).
 *
 * Errors follow pa_bitpacking_hip.h: 0 or a negative PA_E_* code, pa_last_error() for the message.
 */
#ifndef PA_AFFINE_HIP_H
#define PA_AFFINE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* One cost model; 0 means absent (the reference's None).  The insert layer exists when ins_open and ins_extend are both non-zero, the
 * delete layer likewise; a gap of length L in a layer costs open + L * extend.  Every cost is in [1, 1000] or 0; a layer with only one
 * of its two costs, or a model with no way to insert or no way to delete, is PA_E_ARG.  (AffineCost<4>, double_affine, has no
 * representation here: pa_affine4_hip.h has its own batch type, pa_affine4_batch_*, global mode with cost and CIGAR.) */
typedef struct pa_affine_cost {
    int32_t sub, ins, del, ins_open, ins_extend, del_open, del_extend;
} pa_affine_cost;

/* Pair p aligns a[p] (a_len[p] bytes) against b[p].  For every pair, (|a| + |b| + 1) * (the largest edge cost, open + extend counted
 * as one) must be below 2^30, else PA_E_ARG naming the pair.  trace != 0 allows pa_affine_batch_align.  A failed create returns NULL.
 * Zero pairs is valid.  Pairs with |b| <= 1024 run several to a wavefront (segments of g = 1, 2, 4 .. 64 lanes of 16 rows each); longer
 * ones take a wavefront each, its strips of 1024 rows one after the other. */
typedef struct pa_affine_batch pa_affine_batch;
pa_affine_batch* pa_affine_batch_create(const uint8_t* const* a, const size_t* a_len, const uint8_t* const* b, const size_t* b_len,
                                        size_t npairs, const pa_affine_cost* cm, int trace);
/* Costs only.  cost_out[p] (may be NULL), kernel_ms (optional): HIP-event time of the forward kernel.  May be called again. */
int pa_affine_batch_run(pa_affine_batch* ab, int32_t* cost_out, float* kernel_ms);
/* Costs and CIGARs (trace batches only, else PA_E_ARG).  cigar_out[p] is malloc'ed (release with pa_free_cigars); on error every
 * cigar_out[p] is NULL.  The pairs run in chunks whose traceback codes (one byte per cell) stay within PA_AFFINE_TRACE_BUDGET_MB, or a
 * quarter of the free device memory; a pair whose codes alone exceed it is PA_E_ARG.  forward_ms / trace_ms (optional): HIP-event time
 * of the forward kernels and of the walks, summed over the chunks. */
int pa_affine_batch_align(pa_affine_batch* ab, int32_t* cost_out, char** cigar_out, float* forward_ms, float* trace_ms);
/* Costs and the same CIGARs as pa_affine_batch_align, in bounded device memory (trace batches only, else PA_E_ARG).  A cost-only pass
 * keeps checkpoints: M and I of the last row of every strip of 1024 rows but the last, and M and D of every row after columns tile_cols,
 * 2 tile_cols, ...  Then, round by round, the one tile (a strip's rows x tile_cols columns) in which each unfinished pair's walk stands is
 * filled with codes from its checkpoints, up to the column where the walk entered it, and the walk goes on to the tile's edge.
 * tile_cols: 0 for the default (1024), else in [64, 2^20] (PA_E_ARG otherwise).  A pair needs about |a| |b| / (8 tile_cols) +
 * |a| |b| / 128 bytes of checkpoints, one tile of (min(|a|, tile_cols) + 1) * (min(rows, 1024) + 1) bytes and |a| + |b| ops; the pairs run
 * in chunks within PA_AFFINE_TRACE_BUDGET_MB (or a quarter of the free device memory), and a pair that alone exceeds it is PA_E_ARG.
 * forward_ms / refill_ms / walk_ms (optional): HIP-event time of the checkpoint passes, the tile fills and the walks, summed. */
int pa_affine_batch_align_tiled(pa_affine_batch* ab, uint32_t tile_cols, int32_t* cost_out, char** cigar_out, float* forward_ms,
                                float* refill_ms, float* walk_ms);
/* The last pa_affine_batch_align_tiled: chunks, rounds (one fill and one walk launch each, summed over the chunks), tile jobs (tiles
 * filled, summed over pairs), cells those fills computed, and the largest chunk's per-pair device bytes. */
void pa_affine_batch_tiled_info(const pa_affine_batch* ab, double* chunks, double* rounds, double* tile_jobs, double* refill_cells,
                                double* chunk_bytes_max);
/* The chained route for pairs with |b| > 1024.  on = 0 (the default): the routes above, a wavefront per such pair.  on = 1: in
 * pa_affine_batch_run and in the checkpoint pass of pa_affine_batch_align_tiled every strip of 1024 rows of such a pair is a job of its
 * own, run by its own wavefront, and strip s + 1 reads the last row of strip s while strip s is still writing it; pairs with |b| <= 1024
 * keep their launch.  Costs and CIGARs are those of on = 0.  pa_affine_batch_align (a code byte per cell) has no chained form and
 * ignores the setting.  A chained pair needs (strips - 1) * (|a| + 1) * 8 bytes of boundary rows: pa_affine_batch_run cuts the chained
 * pairs into chunks within PA_AFFINE_TRACE_BUDGET_MB (or a quarter of the free device memory), and a pair whose rows alone exceed it is
 * PA_E_ARG naming the pair; pa_affine_batch_align_tiled counts these rows among its checkpoints already.  A strip waits for its rows for
 * a bounded time: should a strip never receive them, the call returns PA_E_INTERNAL, pa_last_error() names the chained route, and every
 * cost_out and cigar_out of that call is invalid.  A NULL batch, or a value other than 0 and 1, is PA_E_ARG. */
int pa_affine_batch_set_chain(pa_affine_batch* ab, int on);
/* The setting, and the last chained pass (a run, or the checkpoint passes of an align_tiled, with chaining on): pairs and strip jobs it
 * ran chained, its chunks, and the largest chunk's boundary-row bytes.  Every pointer may be NULL. */
void pa_affine_batch_chain_info(const pa_affine_batch* ab, double* on, double* chain_pairs, double* chain_jobs, double* chunks,
                                double* bnd_bytes_max);
/* Ends-free (semi-global) mode: a is the text, b the pattern, and b is always consumed whole.  Both switches are 0 by default, and with
 * both 0 nothing changes.  There is no counterpart in the reference (its only semi-global code is pa_bitpacking::search, unit costs).
 *   free_start = 1: M(i, 0) = 0 for every column i (I(i, 0) stays absent): a prefix of a costs nothing.
 *   free_end = 1:   the cost is the minimum of M(i, |b|) over i = 0 .. |a|, and `end` the lowest i that reaches it (the tie rule of
 *                   pa_search_batch_run); without it end = |a|.
 * So the cost is the least global cost of (a[s:e], b) over the allowed s <= e (s = 0 unless free_start, e = |a| unless free_end).  The
 * CIGAR is the same first-parent walk over the ends-free matrix, from (end, |b|, main); with free_start it stops at the first state
 * (i, 0, main) it reaches and start = i, else it runs to (0, 0, main) and start = 0.  It describes a[start:end] against b: the free
 * flanks are not printed.  The setting holds for every later run, align and align_tiled (all routes, chained or not) and invalidates what
 * pa_affine_batch_ends would report.  A NULL batch, or a value other than 0 and 1, is PA_E_ARG. */
int pa_affine_batch_set_free_ends(pa_affine_batch* ab, int free_start, int free_end);
/* start and end of every pair in the last successful run, align or align_tiled under the current setting (either pointer may be NULL).
 * After a cost-only run start_out[p] is -1 when free_start is on and 0 otherwise.  Before any such call, or after a change of the
 * setting, PA_E_ARG. */
int pa_affine_batch_ends(const pa_affine_batch* ab, int64_t* start_out, int64_t* end_out);
/* The last row under the current setting: M(i, |b|) for i = 0 .. |a| of pair p to out + offsets[p]; offsets[p] == UINT64_MAX skips the
 * pair.  In global mode these are the costs of b against every prefix of a, the last one the pair's cost.  Runs a cost-only pass of its
 * own over the pairs asked for, in chunks whose rows (4 bytes per column, device memory taken only here) stay within
 * PA_AFFINE_TRACE_BUDGET_MB or a quarter of the free device memory; a pair whose row alone exceeds it is PA_E_ARG naming the pair. */
int pa_affine_batch_last_row(pa_affine_batch* ab, int32_t* out, const uint64_t* offsets);
/* The diagonal-transition (WFA) route: the same global-mode cost as pa_affine_batch_run, found by keeping for every cost s = 0, 1, ..
 * the furthest-reaching point of every diagonal and layer (pa-base-algos dt.rs, cost_for_bounded_dist), so the work is about (cost) x
 * (diagonals reached) plus the bytes matched, not |a| |b|.  s_max in [0, 2^30) bounds the search: a pair whose cost exceeds it is "not
 * found", cost_out[p] = -1 (the reference's None).  There is no doubling, retry or fallback inside the call.  Every model
 * pa_affine_batch_create accepts is accepted (the largest single edge, at most 1000, sets the ring of fronts: largest edge + 1).
 * A batch whose ends-free setting is on is refused, PA_E_ARG (ends-free DT is pa_affine_batch_run_dt_ends).  The chain setting is ignored.  A pair takes a wavefront and, per
 * layer (3, or 1 for a model without affine layers), (largest edge + 2) * (D + 2) * 4 bytes of device memory, where s' = min(s_max, the
 * cost of deleting a and inserting b) and D the diagonals cost s' reaches, clipped to [-|b|, |a|]; the pairs run in chunks within
 * PA_AFFINE_TRACE_BUDGET_MB (or a quarter of the free device memory), and a pair that alone exceeds it is PA_E_ARG naming the pair.
 * kernel_ms (optional): HIP-event time of clearing the fronts and the kernel, summed over the chunks.  A NULL batch or a negative
 * s_max is PA_E_ARG.  Leaves every other route's results and settings as they were. */
int pa_affine_batch_run_dt(pa_affine_batch* ab, int32_t s_max, int32_t* cost_out, float* kernel_ms);
/* Costs and CIGARs by diagonal transition (trace batches only, else PA_E_ARG).  Keeps every front of a pair, (s' + 2) * (D + 2) * 4
 * bytes per layer plus |a| + |b| ops, chunked under the same budget, and walks back from (cost, main, |a|, |b|) to (0, main, 0, 0) over
 * the stored furthest-reaching values.  Main layer: the point before extension is the maximum over the parents in the order
 * substitution, linear insert, linear delete, close of the insert layer, close of the delete layer, each read from the front
 * `s - edge cost`; the matches down to it are emitted, and the walk moves to the first parent in that order that reaches the maximum.
 * Affine layers: open before extend.  At s = 0 the rest is matches.  The CIGAR has the cost of pa_affine_batch_align's and is a valid
 * path, but where several optimal paths exist it may be another one (DEVIATIONS.md).  A pair above s_max gets cost -1 and "".
 * cigar_out[p] is malloc'ed (pa_free_cigars); on error every cigar_out[p] is NULL. */
int pa_affine_batch_align_dt(pa_affine_batch* ab, int32_t s_max, int32_t* cost_out, char** cigar_out, float* forward_ms, float* trace_ms);
/* Ends-free (semi-global) diagonal transition: the cost and `end` of pa_affine_batch_run under pa_affine_batch_set_free_ends(free_start,
 * free_end), a the text and b the pattern, found in work proportional to cost x diagonals.  The switches are arguments of the call: the
 * batch's own ends-free setting, what pa_affine_batch_ends reports, the chain setting and every other route's results are neither read
 * nor changed.  The recurrence, layers, extension and ring are those of pa_affine_batch_run_dt, and three things differ:
 *   free_start = 1: front 0 starts every diagonal k = 0 .. |a| at (k, 0), and the live diagonals of cost s are
 *                   [-min(|b|, reach_ins(s)), |a|] (no further trimming).
 *   free_end = 1:   the pair is found at the first s at which any diagonal holds M_s[k] - k = |b|; end_out[p] is the lowest such
 *                   i = M_s[k] (the lowest column on ties, as in pa_affine_batch_set_free_ends).  Without it end = |a|.
 *   bound:          with either switch on s' = min(s_max, the gap cost of inserting b), which end = 0 or start = |a| always reaches.
 * Device memory per pair and layer: (largest edge + 2) * (D + 2) * 4 bytes, D the diagonals of [kmin, kmax] at s'.  Under free_start
 * the diagonals above |a| - |b| + reach_ins(s') are left out (no path within s' that passes there comes back to an end diagonal, so
 * nothing changes but the work), and kmax = min(|a|, |a| - |b| + reach_ins(s')) whatever the cost: D = kmax + min(|b|, reach_ins(s'))
 * + 1, at most |a| + reach + 1, i.e. about 4 (|a| - |b| + 2 reach) (largest edge + 2) bytes per layer: 35 KB in all for a 150-byte
 * pattern in a 400-byte text at s' = 120 under affine(4, 6, 2) (8 rows, 3 layers, 367 columns), against 12 KB with free_end alone, where D
 * is as in global mode.
 * A pair above s_max gets cost -1 and end -1.  With both switches 0 the call returns what pa_affine_batch_run_dt returns, and end = |a|.
 * A NULL batch, a switch other than 0 and 1, or an s_max outside [0, 2^30) is PA_E_ARG.  Chunking, the order of the pairs, the wide
 * blocks and the refusal of a pair that alone exceeds the budget are those of pa_affine_batch_run_dt. */
int pa_affine_batch_run_dt_ends(pa_affine_batch* ab, int free_start, int free_end, int32_t s_max,
                                int32_t* cost_out, int64_t* end_out, float* kernel_ms);
/* Costs, placements and CIGARs by ends-free diagonal transition (trace batches only, else PA_E_ARG).  Keeps every front of a pair,
 * (s' + 2) * (D + 2) * 4 bytes per layer plus |a| + |b| ops, and walks back from (cost, main, i = end, k = end - |b|) with the parent
 * order and tie rule of pa_affine_batch_align_dt down to s = 0, where the rest is i - k matches and start = k (0 without free_start).
 * The CIGAR describes a[start:end] against b.  Cost and end are those of pa_affine_batch_align in the same ends-free setting; start
 * and the CIGAR are this walk's own and may be another optimal placement (DEVIATIONS.md).  A pair above s_max gets cost -1, start -1,
 * end -1 and "".  cigar_out[p] is malloc'ed (pa_free_cigars); on error every cigar_out[p] is NULL. */
int pa_affine_batch_align_dt_ends(pa_affine_batch* ab, int free_start, int free_end, int32_t s_max, int32_t* cost_out,
                                  int64_t* start_out, int64_t* end_out, char** cigar_out, float* forward_ms, float* trace_ms);
/* The last DT call of either kind: pairs found and not found, chunks, front cells computed (layers x live diagonals, summed over the cost steps of
 * every pair), bytes compared while extending, and the largest chunk's device bytes.  Every pointer may be NULL. */
void pa_affine_batch_dt_info(const pa_affine_batch* ab, double* found, double* not_found, double* chunks, double* front_cells,
                             double* extend_chars, double* bytes_max);
/* pa_affine_batch_align_dt_ends in device memory that grows with the square root of the cost, not with the cost (trace batches only,
 * else PA_E_ARG): cost, start, end and CIGAR are those of pa_affine_batch_align_dt_ends(free_start, free_end, s_max), byte for byte.
 * With E the largest edge, front s depends on fronts s - E .. s - 1 only and a step of the walk lowers s by at most E.  The costs are
 * cut into segments of S >= E costs, segment c = [cS, cS + S - 1].  A checkpoint pass (pa_affine_batch_run_dt_ends' pass over the ring,
 * costs and ends as there) also stores the E fronts below every segment start cS, c >= 1.  Then rounds follow, from every pair's top
 * segment down, one fill launch and one walk launch per round over all unfinished pairs of the chunk: the fill puts the segment's E
 * checkpoint rows at the head of the pair's segment buffer and recomputes the fronts of the segment up to the pair's cost; the walk is
 * pa_affine_batch_align_dt_ends' walk with its state kept between rounds, until it leaves the segment or ends at s = 0.
 *   seg:  0 selects S = max(E, ceil(sqrt((s' + 1) E))) for every pair from its own s' (pa_affine_batch_run_dt_ends' bound: min(s_max,
 *         the gap cost that always reaches)); any other value is S for every pair and must lie in [E, 2^30), else PA_E_ARG.  Where S
 *         exceeds max(E, s' + 1) that is used instead: one segment.
 * Device bytes of a pair, with L = 3 layers (1 for a model without affine layers), W = D + 2 as in pa_affine_batch_run_dt_ends and
 * nseg = s' / S + 1, all taken from the bound s' before anything runs, none shared and none resized after the checkpoint pass:
 *   (E + 2) L W 4  the ring,  (nseg - 1) E L W 4  the checkpoint rows,  (E + S + 1) L W 4  the segment buffer,
 *   (|a| + |b|) rounded up to 16  the ops,  and 40  the walk state and the fills' counters.
 * The pairs run most expensive first in chunks whose sum of these stays within PA_AFFINE_TRACE_BUDGET_MB (or a quarter of the free
 * device memory); a pair that alone exceeds it is PA_E_ARG naming the pair.  The wide-block rule of pa_affine_batch_run_dt applies
 * per launch, to the jobs of that launch.  A pair above s_max gets cost -1, start -1, end -1 and "" and takes no part in the rounds.
 * The batch's ends-free setting, pa_affine_batch_ends, the chain setting and every other route's results are neither read nor changed.
 * A NULL batch, a switch other than 0 and 1, or an s_max outside [0, 2^30) is PA_E_ARG.  forward_ms, refill_ms, walk_ms (optional):
 * HIP-event times of the checkpoint passes, the fills and the walks, summed over chunks and rounds.  Every output pointer may be NULL.
 * cigar_out[p] is malloc'ed (pa_free_cigars); on error every cigar_out[p] is NULL.  pa_affine_batch_dt_info then reports the
 * checkpoint pass. */
int pa_affine_batch_align_dt_seg(pa_affine_batch* ab, int free_start, int free_end, int32_t s_max, uint32_t seg, int32_t* cost_out,
                                 int64_t* start_out, int64_t* end_out, char** cigar_out, float* forward_ms, float* refill_ms,
                                 float* walk_ms);
/* The last pa_affine_batch_align_dt_seg: chunks, rounds (one fill launch and one walk launch each, summed over the chunks: per chunk
 * the largest cost / S + 1 among its found pairs), segment jobs (the sum of cost / S + 1 over the found pairs), front cells the fills
 * computed, and the largest chunk's device bytes by the formula above.  Every pointer may be NULL. */
void pa_affine_batch_dt_seg_info(const pa_affine_batch* ab, double* chunks, double* rounds, double* seg_jobs, double* refill_cells,
                                 double* bytes_max);
/* Plan shape of run() with chaining off (the setting does not change it): wavefronts launched, pairs packed into segments (|b| <= 1024), pairs on strips of their own, lanes carrying rows
 * of b (sum of ceil(max(|b|, 1) / 16)) over lanes launched (64 per wavefront and strip), and the chunks of the last align(). */
void pa_affine_batch_info(const pa_affine_batch* ab, double* waves, double* packed_pairs, double* strip_pairs, double* lane_use,
                          double* trace_chunks);
void pa_affine_batch_destroy(pa_affine_batch* ab);

#ifdef __cplusplus
}
#endif
#endif
