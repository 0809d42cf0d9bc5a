/*
 * pa_affine4_dt_seg_hip.h -- the segmented traceback of the diagonal-transition route of the batched double-affine alignment
 * (pa_affine4_dt_hip.h): the results of pa_affine4_batch_align_dt_ends in device memory that grows with the square root of the bound
 * instead of with the bound (libastarpa_c_hip.so, MI355X / gfx950).  The functions mirror pa_affine_batch_align_dt_seg and
 * _dt_seg_info of pa_affine_hip.h over the four layers [insert, delete, insert, delete].
 *
 * Results: cost, start, end and CIGAR of pa_affine4_batch_align_dt_ends(free_start, free_end, s_max), byte for byte, in every ends
 * setting; with both switches 0 those of pa_affine4_batch_align_dt with start = 0 and end = |a|.
 *
 * The argument.  Let E be the largest of sub, ins, del (those present) and open[0..3], e_t = extend[t], H = E + e_0 + e_1 + e_2 + e_3
 * and Ew = max(E, e_0, .., e_3).  Front s reads the main layer at s - {sub, ins, del, open[t]} >= s - E and layer t at s - e_t only,
 * and the walk reads the same fronts; one step of the walk lowers s by at most Ew, which can exceed E (an extend may cost more than
 * every open and every linear edge).  The costs are cut into segments of S >= Ew, segment c = [cS, cS + S - 1]: recomputing and
 * walking segment c needs, below cS, the last E fronts of the main layer and the last e_t of layer t, H rows, and the walk leaves
 * segment c into segment c - 1.  A checkpoint pass (the cost-only pass over the per-layer rings) keeps those H rows below every
 * segment; then, from the top segment down, each round is one launch that computes a segment's fronts again for every unfinished
 * pair and one that walks them.  There is no host round trip between the rounds.
 *
 * seg: 0, or the segment length S in [Ew, 2^30); anything else is PA_E_ARG with a message that names Ew.  seg = 0 takes per pair the
 * smallest S with 5 S^2 >= (s' + 1) H, raised to Ew, which balances the checkpoints against the segment buffer.  Either way a length
 * above max(Ew, s' + 1) is that: one segment.  s' = min(s_max, the cost of deleting a and inserting b; of inserting b with a switch on).
 *
 * Device bytes of a pair, with W = diagonals at the bound + 2 as in pa_affine4_dt_hip.h and nseg = s' / S + 1, all taken from the
 * bound s' before anything runs, none shared and none resized after the checkpoint pass; every row is W 4 bytes:
 *   (E + 1) + sum of (e_t + 1) + 1 rows  the rings (36 under open = {6, 6, 24, 24}, extend = {2, 2, 1, 1}, sub = 4),
 *   (nseg - 1) H rows  the checkpoints (H = 30 under that model),  H + 5 S + 1 rows  the segment buffer,
 *   (|a| + |b|) rounded up to 16  the ops,  and 40  the walk state and the fills' counters.
 * The pairs run most expensive first in chunks whose sum of these stays within PA_AFFINE_TRACE_BUDGET_MB (or a quarter of the free
 * device memory); a pair that alone exceeds it is PA_E_ARG naming the pair.  The wide-block rule of pa_affine4_batch_run_dt applies
 * per launch, to the jobs of that launch.  A pair above s_max gets cost -1, start -1, end -1 and "" and takes no part in the rounds.
 *
 * Errors follow pa_affine4_dt_hip.h.  Every message starts with the function's name.  A NULL batch, a batch without trace, an s_max
 * outside [0, 2^30), a switch other than 0 or 1, a bad seg and a pair over budget are PA_E_ARG.  Every output pointer may be NULL.
 * The batch's ends-free setting, pa_affine4_batch_ends, the chain setting and every other route's results are neither read nor
 * changed.
 */
#ifndef PA_AFFINE4_DT_SEG_HIP_H
#define PA_AFFINE4_DT_SEG_HIP_H

#include "pa_affine4_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Trace batches only.  forward_ms, refill_ms, walk_ms: HIP-event times of the checkpoint passes, the fills and the walks, summed over
 * chunks and rounds.  cigar_out[p] is malloc'ed (pa_free_cigars); on error every cigar_out[p] is NULL.  pa_affine4_batch_dt_info
 * then reports the checkpoint pass. */
int pa_affine4_batch_align_dt_seg(pa_affine4_batch* ab, int free_start, int free_end, int32_t s_max, uint32_t seg, int32_t* cost_out,
                                  int64_t* start_out, int64_t* end_out, char** cigar_out, float* forward_ms, float* refill_ms,
                                  float* walk_ms);
/* The last pa_affine4_batch_align_dt_seg: chunks, rounds (one fill launch and one walk launch each, summed over the chunks: per chunk
 * the largest cost / S + 1 among its found pairs), segment jobs (the sum of cost / S + 1 over the found pairs), front cells the fills
 * computed, and the largest chunk's device bytes by the formula above.  All 0 before the first call and for a NULL batch.  Every
 * pointer may be NULL. */
void pa_affine4_batch_dt_seg_info(const pa_affine4_batch* ab, double* chunks, double* rounds, double* seg_jobs, double* refill_cells,
                                  double* bytes_max);

#ifdef __cplusplus
}
#endif
#endif
