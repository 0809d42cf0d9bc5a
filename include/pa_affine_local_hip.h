/*
 * pa_affine_local_hip.h -- local (Smith-Waterman) alignment over a batch of pa_affine_hip.h: the best-matching part of a against the
 * best-matching part of b under the batch's gap-affine cost model and a bonus per match (libastarpa_c_hip.so, MI355X / gfx950).
 *
 * Definition.  cm is the batch's cost model (sub, ins, del, ins_open, ins_extend, del_open, del_extend as in pa_affine_hip.h), `match`
 * an integer in [1, 1000].  Scores are signed, i runs over a and j over b, an absent edge never wins, and NEG is a value no reachable
 * state holds:
 *   I(i,j) = max(H(i,j-1) - ins_open, I(i,j-1) - ins_extend)
 *   D(i,j) = max(H(i-1,j) - del_open, D(i-1,j) - del_extend)
 *   H(i,j) = max(0, H(i-1,j-1) + (a[i-1] == b[j-1] ? match : -sub), H(i,j-1) - ins, H(i-1,j) - del, I(i,j) - ins_extend, D(i,j) - del_extend)
 *   H(i,0) = H(0,j) = 0;  I, D = NEG on row 0 and column 0.
 * A gap of length L scores -(open + L extend), as in the global mode.
 *   Answer: the highest H(i,j) over 0 <= i <= |a|, 0 <= j <= |b|; on ties the lowest i, then the lowest j.  That cell is
 *           (a_end, b_end).  Score 0 is the empty alignment at (0, 0).
 *   Walk:   from (a_end, b_end, main).  In the main layer a state with H = 0 ends the walk, and its (i, j) is (a_start, b_start);
 *           otherwise the first parent that fits, in the order of pa_affine_batch_align: diagonal, linear insertion, linear deletion,
 *           close of the insert layer, close of the delete layer; in the affine layers open before extend.
 *   CIGAR:  the = X I D text of pa_affine_batch_align for a[a_start:a_end] against b[b_start:b_end]; the clipped flanks are not
 *           printed.  A non-empty CIGAR begins and ends with '='.
 * There is no counterpart in the reference (DEVIATIONS.md).
 *
 * `match` is an argument of the call.  The calls neither read nor change the batch's ends-free setting, its chain setting, what
 * pa_affine_batch_ends reports, or any other route's results.
 *
 * Limits.  A pair with match * min(|a|, |b|) >= 2^30 is refused (PA_E_ARG naming the pair) before anything is launched.
 *
 * Out of scope: tiled and chained forms, diagonal transition, and a banded form.  The double-affine batch (pa_affine4_hip.h) has the
 * same calls in a header of its own, pa_affine4_local_hip.h.
 */
#ifndef PA_AFFINE_LOCAL_HIP_H
#define PA_AFFINE_LOCAL_HIP_H

#include "pa_affine_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Every output pointer of these calls may be NULL.  PA_E_ARG, with pa_last_error() starting with the function's name, for a NULL batch,
 * a `match` outside [1, 1000] and a pair over the score bound.  A batch of zero pairs is valid. */

/* Scores and ends only: score_out[p], (a_end_out[p], b_end_out[p]) of every pair; kernel_ms receives the kernel time. */
int pa_affine_batch_run_local(pa_affine_batch* ab, int32_t match, int32_t* score_out, int64_t* a_end_out, int64_t* b_end_out, float* kernel_ms);
/* Trace batches only (else PA_E_ARG).  Also the starts and cigar_out[p], a malloc'ed string (pa_free_cigars); on error every
 * cigar_out[p] is NULL.  Runs in chunks whose traceback codes (one byte per cell) stay within PA_AFFINE_TRACE_BUDGET_MB or a quarter
 * of the free device memory; a pair whose codes alone exceed it is PA_E_ARG naming the pair.  forward_ms and trace_ms receive the
 * time of the fills and of the walks. */
int pa_affine_batch_align_local(pa_affine_batch* ab, int32_t match, int32_t* score_out, int64_t* a_start_out, int64_t* a_end_out,
                                int64_t* b_start_out, int64_t* b_end_out, char** cigar_out, float* forward_ms, float* trace_ms);
/* The last pa_affine_batch_align_local: its chunks, and the device bytes of traceback codes of the largest one. */
void pa_affine_batch_local_info(const pa_affine_batch* ab, double* chunks, double* bytes_max);

#ifdef __cplusplus
}
#endif
#endif
