/*
 * pa_affine4_dt_hip.h -- the diagonal-transition (WFA) route of the batched double-affine alignment (pa_affine4_hip.h): the cost, and
 * with a trace batch the CIGAR, of every pair whose cost is at most s_max, in time that grows with the cost instead of with |a| |b|
 * (libastarpa_c_hip.so, MI355X / gfx950).  The functions mirror pa_affine_batch_run_dt, _align_dt, _run_dt_ends, _align_dt_ends and
 * _dt_info of pa_affine_hip.h over the four layers [insert, delete, insert, delete].
 *
 * Semantics: DiagonalTransition over AffineCost<4> of pa-base-algos (dt.rs is generic over the number of layers).  For every cost s a
 * front keeps the furthest-reaching i of every diagonal i - j, for the main layer and each of the four.  Opening layer t costs open[t]
 * and consumes a byte, extending costs extend[t] and consumes one, closing costs extend[t]: a gap of length L in layer t costs
 * open[t] + L extend[t], as in pa_affine4_batch_run.  The pair is found at the first s whose main layer reaches (|a|, |b|).  There is no
 * retry inside: a pair whose cost exceeds s_max is "not found", cost -1.
 *
 * The cost is pa_affine4_batch_run's.  The CIGAR is that of a walk over the fronts: on the main layer the parents come in the order
 * substitution, linear insert, linear delete, close of layer 0, 1, 2, 3, and the first one that reaches the furthest point before the
 * match run is taken; inside a layer open comes before extend.  Gaps of different layers, and linear against affine, stay separate
 * elements as in pa_affine4_batch_align.  Where several optimal paths exist it may be another one than pa_affine4_batch_align's
 * (DEVIATIONS.md).
 *
 * Ends-free (the _ends functions): a is the text, b the pattern, consumed whole; free_start and free_end have the meaning of
 * pa_affine4_batch_set_free_ends (pa_affine4_ends_hip.h) but are arguments of the call: the batch's own setting, pa_affine4_batch_ends
 * and the chain setting are neither read nor changed.  Cost and end are those of the ends-free pa_affine4_batch_run; start and the
 * CIGAR are the walk's own.  With both switches 0 the results are run_dt's and align_dt's with start = 0 and end = |a|.
 *
 * Device memory: per pair W = diagonals at the bound + 2 values of 4 bytes per row.  The cost-only calls keep a ring per layer,
 * (E + 1) + sum of (extend[t] + 1) rows and one more, E the largest of sub, ins, del and open[0..3]: 36 rows under
 * open = {6, 6, 24, 24}, extend = {2, 2, 1, 1}, sub = 4.  The traced calls keep every front: 5 (s' + 1) + 1 rows and |a| + |b| bytes,
 * s' = min(s_max, the cost of deleting a and inserting b; of inserting b in the _ends calls with a switch on).  The pairs run in chunks
 * within PA_AFFINE_TRACE_BUDGET_MB (or a quarter of the free device memory); a pair that alone exceeds it is PA_E_ARG naming the pair.
 *
 * Errors follow pa_bitpacking_hip.h.  Every message starts with the function's name.  A NULL batch, an s_max outside [0, 2^30) and a
 * switch other than 0 or 1 are PA_E_ARG.  Every output pointer may be NULL.
 */
#ifndef PA_AFFINE4_DT_HIP_H
#define PA_AFFINE4_DT_HIP_H

#include "pa_affine4_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* cost_out[p]: the cost of pair p, or -1 where it exceeds s_max.  kernel_ms: the device time.  PA_E_ARG for a batch in ends-free mode
 * (pa_affine4_batch_set_free_ends): the _ends form takes the switches as arguments. */
int pa_affine4_batch_run_dt(pa_affine4_batch* ab, int32_t s_max, int32_t* cost_out, float* kernel_ms);
/* The same with free text ends.  end_out[p]: where the pattern ends in a, -1 for a pair that was not found. */
int pa_affine4_batch_run_dt_ends(pa_affine4_batch* ab, int free_start, int free_end, int32_t s_max, int32_t* cost_out, int64_t* end_out,
                                 float* kernel_ms);
/* Trace batches only.  cigar_out[p]: a NUL-terminated string to be released with pa_free_cigars, empty for a pair that was not found.
 * forward_ms and trace_ms: the device time of the fronts and of the walks. */
int pa_affine4_batch_align_dt(pa_affine4_batch* ab, int32_t s_max, int32_t* cost_out, char** cigar_out, float* forward_ms, float* trace_ms);
/* The same with free text ends: the CIGAR describes a[start_out[p]:end_out[p]] against b; both are -1 for a pair that was not found. */
int pa_affine4_batch_align_dt_ends(pa_affine4_batch* ab, int free_start, int free_end, int32_t s_max, int32_t* cost_out, int64_t* start_out,
                                   int64_t* end_out, char** cigar_out, float* forward_ms, float* trace_ms);
/* The last of the four calls above: pairs found and not found, chunks, front cells computed (5 layers x live diagonals x cost steps),
 * bytes compared while extending, device bytes of the largest chunk.  All 0 before the first call and for a NULL batch. */
void pa_affine4_batch_dt_info(const pa_affine4_batch* ab, double* found, double* not_found, double* chunks, double* front_cells,
                              double* extend_chars, double* bytes_max);

#ifdef __cplusplus
}
#endif
#endif
