/*
 * pa_affine4_ends_hip.h -- ends-free (semi-global) mode of the batched double-affine alignment (pa_affine4_hip.h): the pattern b placed
 * in a window a of the text under two-piece gap costs (libastarpa_c_hip.so, MI355X / gfx950).
 *
 * The definition is pa_affine_batch_set_free_ends' (pa_affine_hip.h) over the four-layer recurrence of pa_affine4_hip.h.  a is the text
 * (columns), b the pattern (rows), always consumed whole.  Both switches default to 0, and with both at 0 every result is that of the
 * global mode.
 *   free_start = 1: M(i, 0) = 0 for every column i = 0 .. |a| (I1(i, 0) and I2(i, 0) stay absent; row 0's D1 and D2 feed only row 0's
 *                   M, so they do not matter).
 *   free_end = 1:   the cost is the minimum of M(i, |b|) over i = 0 .. |a|, and `end` the lowest i that reaches it; without it
 *                   end = |a|.
 * So the cost is the least global double-affine cost of (a[s:e], b) over the allowed s <= e (s = 0 unless free_start, e = |a| unless
 * free_end).  The CIGAR is the same first-parent walk over the same code bytes, from (end, |b|, main); with free_start it stops at the
 * first state (i, 0, main) it reaches and start = i, else it runs to (0, 0, main) and start = 0.  It describes a[start:end] against b:
 * the free flanks are not printed; gaps of different layers, and linear against affine, stay separate elements as in
 * pa_affine4_batch_align.  There is no counterpart in the reference (DEVIATIONS.md).
 *
 * The setting holds for pa_affine4_batch_run, pa_affine4_batch_align and pa_affine4_batch_align_tiled, and for run and align_tiled
 * under pa_affine4_batch_set_chain(1).  The ends-free values are never above the global ones, so the bound pa_affine4_batch_create
 * checks holds for them too.
 */
#ifndef PA_AFFINE4_ENDS_HIP_H
#define PA_AFFINE4_ENDS_HIP_H

#include "pa_affine4_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* free_start, free_end: 0 or 1 each.  The setting holds for every later run, align and align_tiled (all routes, chained or not) and
 * invalidates what pa_affine4_batch_ends would report.  A NULL batch, or a value other than 0 and 1, is PA_E_ARG. */
int pa_affine4_batch_set_free_ends(pa_affine4_batch* ab, int free_start, int free_end);
/* start and end of every pair in the last successful run, align or align_tiled under the current setting (either pointer may be NULL).
 * After a cost-only run start_out[p] is -1 when free_start is on and 0 otherwise.  Before any such call, or after a change of the
 * setting, PA_E_ARG. */
int pa_affine4_batch_ends(const pa_affine4_batch* ab, int64_t* start_out, int64_t* end_out);
/* The last row under the current setting: M(i, |b|) for i = 0 .. |a| of pair p to out + offsets[p]; offsets[p] == UINT64_MAX skips the
 * pair.  In global mode these are the costs of b against every prefix of a, the last one the pair's cost.  Runs a cost-only pass of its
 * own (never chained) over the pairs asked for, in chunks whose rows (4 bytes per column, device memory taken only here) stay within
 * PA_AFFINE_TRACE_BUDGET_MB or a quarter of the free device memory; a pair whose row alone exceeds it is PA_E_ARG naming the pair. */
int pa_affine4_batch_last_row(pa_affine4_batch* ab, int32_t* out, const uint64_t* offsets);

#ifdef __cplusplus
}
#endif
#endif
