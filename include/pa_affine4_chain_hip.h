/*
 * pa_affine4_chain_hip.h -- the chained route of the batched double-affine alignment (pa_affine4_hip.h): long pairs on a wavefront per
 * strip (libastarpa_c_hip.so, MI355X / gfx950).
 *
 * Without it a pair with |b| > 1024 runs its strips of 1024 rows one after the other on a single wavefront.  With on = 1, in
 * pa_affine4_batch_run and in the checkpoint pass of pa_affine4_batch_align_tiled every strip of such a pair is a job of its own, run by
 * its own wavefront, and strip s + 1 reads the last row of strip s while strip s is still writing it; pairs with |b| <= 1024 keep their
 * plan and their launch.  Costs and CIGARs are byte for byte those of on = 0.  pa_affine4_batch_align (a code byte per cell) has no
 * chained form and ignores the setting.  The ends-free setting (pa_affine4_ends_hip.h) holds in the chained passes too.
 *
 * Memory: a chained pair needs (strips - 1) * (|a| + 1) * 16 bytes of boundary rows, strips = ceil(|b| / 1024): M, I1, I2 of the
 * strip's last row per column, written and read as two 8-byte halves.  pa_affine4_batch_run cuts the chained pairs into chunks whose
 * rows stay within PA_AFFINE_TRACE_BUDGET_MB (or a quarter of the free device memory), and a pair whose rows alone exceed it is PA_E_ARG
 * naming the pair and the route; pa_affine4_batch_align_tiled counts these rows among its checkpoints already
 * (pa_affine4_tiled_hip.h), so its chunks do not change.
 *
 * Bounded wait: a strip waits for its rows for a bounded time (30 s).  Should a strip never receive them, the call returns
 * PA_E_INTERNAL, pa_last_error() names the chained route, and every cost_out and cigar_out of that call is invalid.
 */
#ifndef PA_AFFINE4_CHAIN_HIP_H
#define PA_AFFINE4_CHAIN_HIP_H

#include "pa_affine4_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* on = 0 (the default) or 1; the setting holds for every later run and align_tiled.  A NULL batch, or a value other than 0 and 1, is
 * PA_E_ARG. */
int pa_affine4_batch_set_chain(pa_affine4_batch* ab, int on);
/* The setting, and the last chained pass (a run, or the checkpoint passes of an align_tiled, with chaining on): pairs and strip jobs it
 * ran chained, its chunks, and the largest chunk's boundary-row bytes.  Every pointer may be NULL. */
void pa_affine4_batch_chain_info(const pa_affine4_batch* ab, double* on, double* chain_pairs, double* chain_jobs, double* chunks,
                                 double* bnd_bytes_max);

#ifdef __cplusplus
}
#endif
#endif
