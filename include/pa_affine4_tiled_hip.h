/*
 * pa_affine4_tiled_hip.h -- the tiled traceback of the batched double-affine alignment (pa_affine4_hip.h): the costs and CIGARs of
 * pa_affine4_batch_align, byte for byte, in bounded device memory.
 *
 * A cost-only pass keeps checkpoints; after that only the tiles a pair's path crosses are filled with traceback codes and walked, one
 * tile per pair and round.  With R = 16 rows of b per lane, a row tile is a strip of 64 R = 1024 rows (the one segment of H rows for a
 * pair with |b| <= 64 R), a column tile has C = tile_cols columns.  State (i, j) (i over a, j over b) lies in row tile 0 if j == 0, else
 * (j - 1) / (64 R), and in column tile 0 if i == 0, else (i - 1) / C.
 *
 * Device bytes of one pair, with H = |b| rounded up to its segment or to whole strips and strips = max(1, ceil(|b| / (64 R))):
 *     row checkpoints     (strips - 1) * (|a| + 1) * 16      {M, I1, I2, 0} of every strip's last row but the last strip's
 *   + column checkpoints  floor((|a| - 1) / C) * (H + 1) * 12, rounded up to 16 (0 for |a| == 0)
 *                         {M, D1, D2} of every row, row 0 included, after columns C, 2C, .. < |a|
 *   + one tile            (min(|a|, C) + 1) * (min(H, 64 R) + 1), rounded up to 16
 *   + ops                 |a| + |b|
 * A pair whose matrix is one tile stores no checkpoint.  At C = 1024 a 10 kbp pair takes about 3.6 MB (untiled: 102 MB), a 100 kbp
 * pair about 273 MB (untiled: 10 GB).
 */
#ifndef PA_AFFINE4_TILED_HIP_H
#define PA_AFFINE4_TILED_HIP_H

#include "pa_affine4_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* pa_affine4_batch_align by tiles (trace batches only, else PA_E_ARG).  tile_cols: 0 for the default of 1024, else in [64, 2^20], else
 * PA_E_ARG.  cigar_out[p] is malloc'ed (release with pa_free_cigars); on error every cigar_out[p] is NULL.  The pairs run in chunks
 * whose bytes (the sum above) stay within PA_AFFINE_TRACE_BUDGET_MB, or a quarter of the free device memory; a pair that alone exceeds
 * it is PA_E_ARG naming the pair.  A pair visits at most ceil(|a| / C) + ceil(max(|b|, 1) / (64 R)) tiles; one more is PA_E_INTERNAL.
 * forward_ms / refill_ms / walk_ms (optional): HIP-event time of the checkpoint pass, the tile fills and the walks, summed over the
 * chunks and rounds. */
int pa_affine4_batch_align_tiled(pa_affine4_batch* ab, uint32_t tile_cols, int32_t* cost_out, char** cigar_out, float* forward_ms,
                                 float* refill_ms, float* walk_ms);
/* Shape of the last pa_affine4_batch_align_tiled: chunks, rounds (one fill and one walk launch each), tile jobs, cells the fills
 * computed, and the bytes (the sum above) of the largest chunk.  Every pointer is optional. */
void pa_affine4_batch_tiled_info(const pa_affine4_batch* ab, double* chunks, double* rounds, double* tile_jobs, double* refill_cells,
                                 double* chunk_bytes_max);

#ifdef __cplusplus
}
#endif
#endif
