/*
 * pa_affine4_hip.h -- batched double-affine (two-piece gap cost) global alignment on the GPU (libastarpa_c_hip.so, MI355X / gfx950).
 *
 * What `NW::new(cm, false, false).align(a, b)` of pa-base-algos computes (the full-matrix AffineFront, nw/affine.rs, which is generic
 * over the number of layers) for many independent pairs under an AffineCost<4> with layers [insert, delete, insert, delete]:
 * AffineCost::double_affine(sub, open, extend, open2, extend2) (pa-affine-types/src/cost_model.rs) and its asymmetric forms.  A gap of
 * length L in layer k costs open[k] + L * extend[k], so an insertion of length L costs the minimum over the linear edge (L * ins, where
 * there is one) and the two insert layers, a deletion likewise.  Sequences are any bytes, compared for equality; empty sequences are
 * valid.  a and b are never swapped: I consumes b, D consumes a.
 *
 * CIGAR: the reference's backward walk from (|a|, |b|, main) to (0, 0, main), taking at every state the first parent in
 * EditGraph::iterate_parents order whose cost fits (main layer: diagonal, linear ins, linear del, close of layer 0, 1, 2, 3; affine
 * layers: open before extend), printed as AffineCigar::to_string() (= X I D, the affine ops of every layer as I / D, the count left out
 * when 1).  Ops of different layers, and linear against affine, stay separate elements (push_op merges equal ops only).
 *
 * The tiled traceback, pa_affine4_batch_align in bounded device memory, is declared in pa_affine4_tiled_hip.h, and chained strips (a
 * wavefront per strip of a long pair, in run and in the tiled traceback's checkpoint pass) in pa_affine4_chain_hip.h, and ends-free (semi-global) mode with
 * pa_affine4_batch_set_free_ends, pa_affine4_batch_ends and pa_affine4_batch_last_row in pa_affine4_ends_hip.h.  Not supported: layer lists
 * other than [insert, delete, insert, delete]; the diagonal-transition route is declared in pa_affine4_dt_hip.h and its segmented
 * traceback in pa_affine4_dt_seg_hip.h.
 *
 * Errors follow pa_bitpacking_hip.h: 0 or a negative PA_E_* code, pa_last_error() for the message.
 */
#ifndef PA_AFFINE4_HIP_H
#define PA_AFFINE4_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* One cost model.  sub, ins, del: in [1, 1000], or 0 for absent (the reference's None).  The layer kinds are fixed to [insert, delete,
 * insert, delete]; all four are required: every open[k] and extend[k] is in [1, 1000], and 0 there is PA_E_ARG. */
typedef struct pa_affine4_cost {
    int32_t sub, ins, del;
    int32_t open[4];
    int32_t extend[4];
} pa_affine4_cost;

/* Pair p aligns a[p] (a_len[p] bytes) against b[p].  For every pair, (|a| + |b| + 1) * (the largest edge cost, open + extend counted
 * as one) must be below 2^30, else PA_E_ARG naming the pair.  Arguments are checked before a device is touched.  trace != 0 allows
 * pa_affine4_batch_align.  A failed create returns NULL.  Zero pairs is valid.  With R = 16 rows of b per lane, pairs with |b| <= 64 R
 * run several to a wavefront (segments of g = 1, 2, 4 .. 64 lanes), sorted by (g, |a|); longer ones take a wavefront each, its strips of
 * 64 R rows one after the other through a boundary row of (|a| + 1) * 16 bytes (M, I1, I2 of the strip's last row per column). */
typedef struct pa_affine4_batch pa_affine4_batch;
pa_affine4_batch* pa_affine4_batch_create(const uint8_t* const* a, const size_t* a_len, const uint8_t* const* b, const size_t* b_len,
                                          size_t npairs, const pa_affine4_cost* cm, int trace);
/* Costs only.  cost_out[p] (may be NULL), kernel_ms (optional): HIP-event time of the forward kernel.  May be called again. */
int pa_affine4_batch_run(pa_affine4_batch* ab, int32_t* cost_out, float* kernel_ms);
/* Costs and CIGARs (trace batches only, else PA_E_ARG).  cigar_out[p] is malloc'ed (release with pa_free_cigars); on error every
 * cigar_out[p] is NULL.  The pairs run in chunks whose traceback codes (one byte per cell: (|a| + 1) * (rows + 1) bytes of a pair, rows
 * being |b| rounded up to its segment or to whole strips) stay within PA_AFFINE_TRACE_BUDGET_MB, or a quarter of the free device memory;
 * a pair whose codes alone exceed it is PA_E_ARG naming the pair.  forward_ms / trace_ms (optional): HIP-event time of the forward
 * kernels and of the walks, summed over the chunks. */
int pa_affine4_batch_align(pa_affine4_batch* ab, int32_t* cost_out, char** cigar_out, float* forward_ms, float* trace_ms);
/* Plan shape of run(): wavefronts launched, pairs packed into segments (|b| <= 64 R), pairs on strips of their own, lanes carrying rows
 * of b (sum of ceil(max(|b|, 1) / R)) over lanes launched (64 per wavefront and strip), and the chunks of the last align(). */
void pa_affine4_batch_info(const pa_affine4_batch* ab, double* waves, double* packed_pairs, double* strip_pairs, double* lane_use,
                           double* trace_chunks);
void pa_affine4_batch_destroy(pa_affine4_batch* ab);

#ifdef __cplusplus
}
#endif
#endif
